"""GPU: RePaint resampling -- eod_renoise (csrc/sampler.hip) and `resample=(jump_length, jump_n_sample)` on EODiffusion.sampling /
sampling_scene and DDIMSampler.sample / ddim_sampling / sample_scene.

The kernel is held to an fp32 emulation bit for bit (tests/repaint_ref.py: numpy's correctly rounded sqrt for the two coefficients,
separately rounded torch fp32 multiplies and the add) and its in-register Philox form to eod_randn_philox followed by the given-noise
form; whole calls with injected draws to CPU loops assembled from oracle.sampler_ref's step functions, under the gate of
tests/test_gpu_sampling.py; the Philox keys, the scene samplers and `tile_batch` to bit equalities."""
import functools

import numpy as np
import pytest
import torch

from eo_diffusion_amd import _lib
from eo_diffusion_amd._lib import EodError
from eo_diffusion_amd.tiling import TilePlan
from tests import repaint_ref as RR
from tests.gpu_util import DEV
from tests.helpers import bits_equal, rel_l2, unet_cfgs
from tests.synth import rect_mask, synth_input, synth_state_dict
from tests.test_gpu_sampling import TRAJ_TOL, _model
from tests.test_gpu_scene import _diffusion, _scene_inputs, cut, stitch

pytestmark = pytest.mark.gpu


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _offset_by_4_bytes(t):
    """a copy of `t` that starts 4 bytes behind a 16-byte boundary of its own allocation"""
    base = torch.empty(t.numel() + 4, dtype=torch.float32, device=t.device)
    assert base.data_ptr() % 16 == 0
    v = base[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def renoise(x, noise, acp_from, acp_to, out=None, key=(0, 0, 0, 0)):
    """eod_renoise itself; returns (rc, out)"""
    from eo_diffusion_amd.engine import current_stream_ptr
    out = torch.empty_like(x) if out is None else out
    n = x.shape[0]
    rc = _lib.lib().eod_renoise(x.data_ptr(), _lib.ptr(noise), acp_from, acp_to, out.data_ptr(), n, x.numel() // n, *key,
                                current_stream_ptr(x.device))
    return rc, out


def philox(shape, seed, sample0, step, stream_id):
    from eo_diffusion_amd.engine import current_stream_ptr
    out = torch.empty(shape, dtype=torch.float32, device=DEV)
    _lib.check(_lib.lib().eod_randn_philox(out.data_ptr(), shape[0], out.numel() // shape[0], seed, sample0, step, stream_id,
                                           current_stream_ptr(out.device)), "eod_randn_philox")
    return out


ACP = (float(np.float32(0.9)), float(np.float32(0.3)))


# ------------------------------------------------------------------------------------------- 4. the kernel, given noise
@pytest.mark.parametrize("scale", [1e-30, 1.0, 1e30])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("chw", [3 * 16 * 16, 77, 4099, 3 * 64 * 64])
@pytest.mark.parametrize("unaligned", [False, True])
def test_renoise_with_given_noise_is_bit_exact(unaligned, chw, N, scale):
    x = (synth_input("rx", (N, chw), 3) * scale).to(DEV)
    z = synth_input("rz", (N, chw), 4).to(DEV)
    out = _nan(N, chw)
    if unaligned:
        x, out = _offset_by_4_bytes(x), _offset_by_4_bytes(out)
    for a_from, a_to in (ACP, (float(np.float32(0.37)), float(np.float32(0.37))), (float(np.float32(0.999)), float(np.float32(1e-6)))):
        rc, got = renoise(x, z, a_from, a_to, out=out)
        assert rc == 0
        want = RR.renoise(x.cpu(), z.cpu(), a_from, a_to)
        assert bool(torch.isfinite(got).all()) and bits_equal(got.cpu(), want), (a_from, a_to)


def test_renoise_refuses_a_move_down_the_chain_and_launches_nothing():
    x, z = synth_input("rx", (2, 64), 3).to(DEV), synth_input("rz", (2, 64), 4).to(DEV)
    for a_from, a_to in ((0.3, 0.9), (0.9, 0.0), (0.9, -0.1), (float("nan"), 0.5), (0.5, float("nan"))):
        out = _nan(2, 64)
        rc, _ = renoise(x, z, a_from, a_to, out=out)
        torch.cuda.synchronize()
        assert rc == -1 and bool(torch.isnan(out).all()), (a_from, a_to)
    with pytest.raises(EodError):
        m = _model("fp32", T=8)
        m._renoise(x.view(2, 1, 8, 8), 0.3, 0.9, z.view(2, 1, 8, 8))


# ------------------------------------------------------------------------------------------- 5. the kernel, Philox in registers
@pytest.mark.parametrize("seed", [7, 0x1234567887654321])
@pytest.mark.parametrize("N,chw,sample0", [(2, 3 * 16 * 16, 0), (3, 77, 5), (1, 4099, 1 << 20), (2, 3 * 64 * 64, 3)])
def test_renoise_philox_equals_randn_philox_then_given_noise(N, chw, sample0, seed):
    x = synth_input("px", (N, chw), 5).to(DEV)
    step, stream_id = 6, 2
    rc, got = renoise(x, None, *ACP, out=_nan(N, chw), key=(seed, sample0, step, stream_id))
    z = philox((N, chw), seed, sample0, step, stream_id)
    rc2, want = renoise(x, z, *ACP)
    assert rc == 0 and rc2 == 0 and bool(torch.isfinite(got).all())
    assert bits_equal(got, want)
    assert bits_equal(want.cpu(), RR.renoise(x.cpu(), z.cpu(), *ACP))
    xu = _offset_by_4_bytes(x)                                        # the scalar form of the same
    assert bits_equal(renoise(xu, None, *ACP, key=(seed, sample0, step, stream_id))[1], want)


@pytest.mark.parametrize("chw", [3 * 16 * 16, 77])
def test_renoise_philox_is_invariant_to_batch_sharding(chw):
    x = synth_input("sx", (4, chw), 6).to(DEV)
    full = renoise(x, None, *ACP, key=(11, 0, 3, 4))[1]
    lo = renoise(x[:2].contiguous(), None, *ACP, key=(11, 0, 3, 4))[1]
    hi = renoise(x[2:].contiguous(), None, *ACP, key=(11, 2, 3, 4))[1]
    assert bits_equal(torch.cat([lo, hi]), full)
    assert not bits_equal(renoise(x, None, *ACP, key=(11, 0, 3, 6))[1], full)


# ------------------------------------------------------------------------------------------- 6. moments
def test_renoise_philox_moments():
    """constant input c: out = ca c + cb z, z ~ N(0, 1) over n = 2^22 elements: the mean within six standard errors cb / sqrt(n) of
    ca c, the variance within six standard errors sqrt(2 / n) (relative) of cb^2"""
    n, c = 1 << 22, 0.5
    x = torch.full((1, n), c, dtype=torch.float32, device=DEV)
    rc, out = renoise(x, None, *ACP, key=(3, 0, 5, 2))
    assert rc == 0
    ca, cb = (float(v) for v in RR.renoise_coeffs(*ACP))
    o = out.double().cpu()
    mean, var = float(o.mean()), float(o.var(unbiased=True))
    print(f"mean {mean:.6f} (ca c = {ca * c:.6f}, 6 se = {6 * cb / n ** 0.5:.2e}); var / cb^2 - 1 = {var / cb ** 2 - 1:.2e} (6 se = {6 * (2 / n) ** 0.5:.2e})")
    assert abs(mean - ca * c) < 6 * cb / n ** 0.5
    assert abs(var / cb ** 2 - 1) < 6 * (2 / n) ** 0.5


# ------------------------------------------------------------------------------------------- 7. no jumps: today's bits
def _masked_cond(n, s, seed):
    return torch.cat([synth_input("cg", (n, 3, s, s), seed, uniform=True) * 2 - 1, rect_mask(n, s, s, seed)], 1)


@pytest.mark.parametrize("resample", [(3, 1), (8, 3), (50, 2)])
def test_a_walk_without_jumps_returns_todays_bits(resample):
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    T = 8
    m = _model("fp32", T=T, cond_type="sum")
    cond = _masked_cond(2, 16, 41).to(DEV)
    plain = m.sampling(2, device=DEV, cond=cond, rng="philox", seed=3, progress=False)
    assert torch.equal(m.sampling(2, device=DEV, cond=cond, rng="philox", seed=3, progress=False, resample=resample), plain)
    # DDIM, injected draws (S = 4 of T = 8: num_levels = 4 < 8)
    smp = DDIMSampler(m)
    S = 4
    kw = dict(x_T=synth_input("dx", (2, 3, 16, 16), 42), mask=cond[:, 3:], x0=cond[:, :3].contiguous(), log_every_t=1, progress=False,
              step_noises=synth_input("ds", (S, 2, 3, 16, 16), 42), mix_noises=synth_input("dm", (S, 2, 3, 16, 16), 42))
    smp.make_schedule(ddim_num_steps=S, ddim_eta=0.5, verbose=False)
    d_plain, i_plain = smp.ddim_sampling(None, (2, 3, 16, 16), **kw)
    d_res, i_res = smp.ddim_sampling(None, (2, 3, 16, 16), resample=resample, **kw)
    assert torch.equal(d_res, d_plain) and len(i_res["x_inter"]) == len(i_plain["x_inter"])
    assert all(torch.equal(a, b) for a, b in zip(i_res["pred_x0"], i_plain["pred_x0"]))
    # scenes
    s = 64
    ms = _diffusion("fp32x3", False, T, "sum")
    x_T, noises, scond = _scene_inputs(T, s + 24, 2 * s, 43, True)
    run = lambda **k: ms.sampling_scene((s + 24, 2 * s), True, DEV, cond=scond, overlap=16, seed=4, progress=False, **k)
    assert torch.equal(run(resample=resample), run())
    smps = DDIMSampler(ms)
    runs = lambda **k: smps.sample_scene(S, (s + 24, 2 * s), overlap=16, mask=scond[:, 3:], x0=scond[:, :3], eta=0.5, x_T=x_T,
                                         step_noises=noises[:S], mix_noises=noises[S:2 * S], progress=False, **k)[0]
    assert torch.equal(runs(resample=resample), runs())


# ------------------------------------------------------------------------------------------- 8. whole calls against the CPU loops
def _tiny():
    from eo_diffusion_amd.backbones.unet_openai import unet_param_shapes
    from oracle import unet_ref as UR
    cfg = unet_cfgs()["u_a0_tiny"]
    sd = synth_state_dict(unet_param_shapes(**cfg), 7)
    return lambda x, t: UR.unet_forward(sd, cfg, x, t)


def _ddpm_case(T, resample):
    n_eval, n_jump = (len(v) for v in RR.resample_schedule(T, *resample))
    return dict(x_T=synth_input("qx", (2, 3, 16, 16), 51), noises=synth_input("qn", (n_eval, 2, 3, 16, 16), 51),
                jump_noises=synth_input("qj", (n_jump, 2, 3, 16, 16), 51), cond=_masked_cond(2, 16, 51))


@functools.lru_cache(maxsize=None)
def _ddpm_reference(clip):
    from oracle import schedule as SCH
    c = _ddpm_case(20, (4, 3))
    assert len(c["noises"]) == 52 and len(c["jump_noises"]) == 8
    return RR.ddpm_resampled(SCH.eo_cosine_tables(20), _tiny(), c["x_T"], c["noises"], c["jump_noises"], 20, (4, 3), clip=clip,
                             gt=c["cond"][:, :3], mask=c["cond"][:, 3:])


@pytest.mark.parametrize("prec", ["fp32", "fp16", "fp32x3"])
@pytest.mark.parametrize("clip", [True, False])
def test_resampled_ddpm_call_vs_cpu_loop(clip, prec):
    """T = 20, resample = (4, 3): 52 evaluations, 8 jumps, RePaint mask"""
    c = _ddpm_case(20, (4, 3))
    m = _model(prec, T=20, cond_type="sum")
    out = m.sampling(2, clipped_reverse_diffusion=clip, device=DEV, cond=c["cond"].to(DEV), x_T=c["x_T"], noises=c["noises"],
                     jump_noises=c["jump_noises"], resample=(4, 3), progress=False)
    err = rel_l2(out.cpu(), _ddpm_reference(clip))
    print(f"resampled DDPM T = 20, (4, 3) [{prec}, clip {clip}]: rel-L2 vs the CPU loop = {err:.3e} (gate {TRAJ_TOL[prec]:g})")
    assert err < TRAJ_TOL[prec]


def _ddim_case(S, resample):
    n_eval, n_jump = (len(v) for v in RR.resample_schedule(S, *resample))
    cond = _masked_cond(2, 16, 52)
    return dict(x_T=synth_input("ex", (2, 3, 16, 16), 52), step_noises=synth_input("es", (n_eval, 2, 3, 16, 16), 52),
                mix_noises=synth_input("em", (n_eval, 2, 3, 16, 16), 52), jump_noises=synth_input("ej", (n_jump, 2, 3, 16, 16), 52),
                x0=cond[:, :3].contiguous(), mask=cond[:, 3:].contiguous())


@functools.lru_cache(maxsize=None)
def _ddim_reference(eta):
    from oracle import schedule as SCH
    c = _ddim_case(10, (2, 3))
    tb = SCH.eo_cosine_tables(20)
    steps = SCH.ddim_timesteps("uniform", 10, 20)
    dd = SCH.ddim_tables(tb["alphas_cumprod"], steps, eta)
    return steps, RR.ddim_resampled(tb, dd, steps, _tiny(), c["x_T"], c["step_noises"], c["jump_noises"], (2, 3), x0=c["x0"], mask=c["mask"],
                                    mix_noises=c["mix_noises"])


@pytest.mark.parametrize("prec", ["fp32", "fp16", "fp32x3"])
@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_resampled_ddim_call_vs_cpu_loop(eta, prec):
    """S = 10 of T = 20, resample = (2, 3) over the step indices: 26 evaluations, 8 jumps, mask / x0"""
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    c = _ddim_case(10, (2, 3))
    steps, (ref, ref_p0) = _ddim_reference(eta)
    smp = DDIMSampler(_model(prec, T=20))
    seen = []
    out, inter = smp.sample(10, 2, (3, 16, 16), eta=eta, verbose=False, progress=False, log_every_t=1, resample=(2, 3),
                            callback=seen.append, **{k: (v.to(DEV) if k in ("x0", "mask") else v) for k, v in c.items()})
    assert np.array_equal(np.asarray(smp.ddim_timesteps, np.int64), steps)
    assert seen == list(range(26)) and len(inter["x_inter"]) == 1 + 26          # every executed step is logged (log_every_t = 1)
    e_out, e_p0 = rel_l2(out.cpu(), ref), rel_l2(inter["pred_x0"][-1].cpu(), ref_p0)
    print(f"resampled DDIM 10 of 20, (2, 3) [{prec}, eta {eta}]: rel-L2 vs the CPU loop: out {e_out:.3e}, last pred_x0 {e_p0:.3e} (gate {TRAJ_TOL[prec]:g})")
    assert e_out < TRAJ_TOL[prec] and e_p0 < TRAJ_TOL[prec]


# ------------------------------------------------------------------------------------------- 9. the Philox keys
EVALS, MOVES = RR.EVALS, RR.MOVES  # T = 8, resample = (2, 2): every draw's (step, stream id), written out by hand


def _philox_loop(m, n, seed, offset, cond):
    shape = (n, 3, 16, 16)
    gt, mask = cond[:n, :3].contiguous(), cond[:n, 3][:, None].contiguous()
    acp = m.alphas_cumprod.tolist()
    x = m._philox(shape, DEV, seed, offset, 8, 0)
    for k, (i, sid) in enumerate(EVALS):
        noise = m._philox(shape, DEV, seed, offset, i, sid)
        t = torch.full((n,), i, dtype=torch.int64, device=DEV)
        x = m._repaint_mix(x, gt, mask, t, noise)
        x = m._reverse_diffusion_with_clip(x, t, noise)
        if k + 1 in MOVES:
            a, b, (step, sid2) = MOVES[k + 1]
            rc, x = renoise(x, None, acp[a], acp[b], key=(seed, offset, step, sid2))
            assert rc == 0
    return x


def test_philox_wiring_and_sharding():
    m = _model("fp32", T=8, cond_type="sum")
    cond = _masked_cond(4, 16, 61).to(DEV)
    full = m.sampling(4, device=DEV, cond=cond, rng="philox", seed=9, resample=(2, 2), progress=False)
    assert bool(torch.isfinite(full).all())
    assert torch.equal(full, _philox_loop(m, 4, 9, 0, cond))
    lo = m.sampling(2, device=DEV, cond=cond[:2], rng="philox", seed=9, sample_offset=0, resample=(2, 2), progress=False)
    hi = m.sampling(2, device=DEV, cond=cond[2:], rng="philox", seed=9, sample_offset=2, resample=(2, 2), progress=False)
    assert torch.equal(torch.cat([lo, hi]), full)
    assert not torch.equal(full, m.sampling(4, device=DEV, cond=cond, rng="philox", seed=9, progress=False))
    assert len({(s, i) for s, i in EVALS} | {key for _, _, key in MOVES.values()} | {(8, 0)}) == 14 + 3 + 1   # no two draws share a key


def test_philox_wiring_of_a_scene():
    """sampling_scene draws with the keys of sampling(): the scene is sample 0, its draws are scene-shaped"""
    s, seed = 64, 9
    m = _diffusion("fp32x3", False, 8, "sum")
    plan = TilePlan(s + 24, 2 * s, s, 16)
    shape = (1, 3, plan.H, plan.W)
    _, _, cond = _scene_inputs(1, plan.H, plan.W, 62, True)
    cond = cond.to(DEV)
    gt, mask = cond[:, :3].contiguous(), cond[:, 3:].contiguous()
    acp = m.alphas_cumprod.tolist()
    x = philox(shape, seed, 0, 8, 0)
    for k, (i, sid) in enumerate(EVALS):
        x = m._scene_step(x, i, philox(shape, seed, 0, i, sid), plan, 16, True, gt, mask)
        if k + 1 in MOVES:
            a, b, (step, sid2) = MOVES[k + 1]
            rc, x = renoise(x, None, acp[a], acp[b], key=(seed, 0, step, sid2))
            assert rc == 0
    got = m.sampling_scene((plan.H, plan.W), True, DEV, cond=cond, overlap=16, seed=seed, resample=(2, 2), progress=False)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, x)


# ------------------------------------------------------------------------------------------- 10. scenes
@pytest.mark.parametrize("prec", ["fp32x3", "fp16"])
def test_resampled_scene_with_overlap_0_equals_sampling_on_the_tiles(prec):
    s, T, rs = 64, 8, (2, 2)
    n_eval, n_jump = (len(v) for v in RR.resample_schedule(T, *rs))
    m = _diffusion(prec, False, T, "sum")
    plan = TilePlan(2 * s, 3 * s, s, 0)
    x_T, noises, cond = _scene_inputs(n_eval, plan.H, plan.W, 71, True)
    jn = synth_input("sj", (n_jump, 1, 3, plan.H, plan.W), 71)
    scene = m.sampling_scene((plan.H, plan.W), True, DEV, cond=cond, x_T=x_T, noises=noises, jump_noises=jn, resample=rs, progress=False)
    tiles = m.sampling(6, True, DEV, cond=cut(cond, plan), x_T=cut(x_T, plan), noises=torch.stack([cut(z, plan) for z in noises]),
                       jump_noises=torch.stack([cut(z, plan) for z in jn]), resample=rs, progress=False)
    assert bool(torch.isfinite(scene).all()) and torch.equal(scene, stitch(tiles, plan))
    plain = m.sampling_scene((plan.H, plan.W), True, DEV, cond=cond, x_T=x_T, noises=noises[:T], progress=False)
    assert not torch.equal(scene, plain)


@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_resampled_ddim_scene_with_overlap_0_equals_sample_on_the_tiles(eta):
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    s, S, rs = 64, 5, (2, 2)
    n_eval, n_jump = (len(v) for v in RR.resample_schedule(S, *rs))
    m = _diffusion("fp32x3", False, 20)
    plan = TilePlan(2 * s, 3 * s, s, 0)
    H, W = plan.H, plan.W
    x_T, stp, cond = _scene_inputs(n_eval, H, W, 72, True)
    mix, jn = synth_input("sm", (n_eval, 1, 3, H, W), 72), synth_input("sj", (n_jump, 1, 3, H, W), 72)
    x0, mask = cond[:, :3].contiguous(), cond[:, 3:].contiguous()
    smp = DDIMSampler(m)
    scene, inter = smp.sample_scene(S, (H, W), mask=mask.to(DEV), x0=x0.to(DEV), eta=eta, x_T=x_T, step_noises=stp, mix_noises=mix,
                                    jump_noises=jn, resample=rs, progress=False)
    per_tile = lambda zs: torch.stack([cut(z, plan) for z in zs])
    tiles, inter_t = smp.sample(S, 6, (3, s, s), mask=cut(mask, plan).to(DEV), x0=cut(x0, plan).to(DEV), eta=eta, x_T=cut(x_T, plan),
                                verbose=False, progress=False, step_noises=per_tile(stp), mix_noises=per_tile(mix),
                                jump_noises=per_tile(jn), resample=rs)
    assert torch.equal(scene, stitch(tiles, plan))
    assert len(inter["x_inter"]) == len(inter_t["x_inter"])
    assert torch.equal(inter["pred_x0"][-1], stitch(inter_t["pred_x0"][-1], plan))


def test_tile_batch_never_shows_in_a_resampled_scene():
    """overlap s / 4, a mask that crosses tile borders, Philox noise (the product path: eod_renoise generates the jump noise itself)"""
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    s, T = 64, 6
    m = _diffusion("fp32x3", False, T, "sum")
    H, W = 3 * s - 40, 2 * s + 17
    plan = TilePlan(H, W, s, s // 4)
    mask = torch.ones(1, 1, H, W)
    mask[:, :, 30:110, 40:120] = 0.0                                # 1 = keep; the hole spans the borders at 48 / 64 of both axes
    holes = [float(mask[0, 0, y0:y0 + s, x0:x0 + s].min()) == 0.0 and float(mask[0, 0, y0:y0 + s, x0:x0 + s].max()) == 1.0
             for y0, x0 in plan.origins()]
    assert sum(holes) >= 4
    cond = torch.cat([synth_input("tg", (1, 3, H, W), 73, uniform=True) * 2 - 1, mask], 1)
    run = lambda tb, **k: m.sampling_scene((H, W), True, DEV, cond=cond, overlap=s // 4, tile_batch=tb, seed=5, resample=(2, 2), progress=False, **k)
    ref = run(16)
    assert bool(torch.isfinite(ref).all())
    assert torch.equal(run(1), ref) and torch.equal(run(4), ref) and torch.equal(run(16), ref)
    assert not torch.equal(m.sampling_scene((H, W), True, DEV, cond=cond, overlap=s // 4, seed=5, progress=False), ref)
    md = _diffusion("fp32x3", False, 20)
    smp = DDIMSampler(md)
    n_eval, n_jump = (len(v) for v in RR.resample_schedule(4, 2, 2))
    x_T, stp, _ = _scene_inputs(n_eval, H, W, 74, False)
    jn = synth_input("tj", (n_jump, 1, 3, H, W), 74)
    rund = lambda tb: smp.sample_scene(4, (H, W), overlap=s // 4, tile_batch=tb, mask=mask, x0=cond[:, :3], eta=1.0, x_T=x_T, step_noises=stp,
                                       mix_noises=stp.flip(0), jump_noises=jn, resample=(2, 2), progress=False)[0]
    refd = rund(16)
    assert bool(torch.isfinite(refd).all()) and torch.equal(rund(1), refd) and torch.equal(rund(4), refd)


def test_wrong_lengths_and_bad_arguments_are_refused_before_any_launch():
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    from eo_diffusion_amd.diffusion.model import EODiffusion

    class Never(torch.nn.Module):
        def forward(self, x, t, cond=None, y=None):
            raise AssertionError("the network was reached")

    s, T = 16, 8
    m = EODiffusion(Never(), timesteps=T, image_size=s, in_channels=3, device=DEV).to(DEV)
    smp = DDIMSampler(m)
    n_eval, n_jump = (len(v) for v in RR.resample_schedule(T, 2, 2))     # 14, 3
    z = lambda k, *shape: torch.zeros(k, *shape)
    img, scn = (2, 3, s, s), (1, 3, 32, 48)
    for kw in (dict(resample=(2, 2), jump_noises=z(n_jump + 1, *img)), dict(resample=(2, 2), jump_noises=z(n_jump - 1, *img)),
               dict(resample=(2, 2), noises=z(T, *img)), dict(resample=(0, 2)), dict(resample=(2, 0)), dict(resample=(2.5, 2)),
               dict(resample=3), dict(resample=(2, 2, 2)), dict(jump_noises=z(1, *img))):
        with pytest.raises(EodError):
            m.sampling(2, device=DEV, progress=False, **kw)
    for kw in (dict(resample=(2, 2), jump_noises=z(n_jump + 1, *scn)), dict(resample=(2, 2), noises=z(T, *scn)), dict(resample=(2, -1)),
               dict(jump_noises=[torch.zeros(scn)])):
        with pytest.raises(EodError):
            m.sampling_scene((32, 48), device=DEV, progress=False, **kw)
    n_eval_d, n_jump_d = (len(v) for v in RR.resample_schedule(4, 2, 2))  # S = 4 of T = 8: 6, 1
    for kw in (dict(resample=(2, 2), jump_noises=z(n_jump_d + 1, *img)), dict(resample=(2, 2), step_noises=z(4, *img)),
               dict(resample=(2, 2), mix_noises=z(n_eval_d + 1, *img)), dict(resample=(0, 1))):
        with pytest.raises(EodError):
            smp.sample(4, 2, (3, s, s), verbose=False, progress=False, **kw)
    for kw in (dict(resample=(2, 2), jump_noises=z(n_jump_d + 1, *scn)), dict(resample=(2, 2), step_noises=z(4, *scn)), dict(resample=(1, 0))):
        with pytest.raises(EodError):
            smp.sample_scene(4, (32, 48), progress=False, **kw)
