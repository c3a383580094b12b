"""GPU: whole-scene sampling -- eod_scene_gather / eod_scene_blend (csrc/scene.hip), eo_diffusion_amd/tiling.py,
EODiffusion.sampling_scene and DDIMSampler.sample_scene.

The multi-step checks are all BIT equalities (overlap 0 against today's samplers on the tiles; every tile_batch against every
other): across steps a one-ulp difference is amplified by the network and a tolerance says nothing.  The blend is held to a
plain-torch fp32 emulation that performs the same roundings in the same order (bit equality) AND to a float64 evaluation of the
same fp32 weights with the derivable bound  |err| <= (m + 1) u sum_i |w_i e_i|,  u = 2^-24, m = covering tiles: the term of
tile i carries the rounding of w = wy * wx, the rounding of p = w * e and at most m - 1 additions, (1 + u)^(m + 1) - 1 in all
(plus 2^-149 per operation where a result is subnormal)."""
import numpy as np
import pytest
import torch

from eo_diffusion_amd import _lib
from eo_diffusion_amd._lib import EodError
from eo_diffusion_amd.tiling import TilePlan, blend_tiles, gather_tiles, tile_slots, tiled_estimate
from tests.gpu_util import DEV
from tests.repaint_ref import walk_of
from tests.synth import rect_mask, synth_input, synth_state_dict

pytestmark = pytest.mark.gpu

# (L, tile, overlap) of the issue, as square 2-D plans, plus rectangular ones that pair an odd width with an even height
SQUARE = [(512, 256, 0), (600, 256, 32), (1000, 256, 64), (300, 256, 128), (1000, 64, 32), (257, 256, 16), (777, 64, 24)]
PLANS = [(L, L, t, o) for L, t, o in SQUARE] + [(300, 257, 256, 16), (128, 777, 64, 24), (777, 192, 64, 24), (145, 152, 64, 16)]
U = 2.0 ** -24


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def cut(scene, plan):
    """tiles by torch slicing: scene [1, C, H, W] -> [n_tiles, C, s, s]"""
    s = plan.tile
    return torch.cat([scene[:, :, y0:y0 + s, x0:x0 + s] for y0, x0 in plan.origins()]).contiguous()


def stitch(tiles, plan):
    """overlap 0 with H, W multiples of the tile: the tiles side by side"""
    s = plan.tile
    out = torch.empty((1, tiles.shape[1], plan.H, plan.W), dtype=tiles.dtype, device=tiles.device)
    for i, (y0, x0) in enumerate(plan.origins()):
        out[0, :, y0:y0 + s, x0:x0 + s] = tiles[i]
    return out


def blend_emulated(tiles, plan):
    """the blend in plain torch fp32 on the CPU, rounding for rounding: w = wy * wx, p = w * e, then left to right over the tiles in
    ascending index (the first covering tile's product starts the sum).  tiles [n, C, s, s] (cpu) -> [1, C, H, W]"""
    tiles = tiles.detach().float().cpu()
    s = plan.tile
    acc = torch.full((tiles.shape[1], plan.H, plan.W), float("nan"))
    seen = torch.zeros((plan.H, plan.W), dtype=torch.bool)
    for i, (y0, x0) in enumerate(plan.origins()):
        w = torch.from_numpy(plan.weight(i))                     # fp32 product of the fp32 axis weights
        iy, ix = divmod(i, plan.ntx)
        assert torch.equal(w, torch.from_numpy(plan.wy[iy])[:, None] * torch.from_numpy(plan.wx[ix])[None, :])
        p = w[None] * tiles[i]
        reg, sn = acc[:, y0:y0 + s, x0:x0 + s], seen[y0:y0 + s, x0:x0 + s]
        acc[:, y0:y0 + s, x0:x0 + s] = torch.where(sn[None], reg + p, p)
        seen[y0:y0 + s, x0:x0 + s] = True
    assert bool(seen.all())
    return acc[None]


def blend_float64(tiles, plan):
    """(sum_i w_i e_i, sum_i |w_i e_i|) in float64 with the SAME fp32 weight tables (their exact product), cpu"""
    tiles = tiles.detach().double().cpu()
    s = plan.tile
    tot = torch.zeros((tiles.shape[1], plan.H, plan.W), dtype=torch.float64)
    mag = torch.zeros_like(tot)
    for i, (y0, x0) in enumerate(plan.origins()):
        iy, ix = divmod(i, plan.ntx)
        w = torch.from_numpy(plan.wy[iy]).double()[:, None] * torch.from_numpy(plan.wx[ix]).double()[None, :]
        p = w[None] * tiles[i]
        tot[:, y0:y0 + s, x0:x0 + s] += p
        mag[:, y0:y0 + s, x0:x0 + s] += p.abs()
    return tot[None], mag[None]


def check_blend(out, tiles, plan, what=""):
    """bit equality with the emulation + the float64 bound of the module docstring; prints the figures before asserting"""
    out = out.cpu()
    assert bool(torch.isfinite(out).all()), f"{what}: an element was not written (NaN-filled output) or is not finite"
    emu = blend_emulated(tiles, plan)
    ref, mag = blend_float64(tiles, plan)
    m = torch.from_numpy(plan.cover_count()).double()[None, None]
    err = (out.double() - ref).abs()
    bound = (m + 1) * U * (1 + 1e-6) * mag + (m + 1) * 2.0 ** -149
    nbits = int((out.view(torch.int32) != emu.view(torch.int32)).sum())
    print(f"{what}: {plan}: elements differing from the fp32 emulation {nbits}; max err / bound vs float64 {float((err / bound).max()):.3f}")
    assert nbits == 0
    assert bool((err <= bound).all())


# ------------------------------------------------------------------------------------------------------------------ 1. gather
@pytest.mark.parametrize("C", [1, 3, 7, 13])
@pytest.mark.parametrize("H,W,tile,overlap", PLANS)
def test_gather_is_bit_exact(H, W, tile, overlap, C):
    plan = TilePlan(H, W, tile, overlap)
    scene = synth_input("scene", (1, C, H, W), 3).to(DEV)
    out = _nan(plan.n_tiles, C, tile, tile)
    got = gather_tiles(scene, plan, out=out)
    assert got.shape == (plan.n_tiles, C, tile, tile)
    assert torch.equal(got, cut(scene, plan))
    assert torch.equal(gather_tiles(scene[0], plan), got)          # [C, H, W] is accepted, too


def test_gather_of_an_unaligned_view_and_a_padded_buffer():
    """a scene that starts 4 bytes into its allocation (scalar loads) and an `out` with more slots than tiles"""
    plan = TilePlan(128, 192, 64, 16)
    base = synth_input("unal", (3 * 128 * 192 + 1,), 5).to(DEV)
    scene = base[1:].view(1, 3, 128, 192)
    chunk, slots = tile_slots(plan, 4)
    out = _nan(slots, 3, 64, 64)
    got = gather_tiles(scene, plan, out=out)
    assert torch.equal(got, cut(scene, plan))
    assert bool(torch.isnan(out[plan.n_tiles:]).all())             # the padding slots are the caller's


# ------------------------------------------------------------------------------------------------------------------ 2. blend
@pytest.mark.parametrize("scale", [1.0, 1e-30, 1e30])
@pytest.mark.parametrize("H,W,tile,overlap", PLANS)
def test_blend_is_bit_exact_and_within_the_float64_bound(H, W, tile, overlap, scale):
    plan = TilePlan(H, W, tile, overlap)
    C = 3 if H * W <= 700 * 700 else 1
    tiles = (synth_input("est", (plan.n_tiles, C, tile, tile), 11) * scale).to(DEV)
    out = blend_tiles(tiles, plan, out=_nan(1, C, H, W))
    check_blend(out, tiles, plan, f"scale {scale:g}")


@pytest.mark.parametrize("C", [1, 7, 13])
def test_blend_channel_counts(C):
    plan = TilePlan(145, 257, 64, 24)
    tiles = synth_input("estc", (plan.n_tiles, C, 64, 64), 12).to(DEV)
    check_blend(blend_tiles(tiles, plan, out=_nan(1, C, 145, 257)), tiles, plan, f"C = {C}")


@pytest.mark.parametrize("H,W,tile,overlap", PLANS)
def test_blend_of_a_constant_is_the_constant(H, W, tile, overlap):
    """partition of unity: constant estimate in -> the same constant out within m * 2^-23 relative (the 2-D weights sum to one
    within (2 m + 1) u / 2 -- tests/test_tiling.py -- and the blend adds one product rounding and m - 1 additions)"""
    plan = TilePlan(H, W, tile, overlap)
    k = 0.7316
    tiles = torch.full((plan.n_tiles, 2, tile, tile), k, dtype=torch.float32, device=DEV)
    out = blend_tiles(tiles, plan, out=_nan(1, 2, H, W)).cpu().double()
    m = torch.from_numpy(plan.cover_count()).double()[None, None]
    rel = (out - float(np.float32(k))).abs() / float(np.float32(k))
    print(f"{plan}: max relative deviation {float(rel.max()):.3e} (bound m 2^-23, m <= {int(m.max())})")
    assert bool((rel <= m * 2.0 ** -23).all())
    single = (m == 1).expand_as(out)
    assert bool((out[single] == float(np.float32(k))).all())       # one covering tile: weight exactly 1.0f, value unchanged


def test_blend_with_overlap_0_is_a_bitwise_copy():
    plan = TilePlan(128, 192, 64, 0)
    tiles = synth_input("est0", (6, 3, 64, 64), 13).to(DEV)
    tiles[0, 0, 0, 0] = -0.0
    out = blend_tiles(tiles, plan, out=_nan(1, 3, 128, 192))
    assert torch.equal(out.view(torch.int32), stitch(tiles, plan).view(torch.int32))
    assert torch.equal(gather_tiles(out, plan), tiles)


# -------------------------------------------------------------------------------------------- models shared by the sampler tests
_UNETS = {}


def _unet(prec, attn, s=64, in_ch=3, num_classes=None):
    from eo_diffusion_amd.backbones.unet_openai import UNetModel, unet_param_shapes
    key = (prec, attn, s, in_ch, num_classes)
    if key not in _UNETS:
        cfg = dict(image_size=s, in_channels=in_ch, model_channels=32, out_channels=3, num_res_blocks=1,
                   attention_resolutions=[4] if attn else [], channel_mult=[1, 2, 2] if attn else [1, 2], num_heads=4 if attn else 1)
        if num_classes:
            cfg["num_classes"] = num_classes
        u = UNetModel(**cfg).set_precision(prec)
        u.load_state_dict(synth_state_dict(unet_param_shapes(**cfg), 7))
        _UNETS[key] = u.to(DEV).eval()
    return _UNETS[key]


def _diffusion(prec, attn=False, T=8, cond_type=None, s=64, in_ch=3, num_classes=None):
    from eo_diffusion_amd.diffusion.model import EODiffusion
    return EODiffusion(_unet(prec, attn, s, in_ch, num_classes), timesteps=T, image_size=s, in_channels=3, cond_type=cond_type,
                       device=DEV).to(DEV).eval()


def _scene_inputs(T, H, W, seed, masked):
    x_T = synth_input("sx", (1, 3, H, W), seed)
    noises = synth_input("sn", (T, 1, 3, H, W), seed)
    cond = None
    if masked:
        cond = torch.cat([synth_input("sg", (1, 3, H, W), seed, uniform=True) * 2 - 1, rect_mask(1, H, W, seed)], 1)
    return x_T, noises, cond


# ---------------------------------------------------------------------------------------- 3. overlap 0 is today's sampler
@pytest.mark.parametrize("attn", [False, True])
@pytest.mark.parametrize("prec", ["fp32x3", "fp16"])
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("masked", [False, True])
def test_overlap_0_equals_sampling_on_the_tiles(masked, clip, prec, attn):
    s, T = 64, 8
    m = _diffusion(prec, attn, T, "sum" if masked else None)
    plan = TilePlan(2 * s, 3 * s, s, 0)
    x_T, noises, cond = _scene_inputs(T, plan.H, plan.W, 21, masked)
    scene = m.sampling_scene((plan.H, plan.W), clip, DEV, cond=cond, x_T=x_T, noises=noises, progress=False)
    tiles = m.sampling(6, clip, DEV, cond=None if cond is None else cut(cond, plan), x_T=cut(x_T, plan),
                       noises=torch.stack([cut(noises[k], plan) for k in range(T)]), progress=False)
    assert scene.shape == (1, 3, plan.H, plan.W) and bool(torch.isfinite(scene).all())
    assert torch.equal(scene, stitch(tiles, plan))
    if not attn and clip:                                            # a padded last chunk (4 + 2 tiles + 2 copies) changes nothing
        again = m.sampling_scene((plan.H, plan.W), clip, DEV, cond=cond, x_T=x_T, noises=noises, tile_batch=4, progress=False)
        assert torch.equal(again, scene)


@pytest.mark.parametrize("prec", ["fp32x3", "fp16"])
@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_overlap_0_ddim_equals_sample_on_the_tiles(eta, prec):
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    s, S = 64, 5
    m = _diffusion(prec, False, 20)
    plan = TilePlan(2 * s, 3 * s, s, 0)
    H, W = plan.H, plan.W
    x_T, step_noises, cond = _scene_inputs(S, H, W, 22, True)
    mix_noises = synth_input("sm", (S, 1, 3, H, W), 22)
    x0, mask = cond[:, :3].contiguous(), cond[:, 3:].contiguous()
    smp = DDIMSampler(m)
    scene, inter = smp.sample_scene(S, (H, W), mask=mask.to(DEV), x0=x0.to(DEV), eta=eta, x_T=x_T, step_noises=step_noises,
                                    mix_noises=mix_noises, progress=False)
    tiles, inter_t = smp.sample(S, 6, (3, s, s), mask=cut(mask, plan).to(DEV), x0=cut(x0, plan).to(DEV), eta=eta,
                                x_T=cut(x_T, plan), verbose=False, progress=False,
                                step_noises=torch.stack([cut(step_noises[k], plan) for k in range(S)]),
                                mix_noises=torch.stack([cut(mix_noises[k], plan) for k in range(S)]))
    assert torch.equal(scene, stitch(tiles, plan))
    assert len(inter["x_inter"]) == len(inter_t["x_inter"])
    assert torch.equal(inter["pred_x0"][-1], stitch(inter_t["pred_x0"][-1], plan))
    # unmasked, too (eta decides whether the injected noise matters)
    scene, _ = smp.sample_scene(S, (H, W), eta=eta, x_T=x_T, step_noises=step_noises, progress=False)
    tiles, _ = smp.sample(S, 6, (3, s, s), eta=eta, x_T=cut(x_T, plan), verbose=False, progress=False,
                          step_noises=torch.stack([cut(step_noises[k], plan) for k in range(S)]))
    assert torch.equal(scene, stitch(tiles, plan))


@pytest.mark.parametrize("masked", [False, True])
def test_a_scene_of_one_tile_equals_sampling_1(masked):
    s, T = 64, 8
    m = _diffusion("fp32x3", False, T, "sum" if masked else None)
    x_T, noises, cond = _scene_inputs(T, s, s, 23, masked)
    for overlap in (0, 16):
        scene = m.sampling_scene((s, s), True, DEV, cond=cond, x_T=x_T, noises=noises, overlap=overlap, progress=False)
        assert torch.equal(scene, m.sampling(1, True, DEV, cond=cond, x_T=x_T, noises=noises, progress=False))


# ------------------------------------------------------------------------------------------------ 4. chunking never shows
@pytest.mark.parametrize("prec,masked", [("fp32x3", True), ("fp16", False)])
def test_tile_batch_never_shows_and_philox_is_reproducible(prec, masked):
    s, T = 64, 6
    m = _diffusion(prec, False, T, "sum" if masked else None)
    H, W = 3 * s - 40, 2 * s + 17                                    # odd width, shifted last tiles: 3 x 3 = 9 tiles
    _, _, cond = _scene_inputs(T, H, W, 24, masked)
    run = lambda tb, seed=5: m.sampling_scene((H, W), True, DEV, cond=cond, overlap=s // 4, tile_batch=tb, seed=seed, progress=False)
    ref = run(16)
    assert ref.shape == (1, 3, H, W) and bool(torch.isfinite(ref).all())
    assert torch.equal(run(1), ref) and torch.equal(run(4), ref)
    assert torch.equal(run(16), ref)                                 # a second run, the same seed
    assert not torch.equal(run(16, seed=6), ref)
    torch.manual_seed(3)
    a = m.sampling_scene((H, W), True, DEV, cond=cond, overlap=s // 4, rng="torch", progress=False)
    torch.manual_seed(3)
    b = m.sampling_scene((H, W), True, DEV, cond=cond, overlap=s // 4, tile_batch=2, rng="torch", progress=False)
    assert torch.equal(a, b) and not torch.equal(a, ref)


def test_ddim_tile_batch_never_shows():
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    s, S = 64, 4
    m = _diffusion("fp32x3", False, 20)
    H, W = 2 * s + 24, 2 * s + 17
    x_T, step_noises, cond = _scene_inputs(S, H, W, 25, True)
    smp = DDIMSampler(m)
    run = lambda tb: smp.sample_scene(S, (H, W), overlap=16, tile_batch=tb, mask=cond[:, 3:], x0=cond[:, :3], eta=1.0, x_T=x_T,
                                      step_noises=step_noises, mix_noises=step_noises.flip(0), progress=False)[0]
    ref = run(16)
    assert bool(torch.isfinite(ref).all()) and torch.equal(run(1), ref) and torch.equal(run(4), ref)


def test_baseline_sized_scene():
    """A0 (base 128, mults [1, 2, 3, 4]) at s = 256 on a 512 x 768 scene, overlap 32 (3 x 4 = 12 tiles), 3 steps: finite,
    deterministic, the same for every tile_batch"""
    from eo_diffusion_amd.backbones.unet_openai import UNetModel
    from eo_diffusion_amd.diffusion.model import EODiffusion
    torch.manual_seed(0)
    u = UNetModel(256, in_channels=3, model_channels=128, out_channels=3, num_res_blocks=1, attention_resolutions=[],
                  channel_mult=[1, 2, 3, 4], num_heads=1).set_precision("fp32x3")
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for p in u.parameters():
            if p.dim() > 1 and float(p.abs().max()) == 0.0:
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    m = EODiffusion(u, timesteps=3, image_size=256, in_channels=3, device=DEV).to(DEV).eval()
    run = lambda tb: m.sampling_scene((512, 768), True, DEV, overlap=32, tile_batch=tb, seed=9, progress=False)
    a = run(16)
    assert a.shape == (1, 3, 512, 768) and bool(torch.isfinite(a).all())
    assert torch.equal(run(16), a)
    assert torch.equal(run(4), a) and torch.equal(run(5), a)        # 5: a padded last chunk (12 = 5 + 5 + 2 + 3 copies)


# ------------------------------------------------------------------------------------------ 4b. the order of torch's draws
@pytest.mark.parametrize("resample", [None, (2, 2)])
@pytest.mark.parametrize("masked", [False, True])
def test_sampling_scene_draws_from_torch_in_loop_order(masked, resample):
    """rng="torch": x_T on the CPU generator; on the device generator one scene-sized draw per evaluation (mix AND update) and one
    per jump, in walk order -- drawn by hand, injected, and compared with the sampler drawing for itself from the same seed"""
    s, T = 64, 8
    H, W = s + 24, 2 * s
    shape = (1, 3, H, W)
    m = _diffusion("fp32x3", False, T, "sum" if masked else None)
    _, _, cond = _scene_inputs(1, H, W, 28, masked)
    visits, jump_after = walk_of(T, resample)
    torch.manual_seed(19)
    x_T = torch.randn(shape)
    noises, jump_noises = [], []
    for k in range(len(visits)):
        noises.append(torch.randn(shape, device=DEV))
        if k + 1 in jump_after:
            jump_noises.append(torch.randn(shape, device=DEV))
    run = lambda **kw: m.sampling_scene((H, W), True, DEV, cond=cond, overlap=16, rng="torch", resample=resample, progress=False, **kw)
    want = run(x_T=x_T, noises=noises, jump_noises=jump_noises if resample else None)
    torch.manual_seed(19)
    got = run()
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)
    assert len(jump_noises) == (3 if resample else 0)


@pytest.mark.parametrize("eta", [0.0, 1.0])
@pytest.mark.parametrize("resample", [None, (2, 2)])
@pytest.mark.parametrize("masked", [False, True])
def test_sample_scene_draws_from_torch_in_loop_order(masked, resample, eta):
    """all on the device generator: x_T; per evaluation the mix noise (only with a mask) and, after the estimate, the eta-noise
    ONLY where sigma_t != 0 (eta = 0: no step draw at all); one per jump.  No unused draw."""
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    s, S = 64, 4
    H, W = s + 24, 2 * s
    shape = (1, 3, H, W)
    smp = DDIMSampler(_diffusion("fp32x3", False, 8))
    _, _, cond = _scene_inputs(1, H, W, 29, True)
    kw = dict(overlap=16, eta=eta, progress=False, log_every_t=1, resample=resample)
    if masked:
        kw["x0"], kw["mask"] = cond[:, :3].contiguous().to(DEV), cond[:, 3:].contiguous().to(DEV)
    smp.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=False)
    drawn = [float(v) != 0.0 for v in smp.ddim_sigmas]
    assert len(drawn) == S and all(drawn) == (eta != 0.0) and any(drawn) == (eta != 0.0)
    visits, jump_after = walk_of(S, resample)
    torch.manual_seed(20)
    x_T = torch.randn(shape, device=DEV)
    mix, stp, jn = [], [], []
    for k, index in enumerate(visits):
        if masked:
            mix.append(torch.randn(shape, device=DEV))
        if drawn[index]:
            stp.append(torch.randn(shape, device=DEV))
        if k + 1 in jump_after:
            jn.append(torch.randn(shape, device=DEV))
    want, want_i = smp.sample_scene(S, (H, W), x_T=x_T, step_noises=stp if eta else None, mix_noises=mix if masked else None,
                                    jump_noises=jn if resample else None, **kw)
    torch.manual_seed(20)
    got, got_i = smp.sample_scene(S, (H, W), **kw)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)
    assert len(got_i["pred_x0"]) == len(want_i["pred_x0"]) == 1 + len(visits)
    assert all(torch.equal(a, b) for a, b in zip(got_i["pred_x0"], want_i["pred_x0"]))
    assert len(stp) == (len(visits) if eta else 0) and len(jn) == (1 if resample else 0)


# ------------------------------------------------------------------------ 5. one step against an emulation from public pieces
@pytest.mark.parametrize("prec", ["fp32x3", "fp16"])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("clip", [True, False])
@torch.no_grad()
def test_one_ddpm_step_vs_emulation(clip, masked, prec):
    s, T, i = 64, 8, 5
    m = _diffusion(prec, True, T, "sum" if masked else None)
    H, W = 3 * s - 40, 2 * s + 17
    plan = TilePlan(H, W, s, s // 4)
    x_t, noises, cond = _scene_inputs(1, H, W, 26, masked)
    x_t, noise = x_t.to(DEV), noises[0].to(DEV)
    gt = mask = None
    if masked:
        gt, mask = cond[:, :3].contiguous().to(DEV), cond[:, 3:].contiguous().to(DEV)
    got = m._scene_step(x_t, i, noise, plan, 4, clip, gt, mask)
    # the emulation: public pieces and torch only
    t1 = torch.full((1,), i, dtype=torch.int64, device=DEV)
    x_in = m._repaint_mix(x_t, gt, mask, t1, noise) if masked else x_t
    e_tiles = m.model(cut(x_in, plan), torch.full((plan.n_tiles,), i, dtype=torch.int64, device=DEV))
    e_scene = blend_emulated(e_tiles, plan).to(DEV)
    want = m._ddpm_update(x_in, e_scene, noise, t1, clip)
    assert torch.equal(got, want)
    # the estimate of the scene path itself, against float64
    t4 = torch.full((4,), i, dtype=torch.int64, device=DEV)
    check_blend(tiled_estimate(x_in, plan, 4, lambda x, lo: m.model(x, t4)), e_tiles, plan, "one step")


@pytest.mark.parametrize("masked", [False, True])
@torch.no_grad()
def test_one_ddim_step_vs_emulation(masked):
    """S = 1: the whole call is one step (eta = 1: sigma_t != 0, the injected noise matters)"""
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    from eo_diffusion_amd.engine import current_stream_ptr
    s = 64
    m = _diffusion("fp32x3", False, 20)
    H, W = 2 * s + 24, 2 * s + 17
    plan = TilePlan(H, W, s, 16)
    x_T, nz, cond = _scene_inputs(1, H, W, 27, True)
    mix = synth_input("mx", (1, 1, 3, H, W), 27)
    smp = DDIMSampler(m)
    kw = dict(mask=cond[:, 3:].to(DEV), x0=cond[:, :3].contiguous().to(DEV), mix_noises=mix) if masked else {}
    got, inter = smp.sample_scene(1, (H, W), overlap=16, tile_batch=4, eta=1.0, x_T=x_T, step_noises=nz, progress=False, **kw)
    assert smp.ddim_timesteps.shape[0] == 1
    step = int(smp.ddim_timesteps[0])
    x = x_T.to(DEV)
    if masked:
        x = m._repaint_mix(x, kw["x0"], kw["mask"], torch.full((1,), step, dtype=torch.int64, device=DEV), mix[0].to(DEV))
    e_tiles = m.model(cut(x, plan), torch.full((plan.n_tiles,), step, dtype=torch.int64, device=DEV))
    e = blend_emulated(e_tiles, plan).to(DEV)
    z = nz[0].to(DEV)
    want, p0 = torch.empty_like(x), torch.empty_like(x)
    _lib.check(_lib.lib().eod_ddim_step(x.data_ptr(), e.data_ptr(), z.data_ptr(), float(smp.ddim_alphas[0]), float(smp.ddim_alphas_prev[0]),
                                        float(smp.ddim_sigmas[0]), float(smp.ddim_sqrt_one_minus_alphas[0]), 1.0, want.data_ptr(),
                                        p0.data_ptr(), x.numel(), current_stream_ptr(x.device)), "eod_ddim_step")
    assert float(smp.ddim_sigmas[0]) != 0.0
    assert torch.equal(got, want) and torch.equal(inter["pred_x0"][-1], p0)


# ------------------------------------------------------------------------------------------------------------------ 6. seams
def _ramp_estimate(plan, a, tile_batch=4):
    """blended estimate of a stub network e = x + a * (lx + ly) (tile-local position) on a zero scene"""
    s = plan.tile
    l = torch.arange(s, dtype=torch.float32, device=DEV)
    ramp = (a * (l[None, :] + l[:, None]))[None, None]
    scene = torch.zeros((1, 1, plan.H, plan.W), dtype=torch.float32, device=DEV)
    return tiled_estimate(scene, plan, tile_batch, lambda x, lo: x + ramp).cpu().double()[0, 0]


def test_seams():
    """The weights are applied where they should be, not merely normalised.  A stub whose output is a ramp a * (lx + ly) of the
    TILE-LOCAL position jumps by a * (s - 1) at every tile border when the tiles are only laid side by side (overlap 0).
    Blended: the weights are separable and sum to one per axis, so e(y, x) = f(x) + f(y) with, where two tiles i, i + 1 at
    distance d = s - o share o pixels,  f(x) = a (x - x_i) - a d w_{i+1}(x)  and  w_{i+1} = (k + 1) / (o + 1):  the step between
    neighbouring pixels is  a (1 - d / (o + 1))  in the shared range,  a  in a tile's interior, and
    a (1 - d / (o + 1)) + (second order) across the range's two ends.  With overlap = s / 2 (d <= o + 1) every step is within
    the ramp's own slope times one pixel: |step| <= a.  With overlap = s / 4 the bound is a max(1, d / (o + 1) - 1)."""
    s, a = 64, 0.125                                                 # (a power of two: the ramp values are exact)
    jump0 = _ramp_estimate(TilePlan(2 * s, 3 * s, s, 0), a)
    assert float(jump0.diff(dim=1).abs().max()) == a * (s - 1) and float(jump0.diff(dim=0).abs().max()) == a * (s - 1)
    slack = 2 * (4 + 1) * U * (2 * a * (s - 1))                       # two neighbouring values, each off by at most (m + 1) u |e|, m <= 4
    half = _ramp_estimate(TilePlan(2 * s, 3 * s, s, s // 2), a)     # origins 0, 32, 64 | 0, 32, ..., 128: no shifted tile
    dx, dy = float(half.diff(dim=1).abs().max()), float(half.diff(dim=0).abs().max())
    print(f"overlap s/2: max step {dx:.4f} / {dy:.4f} along x / y (slope {a}, overlap-0 jump {a * (s - 1)})")
    assert dx <= a + slack and dy <= a + slack
    plan = TilePlan(160, 208, s, s // 4)                             # origins 0, 48, 96 | 0, 48, 96, 144: two tiles at most per axis
    assert int(plan.cover_count().max()) == 4
    quarter = _ramp_estimate(plan, a)
    d, o = s - s // 4, s // 4
    bound = a * max(1.0, d / (o + 1) - 1.0)
    dx, dy = float(quarter.diff(dim=1).abs().max()), float(quarter.diff(dim=0).abs().max())
    print(f"overlap s/4: max step {dx:.4f} / {dy:.4f}, bound {bound:.4f}")
    assert dx <= bound + slack and dy <= bound + slack
    # and the blended ramp is what the formula says in the middle of a shared range (x = 48 + 8: tiles 0 and 1, k = 8)
    k = 8
    w1 = (k + 1) / (o + 1)
    want = (1 - w1) * a * (48 + k) + w1 * a * k
    assert abs(float(quarter[5, 48 + k]) - (want + a * 5)) <= 1e-5


# ------------------------------------------------------------------------------ 7. known region, labels, guidance reach every tile
def test_repaint_keeps_the_known_region_of_a_scene():
    """as test_repaint_keeps_known_region_statistics per image: at the last step (t = 0) the kept region of the UNet's input is
    sqrt(acp_0) * gt -- for every tile of the scene, through the scene loop, with a denoiser that predicts zero"""
    from eo_diffusion_amd.diffusion.model import EODiffusion

    class Echo(torch.nn.Module):
        def forward(self, x, t, cond=None, y=None):
            self.last_x, self.last_t = x.clone(), t.clone()
            return torch.zeros_like(x)

    s, H, W = 16, 40, 57
    m = EODiffusion(Echo(), timesteps=4, image_size=s, in_channels=3, cond_type="sum", device=DEV).to(DEV)
    plan = TilePlan(H, W, s, 4)
    gt0 = synth_input("rk", (1, 3, H, W), 71, uniform=True).to(DEV)
    mask = rect_mask(1, H, W, 71).to(DEV)
    m.sampling_scene((H, W), True, DEV, cond=torch.cat([gt0, mask], 1), x_T=torch.zeros(1, 3, H, W), noises=torch.zeros(4, 1, 3, H, W),
                     overlap=4, tile_batch=plan.n_tiles, progress=False)
    assert m.model.last_x.shape == (plan.n_tiles, 3, s, s) and bool((m.model.last_t == 0).all())
    kept = cut(mask.expand_as(gt0).contiguous(), plan) > 0
    expect = cut(m.sqrt_alphas_cumprod[0] * gt0, plan)
    assert torch.allclose(m.model.last_x[kept], expect[kept], rtol=0, atol=1e-6)


def test_label_and_concat_cond_reach_every_tile():
    """class-conditional UNet with a channel-concatenated cond: a scene of identical tiles (overlap 0, identical noise per tile)
    comes out as identical tiles, each equal to sampling(1) with that label and that cond; another label gives another scene"""
    s, T = 16, 6
    m = _diffusion("fp32x3", True, T, None, s=s, in_ch=7, num_classes=5)
    plan = TilePlan(2 * s, 3 * s, s, 0)
    rep = lambda t: t.repeat(*([1] * (t.dim() - 2)), 2, 3)
    x1, n1, c1 = synth_input("lx", (1, 3, s, s), 31), synth_input("ln", (T, 1, 3, s, s), 31), synth_input("lc", (1, 4, s, s), 31, uniform=True)
    y = torch.tensor([3])
    scene = m.sampling_scene((plan.H, plan.W), True, DEV, cond=rep(c1), y=y, x_T=rep(x1), noises=rep(n1), tile_batch=4, progress=False)
    one = m.sampling(1, True, DEV, cond=c1.to(DEV), y=y.to(DEV), x_T=x1, noises=n1, progress=False)
    assert torch.equal(scene, rep(one))
    other = m.sampling_scene((plan.H, plan.W), True, DEV, cond=rep(c1), y=torch.tensor([1]), x_T=rep(x1), noises=rep(n1), progress=False)
    assert not torch.equal(other, scene)
    with pytest.raises(EodError):
        m.sampling_scene((plan.H, plan.W), True, DEV, cond=rep(c1), y=torch.tensor([1, 2]), x_T=rep(x1), noises=rep(n1), progress=False)


@pytest.mark.parametrize("scale", [1.0, 2.5])
def test_guidance_reaches_every_tile(scale):
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    s, S = 16, 4
    m = _diffusion("fp32x3", True, 20, None, s=s, in_ch=7)
    plan = TilePlan(2 * s, 3 * s, s, 0)
    rep = lambda t: t.repeat(*([1] * (t.dim() - 2)), 2, 3)
    x1, n1, c1 = synth_input("gx", (1, 3, s, s), 32), synth_input("gn", (S, 1, 3, s, s), 32), synth_input("gc", (1, 4, s, s), 32, uniform=True)
    uc1 = torch.zeros_like(c1)
    smp = DDIMSampler(m)
    scene, _ = smp.sample_scene(S, (plan.H, plan.W), tile_batch=4, conditioning=rep(c1), eta=0.5, x_T=rep(x1), step_noises=rep(n1),
                                unconditional_guidance_scale=scale, unconditional_conditioning=rep(uc1), progress=False)
    one, _ = smp.sample(S, 1, (3, s, s), conditioning=c1.to(DEV), eta=0.5, x_T=x1, step_noises=n1, verbose=False, progress=False,
                        unconditional_guidance_scale=scale, unconditional_conditioning=uc1.to(DEV))
    assert torch.equal(scene, rep(one))
    if scale != 1.0:
        plain, _ = smp.sample_scene(S, (plan.H, plan.W), conditioning=rep(c1), eta=0.5, x_T=rep(x1), step_noises=rep(n1), progress=False)
        assert not torch.equal(plain, scene)


# ------------------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals_come_before_any_launch():
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    from eo_diffusion_amd.diffusion.model import EODiffusion

    class Never(torch.nn.Module):
        def forward(self, x, t, cond=None, y=None):
            raise AssertionError("the network was reached")

    s = 16
    m = EODiffusion(Never(), timesteps=4, image_size=s, in_channels=3, cond_type="sum", device=DEV).to(DEV)
    smp = DDIMSampler(m)
    ok = torch.zeros(1, 4, 32, 48)
    for kw in (dict(scene_size=(15, 48)), dict(scene_size=(32, 8)), dict(scene_size=(32, 48), overlap=9),
               dict(scene_size=(32, 48), overlap=-1), dict(scene_size=(32, 48), cond=torch.zeros(1, 4, 32, 47)),
               dict(scene_size=(32, 48), cond=torch.zeros(2, 4, 32, 48)), dict(scene_size=(32, 48), cond=ok, tile_batch=0),
               dict(scene_size=(32, 48), x_T=torch.zeros(1, 3, 16, 16)), dict(scene_size=(32, 48), rng="numpy"),
               dict(scene_size=(32, 48), device="cpu"), dict(scene_size=32)):
        kw.setdefault("device", DEV)
        with pytest.raises(EodError):
            m.sampling_scene(progress=False, **kw)
    z = torch.zeros(1, 3, 32, 48)
    for kw in (dict(scene_size=(15, 48)), dict(scene_size=(32, 48), overlap=9), dict(scene_size=(32, 48), mask=torch.ones(1, 1, 32, 47), x0=z),
               dict(scene_size=(32, 48), mask=torch.ones(1, 1, 32, 48), x0=torch.zeros(1, 3, 16, 16)),
               dict(scene_size=(32, 48), mask=torch.ones(1, 1, 32, 48)), dict(scene_size=(32, 48), x_T=torch.zeros(1, 3, 32, 32)),
               dict(scene_size=(32, 48), unconditional_conditioning=torch.zeros(1, 4, 32, 48), unconditional_guidance_scale=2.0)):
        with pytest.raises(EodError):
            smp.sample_scene(2, progress=False, **kw)
    plan = TilePlan(32, 48, s, 4)
    with pytest.raises(EodError):
        gather_tiles(torch.zeros(1, 3, 32, 32, device=DEV), plan)
    with pytest.raises(EodError):
        blend_tiles(torch.zeros(plan.n_tiles - 1, 3, s, s, device=DEV), plan)
    with pytest.raises(EodError):
        blend_tiles(torch.zeros(plan.n_tiles, 3, s, 8, device=DEV), plan)
    L = _lib.lib()
    oy, ox, wy, wx = plan.device_tables(DEV)
    t = torch.zeros(plan.n_tiles, 3, s, s, device=DEV)
    sc = torch.zeros(1, 3, 32, 48, device=DEV)
    assert L.eod_scene_gather(sc.data_ptr(), t.data_ptr(), 3, 8, 48, s, oy.data_ptr(), ox.data_ptr(), plan.nty, plan.ntx, 0) == -1
    assert L.eod_scene_blend(t.data_ptr(), 0, wy.data_ptr(), wx.data_ptr(), oy.data_ptr(), ox.data_ptr(), 3, 32, 48, s, plan.nty,
                             plan.ntx, 0) == -1
