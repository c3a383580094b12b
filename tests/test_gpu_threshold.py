"""Dynamic thresholding on the GPU: eod_dyn_threshold against the host emulation tests/threshold_ref.py, bit for
bit in `out` and `s_out` (sizes, alignments, ties and narrow distributions, ranks that part at every bit field of the radix passes,
non-finite values, independence of the batch and of the workspace's contents, refusals), and `threshold=` on the samplers: the wiring
against a loop written here, the tie to the clipped fused kernels, the CPU oracle, range, observations, batches, stacks and scenes."""
import functools
import math

import numpy as np
import pytest
import torch

from eo_diffusion_amd import _lib
from eo_diffusion_amd._lib import EodError
from eo_diffusion_amd.diffusion import consistency as CO
from eo_diffusion_amd.diffusion.threshold import DynamicThreshold, dynamic_threshold
from tests import threshold_ref as TR
from tests.gpu_util import DEV
from tests.helpers import bits_equal, rel_l2
from tests.synth import synth_input

pytestmark = pytest.mark.gpu
INF = math.inf
NS = (1, 2, 77, 768, 4099, 12288, 196608)   # a sample has (n + 3) / 4 quads and a workgroup takes 256 of them at a time: from n = 4099 on
                                            # several workgroups share one sample (5 at 4099 with B = 1, 192 at 196608)


def _stream():
    from eo_diffusion_amd.engine import current_stream_ptr
    return current_stream_ptr(torch.device(DEV))


def _dev(t, off):
    """t on the device, 16-byte aligned or (off) 4 bytes behind a 16-byte boundary"""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=DEV)
    v = buf[1:1 + t.numel()] if off else buf[:t.numel()]
    assert v.data_ptr() % 16 == (4 if off else 0)
    v.copy_(t.reshape(-1))
    return v.view(t.shape)


def _ws(B, n, fill=None, off=False):
    size = int(_lib.lib().eod_dyn_threshold_workspace_size(B, n))
    assert size > 0
    buf = torch.empty(size + 16, dtype=torch.uint8, device=DEV) if fill is None else torch.full((size + 16,), fill, dtype=torch.uint8, device=DEV)
    return buf[4:4 + size] if off else buf[:size]


def call(p, k, frac, cap=INF, *, off=False, ws=None, out=None, s=None, B=None, n=None, ws_bytes=None, p_ptr=None, out_ptr=None, s_ptr=None,
         ws_ptr=None):
    """eod_dyn_threshold itself on p [B, n] (a device tensor); returns (rc, out, s)"""
    Bn, nn = p.shape
    out = _dev(torch.full((Bn, nn), float("nan")), off) if out is None else out
    s = torch.full((Bn,), float("nan"), device=DEV) if s is None else s
    ws = _ws(Bn, nn) if ws is None else ws
    rc = _lib.lib().eod_dyn_threshold(p.data_ptr() if p_ptr is None else p_ptr, k, frac, cap, out.data_ptr() if out_ptr is None else out_ptr,
                                      s.data_ptr() if s_ptr is None else s_ptr, Bn if B is None else B, nn if n is None else n,
                                      ws.data_ptr() if ws_ptr is None else ws_ptr, ws.numel() if ws_bytes is None else ws_bytes, _stream())
    return rc, out, s


def check(p_cpu, k, frac, cap=INF, off=False, **kw):
    """the kernel on p_cpu [B, n] against the emulation, out and s bit for bit; returns (out, s) of the emulation"""
    want_out, want_s, _ = TR.threshold_kf(p_cpu, k, frac, cap)
    rc, out, s = call(_dev(p_cpu, off), k, frac, cap, off=off, **kw)
    assert rc == 0, _lib.lib().eod_last_error()
    assert bits_equal(s.cpu(), want_s), (s.cpu(), want_s, k, frac, cap)
    got = out.cpu()
    if not bits_equal(got, want_out):
        bad = (got.view(torch.int32) != want_out.view(torch.int32)).nonzero()
        raise AssertionError(f"{len(bad)} elements differ, first {bad[0].tolist()}: {got[tuple(bad[0])]} vs {want_out[tuple(bad[0])]}")
    return want_out, want_s


# ------------------------------------------------------------------------------------------------------------ 1. the kernel, bit for bit
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", NS)
def test_kernel_against_the_emulation(n, B):
    """q in {0, 0.5, 0.995, 1} x scales {1e-30, 0.3, 2.5, 1e30}; the alignment (both pointers aligned / both 4 bytes off) and the cap
    (inf / 3.0) alternate over the 16 combinations so that each meets every q and every scale's neighbour"""
    g = torch.Generator().manual_seed(1000 * B + n)
    i = 0
    for q in (0.0, 0.5, 0.995, 1.0):
        k, frac = TR.rank(q, n)
        for scale in (1e-30, 0.3, 2.5, 1e30):
            p = torch.randn(B, n, generator=g) * scale
            check(p, k, frac, cap=(INF, 3.0)[(i // 2) % 2], off=bool(i % 2))
            i += 1


def _from_sorted(n, k, a_k, a_k1, seed, B=2):
    """[B, n] whose k-th and (k + 1)-th smallest |.| are a_k and a_k1 (bit patterns): smaller keys below, larger above, random signs,
    shuffled"""
    g = torch.Generator().manual_seed(seed)
    rows = []
    for b in range(B):
        below = torch.randint(0, a_k + 1, (k,), generator=g, dtype=torch.int64)
        above = torch.randint(a_k1, 0x7F800000, (n - k - 2,), generator=g, dtype=torch.int64)
        keys = torch.cat([below, torch.tensor([a_k, a_k1]), above])
        keys = keys | (torch.randint(0, 2, (n,), generator=g, dtype=torch.int64) << 31)
        keys = keys[torch.randperm(n, generator=g)]
        rows.append((keys - ((keys >> 31) << 32)).to(torch.int32).view(torch.float32))     # (bit 31 set: the negative int32)
    return torch.stack(rows)


# the passes read the key bits 30..23, 22..15, 14..7 and 6..0: pairs (a_(k), a_(k+1)) that part in each field, at its boundary
PAIRS = {"all_fields: 1 - 2^-24 | 1": (0x3F7FFFFF, 0x3F800000),
         "top_exponent_bit: 2 - 2^-23 | 2": (0x3FFFFFFF, 0x40000000),
         "field_1": (0x3F80FFFF, 0x3F810000),
         "field_2": (0x3F80007F, 0x3F800080),
         "lowest_bit": (0x3F800000, 0x3F800001),
         "lowest_bit_above_1": (0x402AAAAA, 0x402AAAAB),
         "equal": (0x3FC00000, 0x3FC00000)}


@pytest.mark.parametrize("name", list(PAIRS))
def test_ranks_that_part_at_every_bit_field(name):
    a_k, a_k1 = PAIRS[name]
    for n, k in ((4099, 2048), (777, 775), (2, 0)):
        p = _from_sorted(n, k, a_k, a_k1, seed=n)
        srt = TR.keys(p).sort(dim=1).values
        assert srt[:, k].tolist() == [a_k] * 2 and srt[:, k + 1].tolist() == [a_k1] * 2          # (the construction)
        for frac in (0.0, 0.5, float(np.float32(0.965))):
            check(p, k, frac, off=(n == 777))


def _narrow(name, B, n):
    g = torch.Generator().manual_seed(n)
    if name == "constant":
        return torch.full((B, n), 1.75)
    if name == "constant_small":
        return torch.full((B, n), -0.3)
    if name == "two_values":
        return torch.where(torch.rand(B, n, generator=g) < 0.7, torch.tensor(0.5), torch.tensor(-2.5))
    if name == "clamped":
        return (torch.randn(B, n, generator=g) * 2.5).clamp(-1, 1)
    if name == "zeros":
        return torch.where(torch.rand(B, n, generator=g) < 0.5, torch.tensor(0.0), torch.tensor(-0.0))
    if name == "denormals":
        return (torch.randint(-(2 ** 23) + 1, 2 ** 23, (B, n), generator=g).float() * 2.0 ** -126) * 2.0 ** -23
    raise KeyError(name)


@pytest.mark.parametrize("name", ["constant", "constant_small", "two_values", "clamped", "zeros", "denormals"])
def test_ties_and_narrow_distributions(name):
    for n in (77, 12288):
        p = _narrow(name, 2, n)
        if name == "denormals":
            assert float(p.abs().max()) < 2.0 ** -126 and float(p.abs().max()) > 0
        for q in (0.0, 0.5, 0.7, 0.995, 1.0):
            k, frac = TR.rank(q, n)
            out, s = check(p, k, frac, off=(n == 77))
            if name in ("clamped", "zeros", "denormals", "constant_small"):
                assert torch.equal(s, torch.ones_like(s)) and bits_equal(out, p.clamp(-1, 1))       # (the static clamp)


def test_non_finite_values():
    n = 4099
    g = torch.Generator().manual_seed(5)
    p = torch.randn(2, n, generator=g) * 2.5
    p[0, 7], p[0, 4000], p[1, 1], p[1, 2] = INF, -INF, -INF, INF
    k, frac = TR.rank(0.995, n)
    out, s = check(p, k, frac)                                            # infinities above the rank: v finite, they come out as +-1
    assert bool(torch.isfinite(s).all()) and float(s.min()) > 1 and out[0, 7] == 1 and out[0, 4000] == -1 and out[1, 1] == -1
    p[0, 100] = float("nan")
    p[1, 200] = -float("nan")
    out, s = check(p, k, frac)                                            # a NaN element becomes -1
    assert bool(torch.isfinite(s).all()) and out[0, 100] == -1 and out[1, 200] == -1 and bool(torch.isfinite(out).all())
    out, s = check(p, n - 1, 0.0)                                         # the rank element is the NaN: s = 1
    assert s.tolist() == [1.0, 1.0] and bits_equal(out, TR.fminf(TR.fmaxf(p, torch.tensor(-1.0)), torch.tensor(1.0)))
    out, s = check(p, n - 3, 0.5)                                         # inf - inf in the interpolation: v NaN, s = 1
    assert s.tolist() == [1.0, 1.0]
    out, s = check(p, n - 3, 0.0, cap=1e30)                               # v = inf: capped
    assert s.tolist() == [float(np.float32(1e30))] * 2


def test_a_sample_does_not_depend_on_the_batch_or_the_workspace():
    n = 12288
    g = torch.Generator().manual_seed(6)
    p = torch.randn(3, n, generator=g) * torch.tensor([[0.3], [2.5], [40.0]])
    k, frac = TR.rank(0.995, n)
    want_out, want_s = check(p, k, frac)
    for b in range(3):                                                    # three single-sample calls
        rc, out, s = call(_dev(p[b:b + 1].contiguous(), False), k, frac)
        assert rc == 0 and bits_equal(out.cpu(), want_out[b:b + 1]) and bits_equal(s.cpu(), want_s[b:b + 1])
    ws, pd = _ws(3, n), _dev(p, False)
    for _ in range(2):                                                    # the second call meets the first call's counters
        rc, out, s = call(pd, k, frac, ws=ws)
        assert rc == 0 and bits_equal(out.cpu(), want_out) and bits_equal(s.cpu(), want_s)
    for off in (False, True):                                             # a workspace of 0xFF bytes, at any alignment
        rc, out, s = call(pd, k, frac, ws=_ws(3, n, fill=255, off=off))
        assert rc == 0 and bits_equal(out.cpu(), want_out) and bits_equal(s.cpu(), want_s)


def test_a_scene_of_2_to_the_24_elements():
    """1 x 4 x 2048^2 (torch.quantile refuses it) and per band: every workgroup strides over its sample many times"""
    x = (torch.randn(1, 4, 2048, 2048, generator=torch.Generator().manual_seed(3)) * 2.5).to(DEV)
    for per in ("sample", "channel"):
        out, s = dynamic_threshold(x, 0.995, per=per)
        want_out, want_s = TR.threshold_image(x.cpu(), 0.995, per=per)
        assert bits_equal(s.cpu(), want_s) and bits_equal(out.cpu(), want_out) and float(s.min()) > 1


def test_refusals_launch_nothing_and_leave_the_outputs_alone():
    B, n = 2, 768
    p = _dev(torch.randn(B, n, generator=torch.Generator().manual_seed(7)), False)
    out, s, ws = torch.full((B, n), float("nan"), device=DEV), torch.full((B,), float("nan"), device=DEV), _ws(B, n)
    buf = torch.full((2 * B * n,), float("nan"), device=DEV)
    rcs = []
    run = lambda k=10, frac=0.5, cap=INF, **kw: rcs.append(call(p, k, frac, cap, **{**dict(out=out, s=s, ws=ws), **kw})[0])
    run(p_ptr=0), run(out_ptr=0), run(s_ptr=0), run(ws_ptr=0)                                       # a null pointer
    run(B=0), run(B=-1), run(n=0), run(n=-4), run(n=2 ** 31), run(n=2 ** 40)                        # (the checks come before any use of n)
    run(k=-1), run(k=n), run(k=2 ** 40)
    run(frac=-0.25), run(frac=1.0), run(frac=1.5), run(frac=float("nan")), run(frac=INF)
    run(cap=0.999), run(cap=0.0), run(cap=-INF), run(cap=float("nan"))
    run(ws_bytes=ws.numel() - 1), run(ws_bytes=0), run(ws_bytes=-1)
    run(out=p), run(s_ptr=p.data_ptr() + 64), run(ws_ptr=p.data_ptr()), run(out_ptr=p.data_ptr() + 4 * n)   # an output on top of p
    in_buf = buf[:B * n].view(B, n)
    run(out=in_buf, s_ptr=buf.data_ptr() + 16), run(out=in_buf, ws_ptr=buf.data_ptr() + 4 * (B * n - 1)), run(s_ptr=ws.data_ptr() + 8)
    torch.cuda.synchronize()
    assert rcs and all(rc == -1 for rc in rcs), rcs
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(s).all()) and bool(torch.isnan(buf).all()) and bool(torch.isfinite(p).all())
    assert _lib.lib().eod_dyn_threshold_workspace_size(0, 16) == -1 and _lib.lib().eod_dyn_threshold_workspace_size(1, 0) == -1
    assert _lib.lib().eod_dyn_threshold_workspace_size(1, 2 ** 31) == -1 and _lib.lib().eod_dyn_threshold_workspace_size(1, 2 ** 31 - 1) > 0
    run(k=0, frac=0.0, cap=1.0), run(k=n - 1, frac=float(np.float32(1 - 2.0 ** -24)))              # (the limits themselves are taken)
    assert rcs[-2:] == [0, 0]
    with pytest.raises(EodError, match="frac"):
        _lib.check(call(p, 10, 1.0, out=out, s=s, ws=ws)[0], "eod_dyn_threshold")


def test_per_channel_is_the_emulation_plane_by_plane():
    x = synth_input("thr_pc", (2, 3, 20, 19), 9) * torch.tensor([0.5, 2.0, 6.0]).view(1, 3, 1, 1)
    out, s = dynamic_threshold(x.to(DEV), 0.9, per="channel")
    assert tuple(s.shape) == (2, 3)
    for b in range(2):
        for c in range(3):
            w_out, w_s, _ = TR.threshold(x[b, c].reshape(1, -1).contiguous(), 0.9)
            assert bits_equal(out[b, c].cpu().reshape(1, -1), w_out) and float(s[b, c]) == float(w_s)
    out1, s1 = dynamic_threshold(x.to(DEV), 0.9, max_value=2.5)
    w_out, w_s = TR.threshold_image(x, 0.9, cap=2.5)
    assert tuple(s1.shape) == (2,) and bits_equal(out1.cpu(), w_out) and bits_equal(s1.cpu(), w_s) and float(s.max()) > 2.5
    with pytest.raises(EodError):
        dynamic_threshold(x, 0.9)                                         # (a CPU tensor: there is no CPU path)


# ------------------------------------------------------------------------------------------------------------ 2. the samplers
from tests import ancestral_ref as AR  # noqa: E402
from tests import consistency_ref as CR  # noqa: E402
from tests import dpm_ref as DR  # noqa: E402
from tests.test_gpu_sampling import TRAJ_TOL, _model  # noqa: E402
from tests.test_gpu_scene_skip import Calls  # noqa: E402

T, S, SHAPE = 20, 10, (3, 16, 16)
EPS = 2.0 ** -23


def _draws(name, count, n=2, seed=17, hw=16):
    return synth_input(name, (count, n, 3, hw, hw), seed)


class Hand:
    """the three C entry points of one evaluation, called by hand: every s of the loop is kept"""

    def __init__(self, shape, thr):
        self.S, self.n = thr.samples(shape)
        self.k, self.frac = TR.rank(thr.quantile, self.n)
        self.cap = thr.cap
        self.ws = _ws(self.S, self.n)
        self.scales = []

    def threshold(self, p):
        out, s = torch.empty_like(p), torch.empty(self.S, device=DEV)
        assert _lib.lib().eod_dyn_threshold(p.data_ptr(), self.k, self.frac, self.cap, out.data_ptr(), s.data_ptr(), self.S, self.n,
                                            self.ws.data_ptr(), self.ws.numel(), _stream()) == 0
        self.scales.append(s)
        return out

    def premise(self):
        s = torch.stack(self.scales).cpu()
        assert float(s.max()) > 1.0, "no evaluation thresholds above 1: the test shows nothing"
        return s


def _ddpm_by_hand(m, x, noise_of, thr):
    L, h = _lib.lib(), Hand(tuple(x.shape), thr)
    n, chw = x.shape[0], x[0].numel()
    for i in range(m.timesteps - 1, -1, -1):
        t = torch.full((n,), i, dtype=torch.int64, device=DEV)
        z = noise_of(i)
        e = m.model(x, t).float().contiguous()
        p, out = torch.empty_like(x), torch.empty_like(x)
        assert L.eod_ddpm_pred_x0(x.data_ptr(), e.data_ptr(), t.data_ptr(), m.alphas_cumprod.data_ptr(), p.data_ptr(), n, chw, m.timesteps, 0,
                                  _stream()) == 0
        p = h.threshold(p)
        assert L.eod_ddpm_step_p0(x.data_ptr(), p.data_ptr(), z.data_ptr(), t.data_ptr(), m.betas.data_ptr(), m.alphas.data_ptr(),
                                  m.alphas_cumprod.data_ptr(), out.data_ptr(), n, chw, m.timesteps, _stream()) == 0
        x = out
    return x, h


@pytest.mark.parametrize("prec", ["fp32x3", "fp16"])
def test_wiring_of_sampling_is_prediction_threshold_step(prec):
    """EODiffusion.sampling(rng="philox", threshold=...) equals the loop of the model's own UNet, eod_ddpm_pred_x0 (clip = 0),
    eod_dyn_threshold and eod_ddpm_step_p0, bit for bit; clipped_reverse_diffusion makes no difference; the clamped call differs"""
    from eo_diffusion_amd.diffusion import chain
    m, thr = _model(prec), DynamicThreshold(0.9)
    shape = (2,) + SHAPE
    with torch.no_grad():
        out = m.sampling(2, device=DEV, rng="philox", seed=5, progress=False, threshold=thr)
        x_T = m._philox(shape, torch.device(DEV), 5, 0, T, chain.X_T_STREAM)
        want, h = _ddpm_by_hand(m, x_T, lambda i: m._philox(shape, torch.device(DEV), 5, 0, i, chain.step_stream(0)), thr)
        other = m.sampling(2, False, device=DEV, rng="philox", seed=5, progress=False, threshold=thr)
        clamped = m.sampling(2, device=DEV, rng="philox", seed=5, progress=False)
    h.premise()
    assert bits_equal(out, want) and bits_equal(other, out) and not torch.equal(clamped, out)
    assert bits_equal(thr.last_bound.last_scale, h.scales[-1])
    assert float(out.abs().max()) <= 1.0                                  # (the step at t = 0 returns the thresholded prediction)


@pytest.mark.parametrize("prec", ["fp32x3", "fp16"])
def test_wiring_of_ddim_is_prediction_threshold_step(prec):
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    m, thr = _model(prec), DynamicThreshold(0.9)
    smp, L = DDIMSampler(m), _lib.lib()
    x_T, sn = synth_input("tdx", (2,) + SHAPE, 21), _draws("tds", S)
    out, inter = smp.sample(S, 2, SHAPE, eta=0.5, x_T=x_T, verbose=False, step_noises=sn, progress=False, log_every_t=1, threshold=thr)
    clamp_free, _ = smp.sample(S, 2, SHAPE, eta=0.5, x_T=x_T, verbose=False, step_noises=sn, progress=False)
    steps = smp.ddim_timesteps
    assert len(steps) == S
    x, h = x_T.to(DEV).contiguous(), Hand((2,) + SHAPE, thr)
    with torch.no_grad():
        for i, index in enumerate(range(S - 1, -1, -1)):
            ts = torch.full((2,), int(steps[index]), device=DEV, dtype=torch.long)
            e = m.model(x, ts).float().contiguous()
            z = sn[i].to(DEV).contiguous()
            p, nxt = torch.empty_like(x), torch.empty_like(x)
            assert L.eod_pred_x0(x.data_ptr(), e.data_ptr(), float(smp.ddim_alphas[index]), float(smp.ddim_sqrt_one_minus_alphas[index]), 0,
                                 p.data_ptr(), x.numel(), _stream()) == 0
            p = h.threshold(p)
            assert L.eod_ddim_step_p0(e.data_ptr(), p.data_ptr(), z.data_ptr(), float(smp.ddim_alphas_prev[index]), float(smp.ddim_sigmas[index]),
                                      1.0, nxt.data_ptr(), x.numel(), _stream()) == 0
            x = nxt
    h.premise()
    assert bits_equal(out, x) and bits_equal(inter["pred_x0"][-1], p) and not torch.equal(clamp_free, out)


@pytest.mark.parametrize("prec", ["fp32x3", "fp16"])
def test_wiring_of_dpm_solver_is_prediction_threshold_step(prec):
    from eo_diffusion_amd.diffusion.dpm_solver import DPMSolverSampler
    from tests.synth import rect_mask
    m, thr = _model(prec), DynamicThreshold(0.9)
    smp, L = DPMSolverSampler(m), _lib.lib()
    x_T = synth_input("tpx", (2,) + SHAPE, 22)
    x0, mask = (synth_input("tp0", (2,) + SHAPE, 22, uniform=True) * 2 - 1).to(DEV), rect_mask(2, 16, 16, 22).to(DEV)
    smp.make_dpm_schedule(S)
    n = smp.num_evaluations                                               # (7 at T = 20: duplicate levels of the logsnr grid are removed)
    mix = _draws("tpm", n)
    kw = dict(order=2, mask=mask, x0=x0, x_T=x_T, mix_noises=mix, progress=False, log_every_t=1)
    out, inter = smp.sample(S, 2, SHAPE, threshold=thr, **kw)
    also, _ = smp.sample(S, 2, SHAPE, clip_denoised=True, threshold=thr, **kw)
    clamped, _ = smp.sample(S, 2, SHAPE, clip_denoised=True, **kw)
    assert n == smp.num_evaluations > 2
    x, h, hist = x_T.to(DEV).contiguous(), Hand((2,) + SHAPE, thr), None
    mk = m._broadcast_mask(mask, x)
    with torch.no_grad():
        for i, index in enumerate(range(n - 1, -1, -1)):
            ts = torch.full((2,), int(smp.dpm_timesteps[index]), device=DEV, dtype=torch.long)
            x = m._repaint_mix(x, x0, mk, ts, mix[i].to(DEV))
            e = m.model(x, ts).float().contiguous()
            second = smp.dpm_second[index] if hist is not None and hist[0] == index + 1 else None
            c_x, c_d, w_cur, w_prev = smp.dpm_first[index] if second is None else second
            p, nxt = torch.empty_like(x), torch.empty_like(x)
            assert L.eod_pred_x0(x.data_ptr(), e.data_ptr(), float(smp.ddim_alphas[index]), float(smp.dpm_sqrt_one_minus_alphas[index]), 0,
                                 p.data_ptr(), x.numel(), _stream()) == 0
            p = h.threshold(p)
            assert L.eod_dpmpp_step_p0(x.data_ptr(), p.data_ptr(), 0 if second is None else hist[1].data_ptr(), float(c_x), float(c_d),
                                       float(w_cur), float(w_prev), nxt.data_ptr(), x.numel(), _stream()) == 0
            x, hist = nxt, (index, p)
    h.premise()
    assert bits_equal(out, x) and bits_equal(inter["pred_x0"][-1], p) and bits_equal(also, out) and not torch.equal(clamped, out)


class Scales:
    """forward hook on the UNet: the threshold's scale of the evaluation before each call, and (done()) of the last one"""

    def __init__(self, module, thr):
        self.thr, self.seen = thr, []
        self.handle = module.register_forward_hook(lambda *a: self.seen.append(thr.last_bound.last_scale.clone()))

    def done(self):
        self.handle.remove()
        return torch.stack(self.seen[1:] + [self.thr.last_bound.last_scale]).cpu()       # (the first call sees the unwritten tensor)


def test_quantile_0_is_the_clipped_fused_path_bit_for_bit():
    """DynamicThreshold(0.0): v = min |p0| <= 1 on every evaluation (asserted), so s = 1, the operator is the static clamp, and
    prediction -> threshold -> step_p0 has the bits of the clipped fused kernels"""
    from eo_diffusion_amd.diffusion.dpm_solver import DPMSolverSampler
    m = _model("fp32x3")
    x_T = synth_input("t0x", (2,) + SHAPE, 23)
    smp, thr = DPMSolverSampler(m), DynamicThreshold(0.0)
    sc = Scales(m.model, thr)
    out, inter = smp.sample(S, 2, SHAPE, x_T=x_T, progress=False, log_every_t=1, threshold=thr)
    s = sc.done()
    assert s.shape == (smp.num_evaluations, 2) and bool((s == 1.0).all())
    want, winter = smp.sample(S, 2, SHAPE, x_T=x_T, progress=False, log_every_t=1, clip_denoised=True)
    assert bits_equal(out, want) and all(bits_equal(a, b) for a, b in zip(inter["pred_x0"], winter["pred_x0"]))
    nz = _draws("t0n", T)
    thr = DynamicThreshold(quantile=0.0)
    sc = Scales(m.model, thr)
    out = m.sampling(2, device=DEV, x_T=x_T, noises=nz, progress=False, threshold=thr)
    s = sc.done()
    assert s.shape == (T, 2) and bool((s == 1.0).all())
    assert bits_equal(out, m.sampling(2, device=DEV, x_T=x_T, noises=nz, progress=False))


def _cpu_eps():
    from tests.test_gpu_repaint_resample import _tiny
    return _tiny()


def test_dpm_solver_call_against_the_oracle_loop():
    """10 evaluations of T = 1000 (test_gpu_dpm_solver.test_call_vs_cpu_loop's chain) with DynamicThreshold(0.9): the CPU loop is the oracle
    UNet, tests/dpm_ref.py's arithmetic and the emulation.  The quantile is 1-Lipschitz in the maximum norm and the division is by
    s >= 1, so the walk is no less stable than the clamped one TRAJ_TOL was set for."""
    from eo_diffusion_amd.diffusion.dpm_solver import DPMSolverSampler
    from eo_diffusion_amd.diffusion.util import make_dpm_timesteps
    from oracle import schedule as SCH
    prec, Tl = "fp32x3", 1000
    tb = SCH.eo_cosine_tables(Tl)
    levels = make_dpm_timesteps("logsnr", S, tb["alphas_cumprod"])
    a, s1m, first, second = DR.tables(tb["alphas_cumprod"].numpy(), levels)
    eps, x_T = _cpu_eps(), synth_input("tox", (2,) + SHAPE, 24)
    f = lambda v: float(np.float32(v))
    x, hist, scales = x_T, None, []
    for index in range(len(levels) - 1, -1, -1):
        ts = torch.full((2,), int(levels[index]), dtype=torch.long)
        e = eps(x, ts)
        p0 = (x - e * f(s1m[index])) / float(np.sqrt(np.float32(a[index])))
        p0, s = TR.threshold_image(p0, 0.9)
        scales.append(s)
        use = hist is not None and index > 0
        c_x, c_d, w_cur, w_prev = second[index] if use else first[index]
        D = p0 * f(w_cur) + hist * f(w_prev) if use else p0
        x, hist = x * f(c_x) + D * f(c_d), p0
    assert float(torch.stack(scales).max()) > 1.0
    smp = DPMSolverSampler(_model(prec, T=Tl))
    out, inter = smp.sample(S, 2, SHAPE, x_T=x_T, progress=False, log_every_t=1, threshold=DynamicThreshold(0.9))
    assert np.array_equal(smp.dpm_timesteps, levels)
    e_out, e_p0 = rel_l2(out.cpu(), x), rel_l2(inter["pred_x0"][-1].cpu(), hist)
    print(f"DPM-Solver++ with DynamicThreshold(0.9) [{prec}]: rel-L2 vs the CPU loop: out {e_out:.3e}, last pred_x0 {e_p0:.3e} (gate {TRAJ_TOL[prec]:g})")
    assert e_out < TRAJ_TOL[prec] and e_p0 < TRAJ_TOL[prec]


def test_ancestral_call_against_the_oracle_loop():
    """20 steps of T = 20 with DynamicThreshold(0.9) against tests/ancestral_ref.py's loop with the emulation as its one link"""
    from oracle import schedule as SCH
    prec = "fp32x3"
    tb = SCH.eo_cosine_tables(T)
    x_T, nz = synth_input("tax", (2,) + SHAPE, 25), _draws("tan", T, seed=25)
    scales = []

    def link(p):
        out, s = TR.threshold_image(p, 0.9)
        scales.append(s)
        return out
    ref = AR.ddpm_sampled(tb, _cpu_eps(), x_T, nz, lambda k: [link], clip=False)
    assert float(torch.stack(scales).max()) > 1.0
    out = _model(prec).sampling(2, device=DEV, x_T=x_T, noises=nz, progress=False, threshold=DynamicThreshold(0.9)).cpu()
    err = rel_l2(out, ref)
    print(f"ancestral sampling with DynamicThreshold(0.9) [{prec}]: rel-L2 vs the CPU loop = {err:.3e} (gate {TRAJ_TOL[prec]:g})")
    assert err < TRAJ_TOL[prec] and float(out.abs().max()) <= 1.0 and float(ref.abs().max()) <= 1.0


def test_an_ancestral_call_without_an_observation_returns_values_in_the_unit_range():
    m = _model("fp16")
    for thr in (DynamicThreshold(), DynamicThreshold(0.5, max_value=2.0), DynamicThreshold(0.9, per="channel")):
        out = m.sampling(3, device=DEV, rng="philox", seed=9, progress=False, threshold=thr)
        assert bool(torch.isfinite(out).all()) and float(out.abs().max()) <= 1.0
        assert tuple(thr.last_bound.last_scale.shape) == ((3, 3) if thr.per == "channel" else (3,))


def test_threshold_first_then_the_observation():
    """the returned sample has the observation's block means, under test_gpu_ancestral_obs's bound for the same statement without a
    threshold: 4 eps * max(1, |x|max) -- the threshold comes first, the projection last"""
    from eo_diffusion_amd.diffusion.consistency import Observation
    factors = (1, 2, 4)
    truth = (synth_input("tbt", (2,) + SHAPE, 26, uniform=True) * 2 - 1).to(DEV)
    values = CO.block_mean(truth, factors)
    m = _model("fp32x3")
    x_T, nz = synth_input("tbx", (2,) + SHAPE, 26), _draws("tbn", T, seed=26)
    out = m.sampling(2, device=DEV, x_T=x_T, noises=nz, progress=False, observation=Observation(values, factors), threshold=DynamicThreshold(0.9))
    free = m.sampling(2, device=DEV, x_T=x_T, noises=nz, progress=False, threshold=DynamicThreshold(0.9))
    miss = float((CO.block_mean(out, factors) - values).abs().max())
    bound = 4 * EPS * max(1.0, float(out.abs().max()))
    print(f"threshold + observation: max |block mean of the returned sample - values| = {miss:.3e} (bound {bound:.3e})")
    assert miss <= bound and float((CO.block_mean(free, factors) - values).abs().max()) > 1e-2


def test_a_member_does_not_depend_on_the_batch():
    m, thr = _model("fp32x3"), DynamicThreshold(0.9)
    x_T = synth_input("tmx", (3,) + SHAPE, 27) * torch.tensor([1.0, 0.5, 2.0]).view(3, 1, 1, 1)
    nz = _draws("tmn", T, n=3, seed=27)
    out = m.sampling(3, device=DEV, x_T=x_T, noises=nz, progress=False, threshold=thr)
    s3 = thr.last_bound.last_scale.clone()
    one = m.sampling(1, device=DEV, x_T=x_T[1:2], noises=nz[:, 1:2], progress=False, threshold=thr)
    assert bits_equal(out[1:2], one) and bits_equal(s3[1:2], thr.last_bound.last_scale)


def test_scenes_and_stacks():
    m = _model("fp32x3", T=8)
    thr = DynamicThreshold(0.9)
    kw = dict(device=DEV, overlap=8, progress=False, rng="philox", seed=3, threshold=thr)
    stack = m.sampling_scene((24, 24), n_scenes=2, **kw)                  # member b is the single-scene call with sample_offset = b
    for b in range(2):
        assert bits_equal(stack[b:b + 1], m.sampling_scene((24, 24), sample_offset=b, **kw))
    assert bits_equal(m.sampling_scene((24, 24), tile_batch=1, **kw), stack[0:1])              # (not on tile_batch)
    assert bits_equal(m.sampling_scene((24, 24), tile_batch=3, **kw), stack[0:1])
    assert float(stack.abs().max()) <= 1.0
    x_T, nz = synth_input("tsx", (1,) + SHAPE, 28), _draws("tsn", 8, n=1, seed=28)
    scene = m.sampling_scene((16, 16), device=DEV, overlap=0, x_T=x_T, noises=nz, progress=False, threshold=thr)   # one tile: the batch form
    assert bits_equal(scene, m.sampling(1, device=DEV, x_T=x_T, noises=nz, progress=False, threshold=thr))
    per_band = m.sampling_scene((24, 24), **{**kw, "threshold": DynamicThreshold(0.9, per="channel")})
    assert not torch.equal(per_band, stack[0:1]) and float(per_band.abs().max()) <= 1.0


def test_refusals_come_before_the_first_unet_call():
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    from eo_diffusion_amd.diffusion.dpm_solver import DPMSolverSampler
    from tests.synth import rect_mask
    m = _model("fp32x3", T=8, cond_type="sum")
    gt, mask = synth_input("trg", (1, 3, 24, 24), 29, uniform=True) * 2 - 1, rect_mask(1, 24, 24, 29)
    cond = torch.cat([gt, mask], 1)
    thr = DynamicThreshold(0.9)
    with Calls(m.model) as calls:
        for bad in (dict(skip_known=True, threshold=thr), dict(threshold=0.995), dict(threshold="dynamic"), dict(threshold=CO)):
            with pytest.raises(EodError, match="threshold"):
                m.sampling_scene((24, 24), device=DEV, cond=cond, overlap=8, progress=False, **bad)
            for smp in (DDIMSampler(m), DPMSolverSampler(m)):
                with pytest.raises(EodError, match="threshold"):
                    smp.sample_scene(4, (24, 24), overlap=8, mask=mask, x0=gt, progress=False, **bad)
        for bad in (0.995, "dynamic"):
            with pytest.raises(EodError, match="threshold"):
                m.sampling(1, device=DEV, progress=False, threshold=bad)
            with pytest.raises(EodError, match="threshold"):
                DDIMSampler(m).sample(4, 1, SHAPE, verbose=False, progress=False, threshold=bad)
            with pytest.raises(EodError, match="threshold"):
                DPMSolverSampler(m).sample(4, 1, SHAPE, progress=False, threshold=bad)
        assert calls.batches == []
