"""GPU: the exact PSF data consistency -- eod_psf_gram, eod_psf_cg (csrc/psf_cg.hip) and PsfObservation(solver="cg") on `observation=`
(diffusion/consistency.py).  DESIGN.md section 9.9.

The stencil is held bit for bit (torch.equal) to the torch fp32 emulation of tests/psf_cg_ref.py; the reduction to a float64 dot of the same
fp32 tensors; a plane's result to the same plane in any other launch, bit for bit; the whole solve to the emulation within the emulation's own
distance from float64; its fixed point to a dense float64 solve; the product's residual to Landweber's; identity taps to eod_obs_project;
nothing observed to the input; bad arguments to -1 with the outputs untouched; the default solver to the launches it took before; whole calls
to CPU loops of the oracle UNet with the emulation as the link, under the gates of tests/test_gpu_psf.py."""
import functools
import os
import re
import types

import numpy as np
import pytest
import torch

from eo_diffusion_amd import _lib
from eo_diffusion_amd._lib import EodError
from eo_diffusion_amd.diffusion import consistency as CO
from eo_diffusion_amd.diffusion.consistency import Observation, PsfObservation, bind, gaussian_psf, psf_gram, psf_observe
from eo_diffusion_amd.tiling import TilePlan
from tests import psf_cg_ref as GR
from tests import psf_ref as PR
from tests import spectral_ref as XR
from tests import test_gpu_consistency as TC
from tests import test_gpu_psf as TP
from tests import test_gpu_spectral as TS
from tests.gpu_util import DEV
from tests.helpers import rel_l2
from tests.synth import synth_input
from tests.test_gpu_dpm_solver import _eps_tiny, _nan, _offset_by_4_bytes
from tests.test_gpu_sampling import TRAJ_TOL, _model
from tests.test_gpu_scene import _diffusion
from tests.test_gpu_scene_skip import Calls

pytestmark = pytest.mark.gpu

EPS = XR.EPS
# (f, r, fine plane): the cases of the issue
CASES = [(6, 9, (6, 6)), (3, 5, (12, 18)), (5, 7, (35, 70)), (8, 12, (24, 168)), (1, 2, (16, 16)), (1, 12, (40, 40)), (2, 3, (140, 148)), (4, 6, (32, 32))]
CHANNELS = [(1, None), (4, None), (4, (1, 3)), (13, None), (13, (0, 4, 5, 12))]          # (C, channels): all / a strict subset
MASKS = {"nomask": None, "full": (True, True), "bcast": (False, False), "k1": (True, False)}   # mask per sample?, per band?


def _stream():
    from eo_diffusion_amd.engine import current_stream_ptr
    return current_stream_ptr(torch.device(DEV))


def _taps(f, r):
    return PR.gaussian(max(f, 2), 0.3, radius=r)


def _binary(name, shape, seed):
    return (synth_input(name, shape, seed, uniform=True) > 0.3).float()


def _workspace(B, K, Hc, Wc, unaligned=False):
    """0xff bytes (NaN as floats and doubles): nothing may depend on what the workspace held"""
    n = int(_lib.lib().eod_psf_cg_workspace_size(B, K, Hc, Wc))
    assert n > 0
    buf = torch.full((n + 16,), 255, dtype=torch.uint8, device=DEV)
    ws = buf[4:4 + n] if unaligned else buf[:n]
    assert ws.data_ptr() % 16 == (4 if unaligned else 0)
    return ws


def _coarse(f, r, plane, B, K, mode, unaligned=False, seed=23):
    """device tensors of a kernel case on the coarse grid: d (the right-hand side: d under the mask), a binary mask, the product's tables"""
    Hc, Wc = plane[0] // f, plane[1] // f
    h = _taps(f, r)
    gy, b = psf_gram(h, f, plane[0])
    gx, _ = psf_gram(h, f, plane[1])
    t = dict(d=synth_input("cd", (B, K, Hc, Wc), seed), gy=torch.from_numpy(gy), gx=torch.from_numpy(gx))
    if MASKS[mode] is not None:
        mb, mk = MASKS[mode]
        t["mask"] = _binary("cm", (B if mb else 1, K if mk else 1, Hc, Wc), seed + 2)
    t = {k: v.to(DEV) for k, v in t.items()}
    t["c"] = t["d"] if "mask" not in t else (t["mask"] * t["d"]).contiguous()
    t["q"] = _nan(B, K, Hc, Wc)
    if unaligned:
        t = {k: _offset_by_4_bytes(v) for k, v in t.items()}
    t["sigma"] = torch.full((B * K,), float("nan"), dtype=torch.float64, device=DEV)       # (double: 8-byte aligned in every case)
    t["ws"] = _workspace(B, K, Hc, Wc, unaligned)
    t["b"] = b
    return t


def gram_(t, mu, d=None, q=None, b=None, sigma=None, ws=None, ws_bytes=None, shape=None, mask="t", gy=None, gx=None):
    d = t["d"] if d is None else d
    q = t["q"] if q is None else q
    m = t.get("mask") if isinstance(mask, str) else mask
    B, K, Hc, Wc = t["d"].shape if shape is None else shape
    ws = t["ws"] if ws is None else ws
    sigma = t["sigma"] if sigma is None else sigma
    rc = _lib.lib().eod_psf_gram(_lib.ptr(d), _lib.ptr(m), float(mu), _lib.ptr(t["gy"] if gy is None else gy), _lib.ptr(t["gx"] if gx is None else gx),
                                 t["b"] if b is None else b, B, K, Hc, Wc, int(m is not None and m.shape[0] != B), int(m is not None and m.shape[1] != K),
                                 _lib.ptr(q), _lib.ptr(sigma), _lib.ptr(ws), ws.numel() if ws_bytes is None else ws_bytes, _stream())
    return rc, q, sigma


def cg_(t, mu, lam, iters, c=None, q=None, b=None, ws=None, ws_bytes=None, shape=None, mask="t", gy=None, gx=None):
    c = t["c"] if c is None else c
    q = t["q"] if q is None else q
    m = t.get("mask") if isinstance(mask, str) else mask
    B, K, Hc, Wc = t["d"].shape if shape is None else shape
    ws = t["ws"] if ws is None else ws
    rc = _lib.lib().eod_psf_cg(_lib.ptr(c), _lib.ptr(m), float(mu), float(lam), _lib.ptr(t["gy"] if gy is None else gy),
                               _lib.ptr(t["gx"] if gx is None else gx), t["b"] if b is None else b, iters, B, K, Hc, Wc,
                               int(m is not None and m.shape[0] != B), int(m is not None and m.shape[1] != K), _lib.ptr(q), _lib.ptr(ws),
                               ws.numel() if ws_bytes is None else ws_bytes, _stream())
    return rc, q


def _cpu(t, *names):
    return [None if t.get(k) is None else t[k].cpu() for k in names]


# ------------------------------------------------------------------------------------------------------------ 1. the stencil and the reduction
@pytest.mark.parametrize("unaligned", [False, True])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("f,r,plane", CASES)
def test_gram_is_bit_exact_and_its_dot_is_float64(f, r, plane, B, unaligned):
    """every (C, channels) x mask form x mu in {0, 0.05}: q torch.equal to the emulation; sigma within 1e-12 of numpy's float64 dot of the same
    fp32 tensors, relative to the sum of the absolute products (the products are exact in float64 and the sum is taken in float64)"""
    for C, channels in CHANNELS:
        K = C if channels is None else len(channels)
        for mode in MASKS:
            t = _coarse(f, r, plane, B, K, mode, unaligned)
            d, mask, gy, gx = _cpu(t, "d", "mask", "gy", "gx")
            for mu in (0.0, 0.05):
                t["q"].fill_(float("nan"))
                rc, q, sigma = gram_(t, mu)
                assert rc == 0, _lib.lib().eod_last_error()
                want = GR.gram32(d, gy, gx, mask, mu)
                assert torch.equal(q.cpu(), want) and bool(torch.isfinite(q).all()), (K, mode, mu)
                prod = d.numpy().astype(np.float64) * want.numpy().astype(np.float64)
                ref, scale = prod.sum(axis=(2, 3)).ravel(), np.abs(prod).sum(axis=(2, 3)).ravel()
                assert np.all(np.abs(sigma.cpu().numpy() - ref) <= 1e-12 * scale), (K, mode, mu)


@pytest.mark.parametrize("one", ["d", "mask", "q", "gy", "gx"])
def test_one_unaligned_pointer_takes_the_scalar_form_with_the_same_bits(one):
    for f, r, plane in ((2, 3, (140, 144)), (1, 2, (16, 16)), (4, 6, (32, 32))):           # (Wc multiples of 4: the aligned launch is the vector form)
        a = _coarse(f, r, plane, 2, 3, "full")
        u = dict(a, q=_nan(*a["q"].shape), sigma=a["sigma"].clone())
        u[one] = _offset_by_4_bytes(u[one])
        (rc0, q0, s0), (rc1, q1, s1) = gram_(a, 0.05), gram_(u, 0.05)
        assert (rc0, rc1) == (0, 0) and torch.equal(q0, q1) and torch.equal(s0, s1)


# ------------------------------------------------------------------------------------------------------------ 2. the solve
def _emulated(t, mu, lam, iters):
    c, mask, gy, gx = _cpu(t, "c", "mask", "gy", "gx")
    emu = GR.cg32(c, gy, gx, mask, mu, lam, iters)
    m64 = 1.0 if mask is None else mask.numpy().astype(np.float64)
    z64 = GR.cg64(c.numpy(), GR.dense_of(gy.numpy()), GR.dense_of(gx.numpy()), None if mask is None else m64, float(np.float32(mu)), iters)
    return emu, float(np.float32(lam)) * (m64 * z64)


@pytest.mark.parametrize("unaligned", [False, True])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("f,r,plane", CASES)
def test_cg_against_the_emulation(f, r, plane, B, unaligned):
    """iters in {1, 3, 8}: the relative L2 of q_out between the GPU and the fp32 emulation must not exceed the emulation's own distance from the
    float64 CG (same tables, same iteration count) plus 1e-7: two fp32 evaluations agree no closer than fp32's own noise on this algorithm.
    Measured on an MI355X: the GPU is bit-equal to the emulation on every case (0 against 1.5e-7 to 3.1e-7)"""
    worst = (0.0, 0.0)
    for (C, channels), mode in zip(CHANNELS, ("nomask", "full", "bcast", "k1", "full")):
        K = C if channels is None else len(channels)
        t = _coarse(f, r, plane, B, K, mode, unaligned)
        for iters, mu, lam in ((1, 0.0, 1.0), (3, 0.05, 0.75), (8, 0.0, 0.625)):
            t["q"].fill_(float("nan"))
            rc, q = cg_(t, mu, lam, iters)
            assert rc == 0, _lib.lib().eod_last_error()
            emu, f64 = _emulated(t, mu, lam, iters)
            scale = float(np.linalg.norm(f64))
            d_gpu = float(np.linalg.norm(q.cpu().numpy().astype(np.float64) - emu.numpy())) / scale
            d_emu = float(np.linalg.norm(emu.numpy().astype(np.float64) - f64)) / scale
            worst = max(worst, (d_gpu, d_emu))
            assert bool(torch.isfinite(q).all()) and d_gpu <= d_emu + 1e-7, (K, mode, iters, d_gpu, d_emu)
    print(f"f={f} r={r} {plane} B={B}: worst GPU vs emulation {worst[0]:.3e} (the emulation vs float64 there: {worst[1]:.3e})")


def _link(t_fine, h, f, lam, iters, mu, solver="cg"):
    """the product's BoundPsf on fine tensors dict(p, values, mask, cs)"""
    B, C, H, W = t_fine["p"].shape
    values, mask = _cpu(t_fine, "values", "mask")
    kw = dict(solver="cg", damping=mu) if solver == "cg" else {}
    link = bind([PsfObservation(values, h, f, t_fine["cs"], mask, lam, iters, **kw)], "test", (B, C, H, W), 1, torch.device(DEV)).links[0]
    assert isinstance(link, CO.BoundPsf)
    return link


def _fine(f, r, plane, B, C, channels, mode, seed=31):
    cs = tuple(range(C)) if channels is None else channels
    K, Hc, Wc = len(cs), plane[0] // f, plane[1] // f
    t = dict(p=synth_input("fp", (B, C, *plane), seed), values=synth_input("fv", (B, K, Hc, Wc), seed + 1, uniform=True) * 2 - 1)
    if MASKS[mode] is not None:
        mb, mk = MASKS[mode]
        t["mask"] = _binary("fm", (B if mb else 1, K if mk else 1, Hc, Wc), seed + 2)
    t = {k: v.to(DEV) for k, v in t.items()}
    t["cs"] = cs
    return t


def _project(t, h, f, lam=0.75, iters=5, mu=0.05):
    link = _link(t, h, f, lam, iters, mu)
    out = link.project(0, t["p"])
    return out, link._coarse[1].clone()


@pytest.mark.parametrize("f,r,plane", CASES)
def test_a_plane_does_not_depend_on_its_launch(f, r, plane):
    """a second run; member b of B = 3 against the launch on its slice; a listed channel against the launch that lists it alone: torch.equal on
    q_out and on BoundPsf.project's output"""
    h = _taps(f, r)
    for mode in ("full", "bcast", "nomask"):
        t = _fine(f, r, plane, 3, 4, (1, 3), mode)
        out, q = _project(t, h, f)
        out2, q2 = _project(t, h, f)
        assert torch.equal(out, out2) and torch.equal(q, q2) and bool(torch.isfinite(out).all()) and not torch.equal(out, t["p"])
        for b in range(3):
            one = {k: (v[b:b + 1].contiguous() if torch.is_tensor(v) and v.shape[0] == 3 else v) for k, v in t.items()}
            o1, q1 = _project(one, h, f)
            assert torch.equal(o1, out[b:b + 1]) and torch.equal(q1, q[b:b + 1]), (mode, b)
        alone = dict(t, cs=(3,), values=t["values"][:, 1:2].contiguous())
        if "mask" in t and t["mask"].shape[1] != 1:
            alone["mask"] = t["mask"][:, 1:2].contiguous()
        o1, q1 = _project(alone, h, f)
        assert torch.equal(o1[:, 3], out[:, 3]) and torch.equal(q1[:, 0], q[:, 1]) and torch.equal(o1[:, 1], t["p"][:, 1]), mode


def test_a_launch_beyond_the_grid_cap_is_walked_by_the_stride_loop():
    """B = 3, K = 13, coarse 330 x 330 (11 x 11 tiles a plane), iters = 2: more (plane, tile) pairs than EOD_PSF_GRID_BLOCKS, so the first
    workgroups take a second one; one of its planes alone gives the same bits"""
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "eodiff.h")).read()
    cap = int(re.search(r"#define EOD_PSF_GRID_BLOCKS (\d+)", hdr).group(1))
    assert 3 * 13 * 11 * 11 > cap
    h = _taps(1, 2)
    t = _fine(1, 2, (330, 330), 3, 13, None, "k1")
    out, q = _project(t, h, 1, iters=2)
    b, k = 2, 11
    one = dict(p=t["p"][b:b + 1, k:k + 1].contiguous(), values=t["values"][b:b + 1, k:k + 1].contiguous(), mask=t["mask"][b:b + 1].contiguous(), cs=(0,))
    o1, q1 = _project(one, h, 1, iters=2)
    assert torch.equal(o1[0, 0], out[b, k]) and torch.equal(q1[0, 0], q[b, k]) and bool(torch.isfinite(out).all())


# ------------------------------------------------------------------------------------------------------------ 3. where it lands
EXACT = [(4, 0.6, (32, 32), 0.0), (2, 0.3, (24, 28), 0.0), (3, 0.3, (12, 18), 0.0), (4, 0.6, (32, 32), 0.05)]


@pytest.mark.parametrize("f,mtf,plane,mu", EXACT)
def test_48_iterations_land_on_the_dense_float64_solve(f, mtf, plane, mu):
    """consistent observations made with psf_observe, a binary mask, weight 1, 48 iterations: the true relative residual, in float64 from the GPU's
    out (mu > 0: of the damped system, c - S z, from the GPU's q_out), is <= 1e-5, and the correction out - p is within 1e-5 relative L2 of the
    dense float64 solve's.  The CPU emulation measures 8e-8 to 4.4e-7; the cap leaves a factor of 20 for the fp32 fine-grid kernels on either
    side of the solve.  Measured on an MI355X: residuals 1.3e-7 to 3.5e-7, corrections 2.3e-7 to 3.4e-7"""
    h = PR.gaussian(f, mtf)
    H, W = plane
    truth = (synth_input("et", (2, 2, H, W), 41, uniform=True) * 2 - 1).to(DEV)
    t = dict(p=synth_input("ep", (2, 2, H, W), 42).to(DEV), values=psf_observe(truth, h, f), mask=_binary("em", (2, 1, H // f, W // f), 43).to(DEV), cs=(0, 1))
    link = _link(t, h, f, 1.0, 48, mu)
    out = link.project(0, t["p"])
    q = link._coarse[1].cpu().numpy().astype(np.float64)
    p64, y64, m64 = (t[k].cpu().numpy().astype(np.float64) for k in ("p", "values", "mask"))
    Gy, Gx = GR.gram64(h, H, f), GR.gram64(h, W, f)
    c = m64 * (PR.apply64(p64, h, f) - y64)
    z = GR.dense64(c, Gy, Gx, m64, float(np.float32(mu)))
    want = -PR.adjoint64(m64 * z, h, f, H, W)
    got = out.cpu().numpy().astype(np.float64) - p64
    if mu == 0.0:
        res = m64 * (PR.apply64(out.cpu().numpy(), h, f) - y64)
    else:
        res = c - (m64 * np.einsum("yh,bkhw,xw->bkyx", Gy, m64 * q, Gx) + float(np.float32(mu)) * q)
    e_res, e_cor = float(np.linalg.norm(res) / np.linalg.norm(c)), float(np.linalg.norm(got - want) / np.linalg.norm(want))
    print(f"f={f} MTF {mtf} {plane} mu={mu}: true residual / start {e_res:.3e}, correction vs the dense float64 solve {e_cor:.3e}")
    assert e_res <= 1e-5 and e_cor <= 1e-5


def test_cg_16_against_landweber_8():
    """f = 4, MTF 0.6, 32 x 32, white noise p and y, both through the product: the cg residual at 16 iterations is at most 0.01 x the Landweber
    residual at 8 steps (the CPU emulation: 6.9e-6 against 6.3e-2 of the start; measured on an MI355X with this test's inputs: 8.7e-6 against
    9.7e-2)"""
    f, h = 4, PR.gaussian(4, 0.6)
    t = dict(p=synth_input("lp", (1, 2, 32, 32), 51).to(DEV), values=synth_input("lv", (1, 2, 8, 8), 52).to(DEV), cs=(0, 1))
    y64 = t["values"].cpu().numpy().astype(np.float64)
    res = lambda z: float(np.linalg.norm(PR.apply64(z.cpu().numpy(), h, f) - y64))
    start = res(t["p"])
    cg, lw = res(_link(t, h, f, 1.0, 16, 0.0).project(0, t["p"])), res(_link(t, h, f, 1.0, 8, 0.0, "landweber").project(0, t["p"]))
    print(f"residual / start: cg iters=16 {cg / start:.3e}, Landweber iters=8 {lw / start:.3e}")
    assert cg <= 0.01 * lw


@pytest.mark.parametrize("f", [1, 2, 4, 8])
def test_identity_taps_are_obs_project(f):
    """h = [1.0], one iteration: G = I / f^2 is exact for these f and one CG step solves it -- eod_obs_project on the replicated observation
    within 4 eps max(1, |p|max)"""
    for mode, plane in (("full", (2 * f, 3 * f)), ("nomask", (16 * f, 20 * f))):
        t = _fine(f, 0, plane, 2, 3, None, mode)
        rep = lambda z: None if z is None else z.repeat_interleave(f, 2).repeat_interleave(f, 3).contiguous()
        to = dict(x=t["p"], values=rep(t["values"]), mask=rep(t.get("mask")), out=_nan(*t["p"].shape))
        rc, want = TS.obs_project(to, (f,) * 3, 1.0, t["p"], to["out"])
        got = _link(t, [1.0], f, 1.0, 1, 0.0).project(0, t["p"])
        assert rc == 0 and float((got - want).abs().max()) <= 4 * EPS * max(1.0, float(t["p"].abs().max()))


@pytest.mark.parametrize("how", ["weight 0", "mask 0"])
@pytest.mark.parametrize("f,r,plane", [(1, 2, (16, 16)), (3, 5, (12, 18)), (6, 9, (6, 6)), (2, 3, (140, 148))])
def test_nothing_observed_returns_the_input(f, r, plane, how):
    t = _fine(f, r, plane, 2, 4, (1, 3), "full")
    if how == "mask 0":
        t["mask"].zero_()
    got = _link(t, _taps(f, r), f, 0.0 if how == "weight 0" else 1.0, 7, 0.0).project(0, t["p"])
    assert got.data_ptr() != t["p"].data_ptr() and torch.equal(got, t["p"])


def test_bad_arguments_return_the_error_and_leave_the_outputs_alone():
    t = _coarse(2, 3, (24, 32), 2, 3, "full")
    B, K, Hc, Wc = t["d"].shape
    n = t["d"].numel()
    ws0 = t["ws"].clone()
    buf = _nan(2 * n)
    calls = []
    g = lambda **kw: calls.append(gram_(t, **{**dict(mu=0.05), **kw})[0])
    s = lambda **kw: calls.append(cg_(t, **{**dict(mu=0.05, lam=1.0, iters=4), **kw})[0])
    none = types.SimpleNamespace(data_ptr=lambda: 0, shape=t["d"].shape, numel=lambda: t["ws"].numel())
    for run in (g, s):
        run(b=-1), run(b=25), run(mu=-0.01), run(mu=float("nan")), run(mu=float("inf"))
        run(q=none), run(gy=none), run(gx=none), run(ws=none)
        run(shape=(0, K, Hc, Wc)), run(shape=(B, 0, Hc, Wc)), run(shape=(B, K, 0, Wc)), run(shape=(B, K, Hc, -1))
        run(ws_bytes=t["ws"].numel() - 1), run(ws_bytes=0), run(ws_bytes=-5)
        run(q=t["mask"]), run(q=t["gy"].view(-1)[:1]), run(ws=t["mask"].view(-1).view(torch.uint8)[:8], ws_bytes=t["ws"].numel())
    g(d=none), g(sigma=none), g(q=t["d"]), g(d=buf[:n].view(t["d"].shape), q=buf[n - 4:2 * n - 4].view(t["d"].shape))
    s(c=none), s(q=t["c"]), s(c=buf[:n].view(t["d"].shape), q=buf[n - 4:2 * n - 4].view(t["d"].shape))
    s(iters=0), s(iters=65), s(iters=-1)
    for lam in (-0.25, 1.5, float("nan"), float("inf")):
        s(lam=lam)
    torch.cuda.synchronize()
    assert calls and all(rc == -1 for rc in calls), calls
    for z in (t["q"], t["sigma"], buf):
        assert bool(torch.isnan(z).all())
    assert torch.equal(t["ws"], ws0) and bool(torch.isfinite(t["d"]).all()) and bool(torch.isfinite(t["gy"]).all())
    with pytest.raises(EodError):
        _lib.check(cg_(t, 0.0, 1.0, 65)[0], "eod_psf_cg")
    assert _lib.lib().eod_psf_cg_workspace_size(0, 1, 4, 4) == -1
    assert cg_(t, 0.05, 1.0, 64)[0] == 0 and gram_(t, 0.0, b=0, gy=t["gy"], gx=t["gx"])[0] == 0            # (the limits themselves are taken)


def test_the_default_solver_takes_the_launches_it_took_before():
    """solver="landweber" (and no solver at all) against iters x (eod_psf_residual, eod_psf_update) launched directly, as project did before"""
    f, r, plane, lam, iters = 4, 6, (32, 32), 0.625, 3
    h = _taps(f, r)
    t = TP._tensors(f, r, *plane, 2, 4, (1, 3), "full")
    values, mask = _cpu(t, "values", "mask")
    shape = tuple(t["p"].shape)
    p = t["p"]
    bufs = [_nan(*shape), _nan(*shape)]
    step = bind([PsfObservation(values, h, f, t["cs"], mask, lam, iters)], "test", shape, 1, torch.device(DEV)).links[0].step
    for it in range(iters):
        rc1, q = TP.residual_(t, h, f, lam, p=p)
        rc2, p = TP.update_(t, h, f, step, p=p, q=q, out=bufs[it % 2])
        assert (rc1, rc2) == (0, 0)
    for kw in (dict(), dict(solver="landweber"), dict(solver="landweber", damping=0.0)):
        link = bind([PsfObservation(values, h, f, t["cs"], mask, lam, iters, **kw)], "test", shape, 1, torch.device(DEV)).links[0]
        assert torch.equal(link.project(0, t["p"]), p)


# ------------------------------------------------------------------------------------------------------------ 4. whole calls
T_CALL, S_CALL, VARIANTS = TS.T_CALL, TS.S_CALL, TS.VARIANTS
FORMS = ("cg", "chain")
H4 = PR.gaussian(4)                                                                        # f = 4, MTF 0.3: r = 6


def _links(form, shape, n_eval, seed, iters=8):
    """form "cg": one cg link, channels 0 and 2 at f = 4 under a binary coarse mask; "chain": [a pan band at f = 1 (a SpectralObservation), the
    three bands through the PSF at f = 4 with solver="cg"].  One weight and one damping per evaluation and link."""
    B, C, H, W = shape
    truth = synth_input("lt", shape, seed, uniform=True) * 2 - 1
    w_down = [float(np.float32(w)) for w in np.linspace(1.0, 0.5, n_eval)]
    w_up = [float(np.float32(w)) for w in np.linspace(0.25, 1.0, n_eval)]
    damp = [float(np.float32(w)) for w in np.linspace(0.1, 0.0, n_eval)]
    gy, gx = GR.tables(H4, 4, H, W)
    if form == "cg":
        return [dict(kind="cg", values=PR.apply(truth, H4, 4, (0, 2)), h=H4, f=4, channels=(0, 2), iters=iters, gy=gy, gx=gx,
                     mask=_binary("lm", (B, 1, H // 4, W // 4), seed), weights=w_down, dampings=damp)]
    return [dict(kind="spec", values=XR.apply(truth, TS.PAN3, 1), R=TS.PAN3, f=1, mask=None, weights=w_up),
            dict(kind="cg", values=PR.apply(truth, H4, 4), h=H4, f=4, channels=None, iters=iters, gy=gy, gx=gx, mask=None, weights=w_down, dampings=damp)]


def _observation(links, sl=None):
    sl = sl or (lambda z, f: z)
    out = []
    for l in links:
        if l["kind"] == "cg":
            out.append(PsfObservation(sl(l["values"], l["f"]), l["h"], l["f"], l["channels"], None if l["mask"] is None else sl(l["mask"], l["f"]),
                                      l["weights"], l["iters"], "cg", l["dampings"]))
        else:
            out.append(TS._observation([dict(l, values=sl(l["values"], 1))], None, True))
    return out[0] if len(out) == 1 else out


def _cpu_links(links, k):
    return [GR.cg_link(l["values"], l["h"], l["f"], l["gy"], l["gx"], l["channels"], l["mask"], l["weights"][k], l["dampings"][k], l["iters"])
            if l["kind"] == "cg" else TS._cpu_links([l], k)[0] for l in links]


def _call_case(form, n_lv, masked=False, resample=None, seed=97):
    c = TC._call_case(n_lv, masked, resample, seed)
    c["links"] = _links(form, (2, 3, 16, 16), len(c["obs"]["weights"]), seed)
    return c


@functools.lru_cache(maxsize=None)
def _ddim_reference(form, variant):
    from oracle import schedule as SCH
    steps = TC._ddim_steps()
    c = _call_case(form, len(steps), **VARIANTS[variant])
    dd = SCH.ddim_tables(TC._tables()["alphas_cumprod"], steps, 0.5)
    _, _, eps = _eps_tiny()
    return XR.ddim_sampled(TC._tables(), dd, steps, eps, c["x_T"], c["step_noises"], lambda k: _cpu_links(c["links"], k), c.get("x0"), c.get("mask"),
                           c.get("mix_noises"), VARIANTS[variant].get("resample"), c["jump_noises"])


@functools.lru_cache(maxsize=None)
def _dpm_reference(form, variant, clip):
    levels = TC._dpm_levels()
    c = _call_case(form, len(levels), **VARIANTS[variant])
    _, _, eps = _eps_tiny()
    return XR.dpm_sampled(TC._tables(), levels, eps, c["x_T"], lambda k: _cpu_links(c["links"], k), 2, clip, c.get("x0"), c.get("mask"),
                          c.get("mix_noises"), VARIANTS[variant].get("resample"), c["jump_noises"])


@pytest.mark.parametrize("prec", ["fp32", "fp16", "fp32x3"])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("form", FORMS)
def test_ddim_call_vs_cpu_loop(form, variant, prec):
    """the call of tests/test_gpu_psf.py with cg links (8 iterations, one weight and one damping per evaluation): the CPU loop is the oracle
    UNet with the fp32 emulation of the solve as the link.  Gates: TRAJ_TOL"""
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    steps = TC._ddim_steps()
    kw = VARIANTS[variant]
    c = _call_case(form, len(steps), **kw)
    ref, ref_p0 = _ddim_reference(form, variant)
    smp = DDIMSampler(_model(prec, T=T_CALL))
    extra = dict(x0=c["x0"].to(DEV), mask=c["mask"].to(DEV), mix_noises=c["mix_noises"]) if kw.get("masked") else {}
    out, inter = smp.sample(S_CALL, 2, (3, 16, 16), eta=0.5, verbose=False, progress=False, log_every_t=1, x_T=c["x_T"], step_noises=c["step_noises"],
                            resample=kw.get("resample"), jump_noises=c["jump_noises"], observation=_observation(c["links"]), **extra)
    e_out, e_p0 = rel_l2(out.cpu(), ref), rel_l2(inter["pred_x0"][-1].cpu(), ref_p0)
    print(f"DDIM + {form}, {variant} [{prec}]: rel-L2 vs the CPU loop: out {e_out:.3e}, last pred_x0 {e_p0:.3e} (gate {TRAJ_TOL[prec]:g})")
    assert e_out < TRAJ_TOL[prec] and e_p0 < TRAJ_TOL[prec]


@pytest.mark.parametrize("prec", ["fp32", "fp16", "fp32x3"])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("form", FORMS)
def test_dpm_call_vs_cpu_loop(form, variant, clip, prec):
    from eo_diffusion_amd.diffusion.dpm_solver import DPMSolverSampler
    levels = TC._dpm_levels()
    kw = VARIANTS[variant]
    c = _call_case(form, len(levels), **kw)
    ref, ref_p0 = _dpm_reference(form, variant, clip)
    smp = DPMSolverSampler(_model(prec, T=T_CALL))
    extra = dict(x0=c["x0"].to(DEV), mask=c["mask"].to(DEV), mix_noises=c["mix_noises"]) if kw.get("masked") else {}
    out, inter = smp.sample(S_CALL, 2, (3, 16, 16), clip_denoised=clip, x_T=c["x_T"], resample=kw.get("resample"), jump_noises=c["jump_noises"],
                            progress=False, log_every_t=1, observation=_observation(c["links"]), **extra)
    e_out, e_p0 = rel_l2(out.cpu(), ref), rel_l2(inter["pred_x0"][-1].cpu(), ref_p0)
    print(f"DPM-Solver++ + {form}, {variant}, clip {clip} [{prec}]: rel-L2 vs the CPU loop: out {e_out:.3e}, last pred_x0 {e_p0:.3e} "
          f"(gate {TRAJ_TOL[prec]:g})")
    assert e_out < TRAJ_TOL[prec] and e_p0 < TRAJ_TOL[prec]


def test_the_ancestral_sampler_returns_a_sample_that_meets_the_observation():
    """EODiffusion.sampling, weight 1, 32 iterations: the returned sample, seen through psf_observe, meets `values` on the mask to <= 1e-4
    relative -- the promise section 9.8 makes for the other kinds of observation.  Measured on an MI355X: 1.4e-7 (Landweber iters=8: 1.1e-1)"""
    m = _model("fp32x3", T=20)
    truth = (synth_input("at", (2, 3, 16, 16), 61, uniform=True) * 2 - 1).to(DEV)
    values, mask = psf_observe(truth, H4, 4), _binary("am", (2, 1, 4, 4), 62).to(DEV)
    obs = PsfObservation(values.cpu(), H4, 4, None, mask.cpu(), 1.0, 32, "cg")
    out = m.sampling(2, device=DEV, rng="philox", seed=3, progress=False, observation=obs)
    free = m.sampling(2, device=DEV, rng="philox", seed=3, progress=False)
    miss = lambda z: float((mask * (psf_observe(z, H4, 4) - values)).double().norm() / (mask * values).double().norm())
    lw = m.sampling(2, device=DEV, rng="philox", seed=3, progress=False, observation=PsfObservation(values.cpu(), H4, 4, None, mask.cpu(), 1.0, 8))
    print(f"|m (A x - y)| / |m y| of the returned sample: cg iters=32 {miss(out):.3e}, Landweber iters=8 {miss(lw):.3e}, no observation {miss(free):.3e}")
    assert bool(torch.isfinite(out).all()) and miss(out) <= 1e-4


# ------------------------------------------------------------------------------------------------------------ 5. scenes
def _scene_links(H, W, n, seed, B=1, f=4):
    truth = synth_input("st", (B, 3, H, W), seed, uniform=True) * 2 - 1
    h = PR.gaussian(f)
    w = [float(np.float32(v)) for v in np.linspace(1.0, 0.25, n)]
    d = [float(np.float32(v)) for v in np.linspace(0.0, 0.1, n)]
    gy, gx = GR.tables(h, f, H, W)
    return [dict(kind="cg", values=PR.apply(truth, h, f, (0, 2)), h=h, f=f, channels=(0, 2), iters=8, gy=gy, gx=gx,
                 mask=_binary("sm", (B, 1, H // f, W // f), seed), weights=w, dampings=d)]


def _emulate_last(smp, which, seen, links, k):
    if which == "ddim":
        x, e_t, noise, index, temperature, obs = seen[-1]
        return XR.ddim_step(x.cpu(), e_t.cpu(), None if noise is None else noise.cpu(), smp.ddim_alphas[index], smp.ddim_alphas_prev[index],
                            smp.ddim_sigmas[index], smp.ddim_sqrt_one_minus_alphas[index], temperature, _cpu_links(links, k))
    x, e_t, hist, index, clip, obs = seen[-1]
    assert index == 0
    return XR.dpm_step(x.cpu(), e_t.cpu(), None, smp.ddim_alphas[index], smp.dpm_sqrt_one_minus_alphas[index], *smp.dpm_first[index], clip,
                       _cpu_links(links, k))


@pytest.mark.parametrize("which", ["ddim", "dpm"])
def test_a_footprint_across_a_tile_border_follows_the_emulation_on_the_recorded_inputs(which):
    """overlap 8, tile 16, scene 24 x 36, f = 4, r = 6: every coarse pixel's footprint crosses a tile edge and the solve couples the whole coarse
    plane.  The scene-level step is one pass over the scene: its recorded inputs go through the emulation, one step, under the fp32 gate"""
    s, S, H, W = 16, 5, 24, 36
    plan = TilePlan(H, W, s, 8)
    assert len(plan.origins_x) > 2
    smp = TC._samplers(_diffusion("fp32x3", False, 20, s=s))[which]
    n = len(smp.make_dpm_schedule(S)) if which == "dpm" else 5
    links = _scene_links(H, W, n, 86)
    seen = TS._record(smp, which)
    scene, inter = smp.sample_scene(S, (H, W), overlap=8, progress=False, observation=_observation(links), **TC._scene_kw(which, n, H, W, 86))
    assert len(seen) == n and seen[-1][0].shape == (1, 3, H, W) and seen[-1][-1] is not None
    want_x, want = _emulate_last(smp, which, seen, links, n - 1)
    e_x, e_p0 = rel_l2(scene.cpu(), want_x), rel_l2(inter["pred_x0"][-1].cpu(), want)
    print(f"{which} scene: rel-L2 vs the emulation on the recorded inputs: x {e_x:.3e}, pred_x0 {e_p0:.3e}")
    assert e_x < TRAJ_TOL["fp32"] and e_p0 < TRAJ_TOL["fp32"]
    free, _ = smp.sample_scene(S, (H, W), overlap=8, progress=False, **TC._scene_kw(which, n, H, W, 86))
    assert not torch.equal(free, scene)


@pytest.mark.parametrize("which", ["ddim", "dpm"])
def test_member_b_of_a_stack_equals_the_single_scene_call(which):
    s, S, H, W, B = 16, 5, 24, 36, 2
    smp = TC._samplers(_diffusion("fp32x3", False, 20, s=s))[which]
    n = len(smp.make_dpm_schedule(S)) if which == "dpm" else 5
    links = _scene_links(H, W, n, 87, B)
    kw = TC._scene_kw(which, n, H, W, 87, B)
    stack, inter = smp.sample_scene(S, (H, W), overlap=8, progress=False, n_scenes=B, observation=_observation(links), **kw)
    assert stack.shape == (B, 3, H, W) and bool(torch.isfinite(stack).all())
    for b in range(B):
        one_kw = {k: (v[b:b + 1] if k == "x_T" else v[:, b:b + 1] if k == "step_noises" else v) for k, v in kw.items()}
        one, inter1 = smp.sample_scene(S, (H, W), overlap=8, progress=False, observation=_observation(links, lambda z, f: z[b:b + 1]), **one_kw)
        assert torch.equal(stack[b:b + 1], one) and torch.equal(inter["pred_x0"][-1][b:b + 1], inter1["pred_x0"][-1])
    assert not torch.equal(stack[:1], stack[1:])


def test_refusals_come_before_any_launch():
    from eo_diffusion_amd.diffusion.model import EODiffusion

    class Never(torch.nn.Module):
        def forward(self, x, t, cond=None, y=None):
            raise AssertionError("the network was reached")

    s, T, S, H, W = 16, 20, 5, 32, 48
    m = EODiffusion(Never(), timesteps=T, image_size=s, in_channels=3, device=DEV).to(DEV)
    z = torch.zeros
    h = gaussian_psf(4)
    cg = lambda *shape, **kw: PsfObservation(z(*shape), h, 4, solver="cg", **kw)
    ok, ok_obs = cg(1, 3, H // 4, W // 4), Observation(z(1, 3, H, W), (1, 2, 4))
    with Calls(m.model) as calls:
        for kw in (dict(solver="fft"), dict(solver="cg", iters=65), dict(solver="cg", damping=-1.0), dict(damping=0.1),
                   dict(solver="cg", mask=torch.full((1, 1, H // 4, W // 4), 0.5))):
            with pytest.raises(EodError):
                PsfObservation(z(1, 3, H // 4, W // 4), h, 4, **kw)
        for which, smp in TC._samplers(m).items():
            n = len(smp.make_dpm_schedule(S)) if which == "dpm" else 5
            extra = dict(verbose=False) if which == "ddim" else {}
            for kw in (dict(observation=ok, skip_known=True, mask=torch.ones(H, W), x0=z(1, 3, H, W)),       # skip_known + observation stays refused
                       dict(observation=[ok_obs, ok], skip_known=True, mask=torch.ones(H, W), x0=z(1, 3, H, W)),
                       dict(observation=cg(1, 3, H // 4, W // 4, damping=[0.1] * (n + 1))),                  # dampings against the walk
                       dict(observation=[ok_obs, cg(1, 3, H // 4, W // 4, damping=[0.1] * n)], resample=(2, 2)),
                       dict(observation=cg(1, 3, 4, 4))):
                with pytest.raises(EodError):
                    smp.sample_scene(S, (H, W), progress=False, **extra, **kw)
            for kw in (dict(observation=ok), dict(observation=[cg(2, 3, s // 4, s // 4, damping=[0.5] * (n - 1))])):
                with pytest.raises(EodError):
                    smp.sample(S, 2, (3, s, s), progress=False, **extra, **kw)
        for kw in (dict(observation=cg(2, 3, s // 4, s // 4, damping=[0.1] * (T + 1))), dict(observation=[cg(2, 3, s // 4, s // 4, damping=[0.1] * (T - 1))])):
            with pytest.raises(EodError):
                m.sampling(2, device=DEV, progress=False, **kw)
    assert calls.batches == []
