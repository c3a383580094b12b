"""GPU: cross-band PSF observations -- eod_psf_residual_mix, eod_psf_apply_mix, eod_psf_update_mix (csrc/psf.hip) and
PsfObservation(response=...) / psf_observe(response=...) on `observation=` (diffusion/consistency.py).  DESIGN.md section 9.10.

The kernels are held bit for bit (torch.equal) to the torch fp32 emulation of tests/spectral_psf_ref.py in every access form; with one-hot
rows to eod_psf_residual / eod_psf_update; a plane's result to the same plane in any other launch; 48 iterations of the cg link to a dense
float64 solve on kron(R, A_H, A_W); whole calls to CPU loops of the oracle UNet with the emulation as the link, under the gates of
tests/test_gpu_sampling.py; bad arguments to -1 with the outputs untouched; response=None to the launches it took before."""
import ctypes
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
from eo_diffusion_amd.diffusion.consistency import Observation, PsfObservation, bind, gaussian_psf, psf_observe
from eo_diffusion_amd.tiling import TilePlan
from tests import psf_cg_ref as GR
from tests import psf_ref as PR
from tests import spectral_psf_ref as SP
from tests import spectral_ref as XR
from tests import test_gpu_consistency as TC
from tests import test_gpu_psf as TP
from tests import test_gpu_psf_cg as TG
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
# (f, r, C, K, fine plane): the cases of the issue
CASES = [(6, 9, 1, 1, (6, 6)), (1, 12, 4, 1, (40, 40)), (3, 5, 4, 2, (12, 18)), (5, 7, 3, 2, (35, 70)), (2, 3, 13, 2, (140, 148)),
         (4, 6, 4, 3, (32, 32)), (8, 12, 32, 8, (24, 168))]
MODES = {"full": (True, True), "bcast": (False, False), "nomask": (True, None)}          # values per sample?, mask per sample? (None: no mask)

PAN4 = [[0.25, 0.35, 0.25, 0.15]]
R32 = [[0.66, 0.29, 0.05], [0.05, 0.29, 0.66]]
R43 = [[0.4, 0.4, 0.2, 0.0], [0.1, 0.4, 0.4, 0.1], [0.0, 0.2, 0.4, 0.4]]
PAN3 = [[0.3, 0.5, 0.2]]


def _stream():
    from eo_diffusion_amd.engine import current_stream_ptr
    return current_stream_ptr(torch.device(DEV))


def _floats(a):
    a = np.ascontiguousarray(a, np.float32)
    return (ctypes.c_float * a.size)(*a.ravel().tolist())


def _matrix(K, C, seed):
    """any finite matrix will do for the kernels: uniform in (-1, 1) with one exact zero"""
    R = np.random.default_rng(seed).uniform(-1.0, 1.0, (K, C)).astype(np.float32)
    if K * C > 1:
        R[K - 1, C // 2] = 0.0
    return R


def _binary(name, shape, seed):
    return (synth_input(name, shape, seed, uniform=True) > 0.3).float()


def _tensors(f, r, C, K, plane, B, mode, unaligned=False, seed=19):
    """device tensors of a kernel case: arbitrary values and a soft mask [., 1, Hc, Wc] on the coarse grid"""
    vb, mb = MODES[mode]
    H, W = plane
    Hc, Wc = H // f, W // f
    t = dict(p=synth_input("xp", (B, C, H, W), seed), values=synth_input("xv", (B if vb else 1, K, Hc, Wc), seed + 1, uniform=True) * 2 - 1)
    if mb is not None:
        t["mask"] = synth_input("xm", (B if mb else 1, 1, Hc, Wc), seed + 2, uniform=True)
    t = {k: v.to(DEV) for k, v in t.items()}
    t["q"], t["out"] = _nan(B, K, Hc, Wc), _nan(B, C, H, W)
    if unaligned:
        t = {k: _offset_by_4_bytes(v) for k, v in t.items()}
    return t


def apply_mix(t, h, f, R, x=None, out=None, K=None, shape=None):
    x = t["p"] if x is None else x
    out = t["q"] if out is None else out
    B, C, H, W = x.shape if shape is None else shape
    rc = _lib.lib().eod_psf_apply_mix(_lib.ptr(x), None if h is None else _floats(h), 1 if h is None else len(h) // 2, f,
                                      None if R is None else _floats(R), len(R) if K is None else K, _lib.ptr(out), B, C, H, W, _stream())
    return rc, out


def residual_mix(t, h, f, lam, R, p=None, q=None, r=None, K=None, shape=None):
    p = t["p"] if p is None else p
    q = t["q"] if q is None else q
    B, C, H, W = p.shape if shape is None else shape
    v, m = t["values"], t.get("mask")
    rc = _lib.lib().eod_psf_residual_mix(_lib.ptr(p), _lib.ptr(v), _lib.ptr(m), float(lam), None if h is None else _floats(h),
                                         (1 if h is None else len(h) // 2) if r is None else r, f, None if R is None else _floats(R),
                                         len(R) if K is None else K, B, C, H, W, int(v is not None and v.shape[0] != B),
                                         int(m is not None and m.shape[0] != B), _lib.ptr(q), _stream())
    return rc, q


def update_mix(t, h, f, step, G, p=None, q=None, out=None, r=None, K=None, shape=None):
    p = t["p"] if p is None else p
    q = t["q"] if q is None else q
    out = t["out"] if out is None else out
    B, C, H, W = p.shape if shape is None else shape
    rc = _lib.lib().eod_psf_update_mix(_lib.ptr(p), _lib.ptr(q), float(step), None if h is None else _floats(h),
                                       (1 if h is None else len(h) // 2) if r is None else r, f, None if G is None else _floats(G),
                                       len(G[0]) if K is None else K, B, C, H, W, _lib.ptr(out), _stream())
    return rc, out


def _cpu(t, *names):
    return [None if t.get(k) is None else t[k].cpu() for k in names]


def _bound(t, h, f, R, lam, iters, solver="landweber", mu=0.0):
    """the product's BoundPsf on the tensors of t (misaligned ones stay misaligned)"""
    values, mask = _cpu(t, "values", "mask")
    kw = dict(solver="cg", damping=mu) if solver == "cg" else {}
    link = bind([PsfObservation(values, h, f, None, mask, lam, iters, response=R, **kw)], "test", tuple(t["p"].shape), 1, torch.device(DEV)).links[0]
    assert isinstance(link, CO.BoundPsf) and link.mixed
    link.values, link.mask = t["values"], t.get("mask")
    return link


# ------------------------------------------------------------------------------------------------------------ 1. the kernels, bit for bit
def _check(t, h, f, R, G, lam=0.625, step=0.9, iters=None):
    p, values, mask = _cpu(t, "p", "values", "mask")
    rc, got = apply_mix(t, h, f, R)
    assert rc == 0, _lib.lib().eod_last_error()
    assert torch.equal(got.cpu(), SP.apply(p, h, f, R))
    t["q"].fill_(float("nan"))
    rc, q = residual_mix(t, h, f, lam, R)
    want_q = SP.residual(p, values, h, f, R, mask, lam)
    assert rc == 0, _lib.lib().eod_last_error()
    assert torch.equal(q.cpu(), want_q) and bool(torch.isfinite(q).all())
    rc, out = update_mix(t, h, f, step, G)
    assert rc == 0, _lib.lib().eod_last_error()
    assert torch.equal(out.cpu(), SP.update(p, want_q, h, f, G, step)) and bool(torch.isfinite(out).all())
    if iters:                                                                  # BoundPsf.project, Landweber: iters x (residual, update with R^T)
        link = _bound(t, h, f, R, lam, iters)
        assert abs(link.step - SP.step32(h, f, *p.shape[2:], R)) <= EPS * link.step
        assert torch.equal(link.project(0, t["p"]).cpu(), SP.project(p, values, h, f, R, mask, lam, iters, link.step))
    t["q"].fill_(float("nan")), t["out"].fill_(float("nan"))


@pytest.mark.parametrize("unaligned", [False, True])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("f,r,C,K,plane", CASES)
def test_kernels_are_bit_exact(f, r, C, K, plane, B, unaligned):
    """values / mask full, broadcast and absent (eod_psf_apply_mix: no values at all), every pointer aligned or every pointer 4 bytes off:
    apply, residual and update torch.equal to the emulation; G is an arbitrary [C][K] matrix with a zero row"""
    h = TP._taps(f, r)
    R, G = _matrix(K, C, 100 + C), _matrix(C, K, 200 + C)
    if C > 1:
        G[C - 1] = 0.0
    for mode in MODES:
        t = _tensors(f, r, C, K, plane, B, mode, unaligned)
        _check(t, h, f, R, G)
        if C > 1:                                                              # a zero row of G: that channel comes out as p_c
            rc, q = residual_mix(t, h, f, 0.625, R)
            rc2, out = update_mix(t, h, f, 0.9, G)
            assert (rc, rc2) == (0, 0) and torch.equal(out[:, C - 1], t["p"][:, C - 1])


@pytest.mark.parametrize("one", ["p", "values", "mask", "q", "out"])
def test_one_unaligned_pointer_gives_the_aligned_launch_its_bits(one):
    for f, r, C, K, plane in ((2, 3, 4, 2, (12, 32)), (1, 2, 3, 1, (16, 16)), (8, 12, 5, 3, (32, 64))):   # (W and W / f multiples of 4: vector forms)
        h = TP._taps(f, r)
        R, G = _matrix(K, C, 7), _matrix(C, K, 8)
        a = _tensors(f, r, C, K, plane, 2, "full")
        u = dict(a, q=_nan(*a["q"].shape), out=_nan(*a["out"].shape))
        u[one] = _offset_by_4_bytes(u[one])
        (rc0, q0), (rc1, q1) = residual_mix(a, h, f, 0.75, R), residual_mix(u, h, f, 0.75, R)
        (rc2, o0), (rc3, o1) = update_mix(a, h, f, 0.9, G, q=q0), update_mix(u, h, f, 0.9, G, q=u["q"])
        assert (rc0, rc1, rc2, rc3) == (0, 0, 0, 0) and torch.equal(q0, q1) and torch.equal(o0, o1) and bool(torch.isfinite(o1).all())
        _check(u, h, f, R, G, iters=2)


@pytest.mark.parametrize("f,r,C,cs,plane", [(3, 5, 4, (1, 3), (12, 18)), (2, 3, 13, (0, 4, 5, 12), (140, 148)), (4, 6, 4, (0, 1, 2, 3), (32, 32)),
                                            (1, 12, 4, (2,), (40, 40)), (8, 12, 32, (0, 3, 7, 8, 15, 16, 30, 31), (24, 168))])
def test_one_hot_rows_are_the_unmixed_kernels(f, r, C, cs, plane):
    """R = rows of the identity, G = R^T (built here): eod_psf_residual_mix is torch.equal to eod_psf_residual with that channel list,
    eod_psf_update_mix to eod_psf_update, unlisted channels included"""
    h = TP._taps(f, r)
    K = len(cs)
    R = np.eye(C, dtype=np.float32)[list(cs)]
    G = np.ascontiguousarray(R.T)
    for mode in MODES:
        t = _tensors(f, r, C, K, plane, 2, mode)
        t["cs"] = cs
        rc0, q0 = TP.residual_(t, h, f, 0.625, q=_nan(*t["q"].shape))
        rc1, q1 = residual_mix(t, h, f, 0.625, R)
        rc2, o0 = TP.update_(t, h, f, 0.9, q=q0, out=_nan(*t["out"].shape))
        rc3, o1 = update_mix(t, h, f, 0.9, G, q=q1)
        assert (rc0, rc1, rc2, rc3) == (0, 0, 0, 0) and torch.equal(q0, q1) and torch.equal(o0, o1), mode
        rc4, a0 = TP.apply_(t, h, f, out=_nan(*t["q"].shape))
        rc5, a1 = apply_mix(t, h, f, R, out=_nan(*t["q"].shape))
        assert (rc4, rc5) == (0, 0) and torch.equal(a0, a1)
        for c in range(C):
            if c not in cs:
                assert torch.equal(o1[:, c], t["p"][:, c])


# ------------------------------------------------------------------------------------------------------------ 2. launch independence
@pytest.mark.parametrize("mode", ["full", "bcast"])
@pytest.mark.parametrize("f,r,C,K,plane", [(3, 5, 4, 2, (12, 18)), (5, 7, 3, 2, (35, 70)), (8, 12, 32, 8, (24, 168))])
def test_member_b_of_a_batch_and_a_second_run(f, r, C, K, plane, mode):
    h = TP._taps(f, r)
    R, G = _matrix(K, C, 11), _matrix(C, K, 12)
    t = _tensors(f, r, C, K, plane, 3, mode)
    rc1, q = residual_mix(t, h, f, 0.75, R)
    rc2, out = update_mix(t, h, f, 0.9, G)
    rc3, q2 = residual_mix(t, h, f, 0.75, R, q=_nan(*q.shape))
    rc4, out2 = update_mix(t, h, f, 0.9, G, out=_nan(*out.shape))
    assert (rc1, rc2, rc3, rc4) == (0, 0, 0, 0) and torch.equal(q, q2) and torch.equal(out, out2)
    for b in range(3):
        one = {k: (v[b:b + 1].contiguous() if v.shape[0] == 3 else v) for k, v in t.items()}
        one["q"], one["out"] = _nan(1, *q.shape[1:]), _nan(1, *out.shape[1:])
        rc1, q1 = residual_mix(one, h, f, 0.75, R)
        rc2, o1 = update_mix(one, h, f, 0.9, G)
        assert (rc1, rc2) == (0, 0) and torch.equal(q1, q[b:b + 1]) and torch.equal(o1, out[b:b + 1])


def test_a_launch_beyond_the_grid_cap_is_walked_by_the_stride_loop():
    """B = 2, C = 3, K = 2, f = 1 (tiles of 32 x 32), 1056 x 1048: 33 x 33 tiles a plane, so both launches hold more (plane, tile) pairs than
    EOD_PSF_GRID_BLOCKS and the first workgroups take a second one; sample 1 launched alone (below the cap) gives the same bits, and a corner
    of it the emulation's"""
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "eodiff.h")).read()
    cap = int(re.search(r"#define EOD_PSF_GRID_BLOCKS (\d+)", hdr).group(1))
    f, r, C, K, plane = 1, 2, 3, 2, (1056, 1048)
    assert 2 * K * 33 * 33 > cap > K * 33 * 33 and 2 * C * 33 * 33 > cap
    h = TP._taps(f, r)
    R, G = _matrix(K, C, 13), _matrix(C, K, 14)
    t = _tensors(f, r, C, K, plane, 2, "full")
    rc1, q = residual_mix(t, h, f, 0.75, R)
    rc2, out = update_mix(t, h, f, 0.9, G)
    one = {k: v[1:2].contiguous() for k, v in t.items()}
    one["q"], one["out"] = _nan(1, *q.shape[1:]), _nan(1, *out.shape[1:])
    rc3, q1 = residual_mix(one, h, f, 0.75, R)
    rc4, o1 = update_mix(one, h, f, 0.9, G)
    assert (rc1, rc2, rc3, rc4) == (0, 0, 0, 0) and torch.equal(q1, q[1:2]) and torch.equal(o1, out[1:2]) and bool(torch.isfinite(out).all())
    p, values, mask = (z[1:2, :, :40, :40].contiguous() for z in _cpu(t, "p", "values", "mask"))     # the corner 32 x 32 sees only p within r = 2
    assert torch.equal(q[1:2, :, :32, :32].cpu(), SP.residual(p, values, h, f, R, mask, 0.75)[:, :, :32, :32])


# ------------------------------------------------------------------------------------------------------------ 3. where the cg link lands
EXACT = [(PAN4, 4, 0.6, (32, 32), 0.0), (R32, 2, 0.3, (24, 28), 0.0), (R43, 3, 0.3, (12, 18), 0.0), (PAN4, 4, 0.6, (32, 32), 0.05)]


@pytest.mark.parametrize("case", range(4))
def test_48_iterations_land_on_the_dense_float64_solve(case):
    """the cases of tests/test_spectral_psf_host.py through BoundPsf.project: consistent observations made with psf_observe(response=), a binary
    mask that hides about 30 % of the coarse pixels, weight 1, 48 iterations.  The true relative residual, in float64 from the GPU's out
    (mu > 0: of the damped per-plane system, from the GPU's q_out), is <= 1e-5 and the correction out - p is within 1e-5 relative L2 of the
    dense float64 solve on kron(R, A_H, A_W) (section 9.9's gates)"""
    R, f, mtf, (H, W), mu = EXACT[case]
    h = PR.gaussian(f, mtf)
    K, C = np.shape(R)
    truth = (synth_input("et", (2, C, H, W), 41, uniform=True) * 2 - 1).to(DEV)
    t = dict(p=synth_input("ep", (2, C, H, W), 42).to(DEV), values=psf_observe(truth, h, f, response=R), mask=_binary("em", (2, 1, H // f, W // f), 43).to(DEV))
    assert torch.equal(t["values"].cpu(), SP.apply(truth.cpu(), h, f, R))
    link = _bound(t, h, f, R, 1.0, 48, "cg", mu)
    out = link.project(0, t["p"])
    q = link._coarse[1].cpu().numpy().astype(np.float64)
    p64, y64, m64 = (t[k].cpu().numpy().astype(np.float64) for k in ("p", "values", "mask"))
    want, c = SP.dense_correction64(p64, y64, h, f, R, m64, float(np.float32(mu)))
    got = out.cpu().numpy().astype(np.float64) - p64
    if mu == 0.0:
        res = m64 * (SP.apply64(out.cpu().numpy(), h, f, R) - y64)
    else:
        res = c - (m64 * np.einsum("yh,bkhw,xw->bkyx", GR.gram64(h, H, f), m64 * q, GR.gram64(h, W, f)) + float(np.float32(mu)) * q)
    e_res, e_cor = float(np.linalg.norm(res) / np.linalg.norm(c)), float(np.linalg.norm(got - want) / np.linalg.norm(want))
    print(f"case {case} ({C} -> {K}, f={f}, MTF {mtf}, {H} x {W}, mu={mu}): true residual / start {e_res:.3e}, correction vs the dense float64 solve {e_cor:.3e}")
    assert e_res <= 1e-5 and e_cor <= 1e-5


@pytest.mark.parametrize("how", ["weight 0", "mask 0"])
@pytest.mark.parametrize("solver", ["landweber", "cg"])
def test_nothing_observed_returns_the_input(solver, how):
    for f, r, C, K, plane in ((3, 5, 4, 2, (12, 18)), (6, 9, 1, 1, (6, 6)), (2, 3, 13, 2, (140, 148))):
        t = _tensors(f, r, C, K, plane, 2, "full")
        t["mask"] = torch.zeros_like(t["mask"]) if how == "mask 0" else (t["mask"] > 0.3).float()
        R = np.float32(np.eye(K, C) + 0.1)
        link = _bound(t, TP._taps(f, r), f, R, 0.0 if how == "weight 0" else 1.0, 3, solver)
        got = link.project(0, t["p"])
        assert got.data_ptr() != t["p"].data_ptr() and torch.equal(got, t["p"])


def test_psf_observe_with_a_response_is_the_operator():
    x = synth_input("ox", (2, 4, 24, 30), 3).to(DEV)
    h = gaussian_psf(6)
    assert torch.equal(psf_observe(x, h, 6, response=R43).cpu(), SP.apply(x.cpu(), h, 6, R43))
    assert torch.equal(psf_observe(x, h, 6, response=np.eye(4)[[1, 3]]), psf_observe(x, h, 6, [1, 3]))


# ------------------------------------------------------------------------------------------------------------ 4. refusals and defaults
def test_bad_arguments_return_the_error_and_leave_the_outputs_alone():
    f, C, K = 2, 3, 2
    h = np.array([0.25, 0.5, 0.25], np.float32)
    t = _tensors(f, 1, C, K, (16, 16), 2, "full")
    R, G = np.float32(R32), np.ascontiguousarray(np.float32(R32).T)
    shape = tuple(t["p"].shape)
    nq, n = t["q"].numel(), t["p"].numel()
    buf = _nan(2 * n)
    calls = []
    res = lambda **kw: calls.append(residual_mix(t, **{**dict(h=h, f=f, lam=1.0, R=R), **kw})[0])
    upd = lambda **kw: calls.append(update_mix(t, **{**dict(h=h, f=f, step=0.5, G=G), **kw})[0])
    app = lambda **kw: calls.append(apply_mix(t, **{**dict(h=h, f=f, R=R), **kw})[0])
    bad = lambda M, v: np.where(np.arange(M.size).reshape(M.shape) == 1, np.float32(v), M).astype(np.float32)
    for run, M, name in ((res, R, "R"), (upd, G, "G")):
        for bad_f in (0, 9, -1, 3, 5, 7):
            run(f=bad_f)
        run(r=-1), run(r=13), run(h=None)
        run(K=0), run(K=-1), run(K=4), run(K=9)                                            # outside 1 .. min(C, 8)
        run(shape=(2, 33, 16, 16)), run(shape=(2, 1, 16, 16)), run(shape=(0, 3, 16, 16))   # C > 32; K > C
        run(**{name: None, "K": 2})                                                        # a null matrix
        for v in (float("nan"), float("inf"), -float("inf")):
            run(**{name: bad(M, v)})
        for bad_h in ([0.25, float("nan"), 0.25], [-0.1, 1.2, -0.1], [0.2, 0.5, 0.3], [0.5, 0.0, 0.5]):
            run(h=np.asarray(bad_h, np.float32))
    big = dict(t, values=torch.zeros(2, 9, 8, 8, device=DEV), q=_nan(2, 9, 8, 8))          # K = 9 with room for it everywhere
    calls.append(residual_mix(big, h, f, 1.0, np.eye(9, 12, dtype=np.float32), p=torch.zeros(2, 12, 16, 16, device=DEV))[0])
    big["out"] = _nan(2, 12, 16, 16)
    calls.append(update_mix(big, h, f, 0.5, np.eye(12, 9, dtype=np.float32), p=torch.zeros(2, 12, 16, 16, device=DEV), q=torch.zeros(2, 9, 8, 8, device=DEV))[0])
    assert bool(torch.isnan(big["q"]).all()) and bool(torch.isnan(big["out"]).all())
    app(f=3), app(K=9), app(R=None, K=2), app(R=bad(R, float("nan"))), app(x=t["p"], out=t["p"]), app(shape=(2, 33, 16, 16))
    for lam in (-0.25, 1.5, float("nan"), float("inf")):
        res(lam=lam)
    for step in (0.0, -1.0, float("nan"), float("inf")):
        upd(step=step)
    none = types.SimpleNamespace(data_ptr=lambda: 0, shape=shape)
    res(p=none), res(q=none), upd(p=none), upd(q=none), upd(out=none), app(x=none), app(out=none)
    calls.append(residual_mix(dict(t, values=None), h, f, 1.0, R)[0])
    res(q=t["p"].view(-1)[:nq].view(t["q"].shape)), res(q=t["values"]), res(q=t["mask"].view(-1)[:1])   # an output on top of an input
    res(p=buf[:n].view(shape), q=buf[n - 4:n - 4 + nq].view(t["q"].shape))
    upd(out=t["p"]), upd(p=buf[:n].view(shape), out=buf[n // 2:n // 2 + n].view(shape))
    upd(q=buf[n - 4:n - 4 + nq].view(t["q"].shape), out=buf[:n].view(shape))
    torch.cuda.synchronize()
    assert calls and all(rc == -1 for rc in calls), calls
    for z in (t["q"], t["out"], buf):
        assert bool(torch.isnan(z).all())
    for z in (t["p"], t["values"], t["mask"]):                                             # (no input was written)
        assert bool(torch.isfinite(z).all())
    with pytest.raises(EodError):
        _lib.check(residual_mix(t, h, 9, 1.0, R)[0], "eod_psf_residual_mix")
    t8 = _tensors(1, 1, 32, 8, (8, 8), 1, "full")                                         # (the limits themselves are taken)
    assert residual_mix(t8, h, 1, 1.0, _matrix(8, 32, 1))[0] == 0 and update_mix(t8, h, 1, 0.5, _matrix(32, 8, 2))[0] == 0


@pytest.mark.parametrize("solver", ["landweber", "cg"])
def test_without_a_response_the_link_takes_the_launches_it_took_before(solver):
    """response=None (and no response at all) against the launches made directly: iters x (eod_psf_residual, eod_psf_update), or
    eod_psf_residual (weight 1) -> eod_psf_cg -> eod_psf_update (step 1 / f^2)"""
    f, r, plane, lam, iters = 4, 6, (32, 32), 0.625, 3
    h = TP._taps(f, r)
    t = TP._tensors(f, r, *plane, 2, 4, (1, 3), "k1")
    t["mask"] = (t["mask"] > 0.3).float()
    values, mask = _cpu(t, "values", "mask")
    shape = tuple(t["p"].shape)
    kw = dict(solver="cg", damping=0.05) if solver == "cg" else {}
    links = [bind([PsfObservation(values, h, f, t["cs"], mask, lam, iters, **kw, **extra)], "test", shape, 1, torch.device(DEV)).links[0]
             for extra in (dict(), dict(response=None))]
    assert not links[0].mixed and not links[1].mixed
    if solver == "landweber":
        p, bufs = t["p"], [_nan(*shape), _nan(*shape)]
        for it in range(iters):
            rc1, q = TP.residual_(t, h, f, lam, p=p)
            rc2, p = TP.update_(t, h, f, links[0].step, p=p, q=q, out=bufs[it % 2])
            assert (rc1, rc2) == (0, 0)
    else:
        rc1, c = TP.residual_(t, h, f, 1.0)
        tc = dict(d=c, c=c, mask=t["mask"], gy=links[0].gy, gx=links[0].gx, b=links[0].band, q=_nan(*c.shape), ws=TG._workspace(*c.shape))
        rc2, q = TG.cg_(tc, 0.05, lam, iters)
        rc3, p = TP.update_(t, h, f, 1.0 / (f * f), q=q)
        assert (rc1, rc2, rc3) == (0, 0, 0)
    for link in links:
        assert torch.equal(link.project(0, t["p"]), p)


# ------------------------------------------------------------------------------------------------------------ 5. whole calls
T_CALL, S_CALL = TS.T_CALL, TS.S_CALL
VARIANTS = {k: TS.VARIANTS[k] for k in ("plain", "repaint")}                               # plain, and with the RePaint mix
FORMS = ("cg", "chain")
H4, H1 = PR.gaussian(4), PR.gaussian(1)                                                    # f = 4, MTF 0.3: r = 6; f = 1: r = 2


def _links(form, shape, n_eval, seed, iters=8):
    """form "cg": one cg link with a response, K = 2 mixes of the three channels through the PSF at f = 4 under a binary coarse mask; "chain":
    [a pan band at f = 1 through gaussian(1) with a response, channels 0 and 2 through the PSF at f = 4 (channels=)], both cg.  One weight
    and one damping per evaluation and link."""
    B, C, H, W = shape
    truth = synth_input("lt", shape, seed, uniform=True) * 2 - 1
    w_down = [float(np.float32(w)) for w in np.linspace(1.0, 0.5, n_eval)]
    w_up = [float(np.float32(w)) for w in np.linspace(0.25, 1.0, n_eval)]
    damp = [float(np.float32(w)) for w in np.linspace(0.1, 0.0, n_eval)]
    t4, t1 = GR.tables(H4, 4, H, W), GR.tables(H1, 1, H, W)
    if form == "cg":
        return [dict(kind="mix", values=SP.apply(truth, H4, 4, R32), h=H4, f=4, R=R32, iters=iters, gy=t4[0], gx=t4[1],
                     mask=_binary("lm", (B, 1, H // 4, W // 4), seed), weights=w_down, dampings=damp)]
    return [dict(kind="mix", values=SP.apply(truth, H1, 1, PAN3), h=H1, f=1, R=PAN3, iters=iters, gy=t1[0], gx=t1[1], mask=None, weights=w_up, dampings=damp),
            dict(kind="cg", values=PR.apply(truth, H4, 4, (0, 2)), h=H4, f=4, channels=(0, 2), iters=iters, gy=t4[0], gx=t4[1], mask=None,
                 weights=w_down, dampings=damp)]


def _observation(links, sl=None):
    sl = sl or (lambda z, f: z)
    out = []
    for l in links:
        m = None if l["mask"] is None else sl(l["mask"], l["f"])
        if l["kind"] == "mix":
            out.append(PsfObservation(sl(l["values"], l["f"]), l["h"], l["f"], None, m, l["weights"], l["iters"], "cg", l["dampings"], response=l["R"]))
        else:
            out.append(PsfObservation(sl(l["values"], l["f"]), l["h"], l["f"], l["channels"], m, l["weights"], l["iters"], "cg", l["dampings"]))
    return out[0] if len(out) == 1 else out


def _cpu_links(links, k):
    return [SP.cg_link(l["values"], l["h"], l["f"], l["gy"], l["gx"], l["R"], l["mask"], l["weights"][k], l["dampings"][k], l["iters"])
            if l["kind"] == "mix" else
            GR.cg_link(l["values"], l["h"], l["f"], l["gy"], l["gx"], l["channels"], l["mask"], l["weights"][k], l["dampings"][k], l["iters"])
            for l in links]


def _call_case(form, n_lv, masked=False, resample=None, seed=103):
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
    """DDIMSampler.sample with cg links that carry a response (8 iterations, one weight and one damping per evaluation): the CPU loop is the
    oracle UNet with the fp32 emulation as the link.  Gates: TRAJ_TOL"""
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
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("form", FORMS)
def test_dpm_call_vs_cpu_loop(form, variant, prec):
    from eo_diffusion_amd.diffusion.dpm_solver import DPMSolverSampler
    levels = TC._dpm_levels()
    kw = VARIANTS[variant]
    c = _call_case(form, len(levels), **kw)
    ref, ref_p0 = _dpm_reference(form, variant, True)
    smp = DPMSolverSampler(_model(prec, T=T_CALL))
    extra = dict(x0=c["x0"].to(DEV), mask=c["mask"].to(DEV), mix_noises=c["mix_noises"]) if kw.get("masked") else {}
    out, inter = smp.sample(S_CALL, 2, (3, 16, 16), clip_denoised=True, x_T=c["x_T"], resample=kw.get("resample"), jump_noises=c["jump_noises"],
                            progress=False, log_every_t=1, observation=_observation(c["links"]), **extra)
    e_out, e_p0 = rel_l2(out.cpu(), ref), rel_l2(inter["pred_x0"][-1].cpu(), ref_p0)
    print(f"DPM-Solver++ + {form}, {variant} [{prec}]: rel-L2 vs the CPU loop: out {e_out:.3e}, last pred_x0 {e_p0:.3e} (gate {TRAJ_TOL[prec]:g})")
    assert e_out < TRAJ_TOL[prec] and e_p0 < TRAJ_TOL[prec]


def test_the_ancestral_sampler_returns_a_sample_that_meets_the_observation():
    """EODiffusion.sampling, weight 1, 32 iterations, K = 2 mixes at f = 4: the returned sample, seen through psf_observe(response=), meets
    `values` on the mask to <= 1e-4 relative (section 9.9's figure)"""
    m = _model("fp32x3", T=20)
    truth = (synth_input("at", (2, 3, 16, 16), 61, uniform=True) * 2 - 1).to(DEV)
    values, mask = psf_observe(truth, H4, 4, response=R32), _binary("am", (2, 1, 4, 4), 62).to(DEV)
    obs = PsfObservation(values.cpu(), H4, 4, None, mask.cpu(), 1.0, 32, "cg", response=R32)
    out = m.sampling(2, device=DEV, rng="philox", seed=3, progress=False, observation=obs)
    free = m.sampling(2, device=DEV, rng="philox", seed=3, progress=False)
    miss = lambda z: float((mask * (psf_observe(z, H4, 4, response=R32) - values)).double().norm() / (mask * values).double().norm())
    print(f"|m (A x - y)| / |m y| of the returned sample: cg iters=32 {miss(out):.3e}, no observation {miss(free):.3e}")
    assert bool(torch.isfinite(out).all()) and miss(out) <= 1e-4


# ------------------------------------------------------------------------------------------------------------ 6. scenes
def _scene_links(H, W, n, seed, B=1, f=4):
    truth = synth_input("st", (B, 3, H, W), seed, uniform=True) * 2 - 1
    h = PR.gaussian(f)
    w = [float(np.float32(v)) for v in np.linspace(1.0, 0.25, n)]
    d = [float(np.float32(v)) for v in np.linspace(0.0, 0.1, n)]
    gy, gx = GR.tables(h, f, H, W)
    return [dict(kind="mix", values=SP.apply(truth, h, f, R32), h=h, f=f, R=R32, iters=8, gy=gy, gx=gx,
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
    """overlap 8, tile 16, scene 24 x 36, f = 4, r = 6, K = 2 mixes: every coarse pixel's footprint crosses a tile edge and the solve couples
    the whole coarse plane.  The scene-level step is one pass over the scene: its recorded inputs go through the emulation, one step, under
    the fp32 gate"""
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
    mix = lambda *shape, R=R32, **kw: PsfObservation(z(*shape), h, 4, response=R, **kw)
    ok, ok_obs = mix(1, 2, H // 4, W // 4, solver="cg"), Observation(z(1, 3, H, W), (1, 2, 4))
    with Calls(m.model) as calls:
        for kw in (dict(response=R32, channels=[0, 1]), dict(response=PAN3), dict(response=R32, mask=z(1, 2, H // 4, W // 4)),
                   dict(response=[[0.5, 0.5, 0.0], [1.0, 1.0, 0.0]]), dict(response=np.eye(9, 12)), dict(response=np.full((2, 33), 0.1))):
            with pytest.raises(EodError):
                PsfObservation(z(1, 2, H // 4, W // 4), h, 4, **kw)
        with pytest.raises(EodError):
            psf_observe(z(1, 3, H, W, device=DEV), h, 4, [0, 1], response=R32)
        with pytest.raises(EodError):
            psf_observe(z(1, 3, H, W, device=DEV), h, 4, response=PAN4)
        for which, smp in TC._samplers(m).items():
            n = len(smp.make_dpm_schedule(S)) if which == "dpm" else 5
            extra = dict(verbose=False) if which == "ddim" else {}
            for kw in (dict(observation=ok, skip_known=True, mask=torch.ones(H, W), x0=z(1, 3, H, W)),       # skip_known + observation stays refused
                       dict(observation=[ok_obs, ok], skip_known=True, mask=torch.ones(H, W), x0=z(1, 3, H, W)),
                       dict(observation=mix(1, 1, H // 4, W // 4, R=PAN4)),                                  # a response for 4 channels, a state of 3
                       dict(observation=[ok_obs, mix(1, 1, H // 4, W // 4, R=PAN4)]),
                       dict(observation=mix(1, 2, H // 4, W // 4, solver="cg", damping=[0.1] * (n + 1))),    # dampings against the walk
                       dict(observation=mix(1, 2, 4, 4))):
                with pytest.raises(EodError):
                    smp.sample_scene(S, (H, W), progress=False, **extra, **kw)
            for kw in (dict(observation=ok), dict(observation=[mix(2, 1, s // 4, s // 4, R=PAN4)])):
                with pytest.raises(EodError):
                    smp.sample(S, 2, (3, s, s), progress=False, **extra, **kw)
        for kw in (dict(observation=mix(2, 1, s // 4, s // 4, R=PAN4)), dict(observation=[mix(2, 2, s // 4, s // 4, weight=[0.5] * (T - 1))])):
            with pytest.raises(EodError):
                m.sampling(2, device=DEV, progress=False, **kw)
    assert calls.batches == []
