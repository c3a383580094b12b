"""GPU: anisotropic and shifted PSFs -- eod_psf_apply_xy / eod_psf_residual_xy / eod_psf_update_xy (csrc/psf.hip) and
PsfObservation(SeparablePsf(...)) on `observation=`.  The kernels bit for bit against tests/psf_xy_ref.py over the
shape list (tests/psf_xy_ref.py CASES) and three tap families; equal symmetric taps to the bits of the old entry points, plain and mixed;
the orientation on the device; batch members and the stride loop; the reach of a non-finite pixel; bad arguments to -1 with the outputs
untouched; the exact projection against a dense float64 solve; one whole call per sampler family against a CPU loop; bare taps to the
launches they took before."""
import os
import re

import numpy as np
import pytest
import torch

from eo_diffusion_amd import _lib
from eo_diffusion_amd._lib import EodError
from eo_diffusion_amd.diffusion import consistency as CO
from eo_diffusion_amd.diffusion.consistency import PsfObservation, SeparablePsf, bind, gaussian_psf, psf_observe
from eo_diffusion_amd.tiling import TilePlan
from oracle import schedule as SCH
from tests import ancestral_ref as AR
from tests import psf_cg_ref as GR
from tests import psf_ref as PR
from tests import psf_xy_ref as XY
from tests import spectral_ref as XR
from tests import test_gpu_consistency as TC
from tests import test_gpu_psf as TP
from tests import test_gpu_spectral as TS
from tests import test_gpu_spectral_psf as TM
from tests.gpu_util import DEV
from tests.helpers import rel_l2
from tests.synth import synth_input
from tests.test_gpu_dpm_solver import _eps_tiny, _nan, _offset_by_4_bytes
from tests.test_gpu_repaint_resample import _tiny
from tests.test_gpu_sampling import TRAJ_TOL, _model
from tests.test_gpu_scene import _diffusion
from tests.test_gpu_scene_skip import Calls

pytestmark = pytest.mark.gpu

EPS = XR.EPS
CASE_IDS = [f"f{f}-ry{ry}-rx{rx}-{H}x{W}" for f, ry, rx, (H, W) in XY.CASES]
CHANNELS = [(4, (1, 3)), (3, None)]                                  # (C, channels): a strict subset / all
MODES = ("full", "bcast", "nomask")                                  # TP.MASKS: per-sample values and mask / broadcast / no mask
_stream, _floats, _ints, _cpu = TP._stream, TP._floats, TP._ints, TP._cpu


def _list(cs, R):
    """(channels, matrix) of an _xy call: exactly one is given"""
    return (None, _floats(np.asarray(R, np.float32).ravel())) if R is not None else (_ints(cs), None)


def apply_xy(t, hy, hx, f, R=None, x=None, out=None, cs=None):
    x = t["p"] if x is None else x
    out = t["q"] if out is None else out
    cs = t.get("cs") if cs is None else cs
    K = len(R) if R is not None else len(cs)
    rc = _lib.lib().eod_psf_apply_xy(_lib.ptr(x), _floats(hy), len(hy) // 2, _floats(hx), len(hx) // 2, f, *_list(cs, R), K, _lib.ptr(out), *x.shape, _stream())
    return rc, out


def residual_xy(t, hy, hx, f, lam, R=None, p=None, q=None, cs=None, mask_c1=None):
    p = t["p"] if p is None else p
    q = t["q"] if q is None else q
    cs = t.get("cs") if cs is None else cs
    K = len(R) if R is not None else len(cs)
    B, C, H, W = p.shape
    v, m = t["values"], t.get("mask")
    c1 = int(R is not None or (m is not None and m.shape[1] != K)) if mask_c1 is None else mask_c1
    rc = _lib.lib().eod_psf_residual_xy(_lib.ptr(p), _lib.ptr(v), _lib.ptr(m), float(lam), _floats(hy), len(hy) // 2, _floats(hx), len(hx) // 2, f,
                                        *_list(cs, R), K, B, C, H, W, int(v.shape[0] != B), int(m is not None and m.shape[0] != B), c1, _lib.ptr(q), _stream())
    return rc, q


def update_xy(t, hy, hx, f, step, G=None, p=None, q=None, out=None, cs=None):
    p = t["p"] if p is None else p
    q = t["q"] if q is None else q
    out = t["out"] if out is None else out
    cs = t.get("cs") if cs is None else cs
    K = len(G[0]) if G is not None else len(cs)
    rc = _lib.lib().eod_psf_update_xy(_lib.ptr(p), _lib.ptr(q), float(step), _floats(hy), len(hy) // 2, _floats(hx), len(hx) // 2, f, *_list(cs, G), K,
                                      *p.shape, _lib.ptr(out), _stream())
    return rc, out


def _bound(t, hy, hx, f, lam, iters, **kw):
    """the product's BoundPsf on the tensors of t (misaligned ones stay misaligned)"""
    values, mask = _cpu(t, "values", "mask")
    link = bind([PsfObservation(values, SeparablePsf(hx, hy), f, t.get("cs"), mask, lam, iters, **kw)], "test", tuple(t["p"].shape), 1, torch.device(DEV)).links[0]
    assert isinstance(link, CO.BoundPsf) and link.xy
    link.values, link.mask = t["values"], t.get("mask")
    return link


# ------------------------------------------------------------------------------------------------------------ 1. the kernels, bit for bit
def _check(t, hy, hx, f, iters=(1, 3), lam=0.625):
    p, values, mask = _cpu(t, "p", "values", "mask")
    cs = t["cs"]
    H, W = p.shape[2:]
    step = XY.step32(hy, hx, f, H, W)
    rc, got = apply_xy(t, hy, hx, f)
    assert rc == 0, _lib.lib().eod_last_error()
    assert torch.equal(got.cpu(), XY.apply(p, hy, hx, f, cs))
    t["q"].fill_(float("nan"))
    rc, q = residual_xy(t, hy, hx, f, lam)
    want_q = XY.residual(p, values, hy, hx, f, cs, mask, lam)
    assert rc == 0 and torch.equal(q.cpu(), want_q) and bool(torch.isfinite(q).all())
    rc, out = update_xy(t, hy, hx, f, step)
    want = XY.update(p, want_q, hy, hx, f, cs, step)
    assert rc == 0 and torch.equal(out.cpu(), want) and bool(torch.isfinite(out).all())
    for c in range(p.shape[1]):
        if c not in cs:
            assert torch.equal(out[:, c], t["p"][:, c])                    # not listed: copied bit for bit
    for n in iters:
        link = _bound(t, hy, hx, f, lam, n)
        assert abs(link.tau - XY.tau64(hy, hx, f, H, W)) <= 1e-13 * link.tau and abs(link.step - step) <= EPS * step
        got = link.project(0, t["p"])
        assert torch.equal(got.cpu(), XY.project(p, values, hy, hx, f, cs, mask, lam, n, link.step)), n
    t["q"].fill_(float("nan")), t["out"].fill_(float("nan"))


@pytest.mark.parametrize("fam", XY.FAMILIES)
@pytest.mark.parametrize("f,ry,rx,plane", XY.CASES, ids=CASE_IDS)
def test_kernels_and_project_are_bit_exact(f, ry, rx, plane, fam):
    """B in {1, 3} x (C, channels) x mask form x iters in {1, 3}: apply, residual, update and BoundPsf.project"""
    hy, hx = XY.family(fam, f, ry, rx)
    for B in (1, 3):
        for C, channels in CHANNELS:
            for mode in MODES:
                _check(TP._tensors(f, 0, *plane, B, C, channels, mode), hy, hx, f)


@pytest.mark.parametrize("one", ["all", "p", "values", "mask", "q", "out"])
def test_unaligned_pointers_take_the_scalar_form_with_the_same_bits(one):
    """(4, 1, 12, (32, 64)): W and W / f are multiples of 4, both forms are vector forms when aligned"""
    f, ry, rx, plane = XY.CASES[4]
    hy, hx = XY.family("shift", f, ry, rx)
    t = TP._tensors(f, 0, *plane, 2, 4, (1, 3), "full", unaligned=one == "all")
    if one != "all":
        t[one] = _offset_by_4_bytes(t[one])
    _check(t, hy, hx, f, iters=(2,))


def test_the_mixed_form_is_bit_exact():
    """a dense R / G through the _xy entry points and a SeparablePsf link with response=, Landweber"""
    R = np.asarray(TM.R32, np.float32)
    for (f, ry, rx, plane), fam in zip(XY.CASES, XY.FAMILIES * 3):
        hy, hx = XY.family(fam, f, ry, rx)
        G = TM._matrix(3, 2, f)
        for mode in ("full", "bcast", "nomask"):
            t = TM._tensors(f, 0, 3, 2, plane, 2, mode)
            p, values, mask = _cpu(t, "p", "values", "mask")
            rc, got = apply_xy(t, hy, hx, f, R)
            got = got.clone()
            assert rc == 0 and torch.equal(got.cpu(), XY.apply(p, hy, hx, f, None, R)), _lib.lib().eod_last_error()
            rc, q = residual_xy(t, hy, hx, f, 0.625, R)
            want_q = XY.residual(p, values, hy, hx, f, None, mask, 0.625, R)
            assert rc == 0 and torch.equal(q.cpu(), want_q)
            rc, out = update_xy(t, hy, hx, f, 0.9, G)
            assert rc == 0 and torch.equal(out.cpu(), XY.update(p, want_q, hy, hx, f, None, 0.9, G))
            link = _bound(t, hy, hx, f, 0.625, 2, response=R)
            assert link.mixed and abs(link.step - XY.step32(hy, hx, f, *plane, response=R)) <= EPS * link.step
            assert torch.equal(link.project(0, t["p"]).cpu(), XY.project(p, values, hy, hx, f, None, mask, 0.625, 2, link.step, R))
            assert torch.equal(psf_observe(t["p"], SeparablePsf(hx, hy), f, response=R), got)


def test_psf_observe_with_a_separable_psf_is_the_operator():
    f, ry, rx, plane = XY.CASES[6]
    hy, hx = XY.family("shift", f, ry, rx)
    x = synth_input("ox", (2, 4, *plane), 3).to(DEV)
    assert torch.equal(psf_observe(x, SeparablePsf(hx, hy), f, [1, 3]).cpu(), XY.apply(x.cpu(), hy, hx, f, (1, 3)))
    assert torch.equal(psf_observe(x, SeparablePsf(hx, hy), f).cpu(), XY.apply(x.cpu(), hy, hx, f))
    const = torch.full((1, 2, *plane), 0.625, device=DEV)
    assert float((psf_observe(const, SeparablePsf(hx, hy), f) - 0.625).abs().max()) <= 4 * EPS          # N renormalises: a constant stays that constant


# ------------------------------------------------------------------------------------------------------------ 2. equal symmetric taps
@pytest.mark.parametrize("f,r,plane", TP.CASES)
def test_equal_symmetric_taps_have_the_bits_of_the_old_entry_points(f, r, plane):
    h = TP._taps(f, r)
    for B, mode in ((1, "full"), (3, "bcast"), (2, "nomask")):
        t = TP._tensors(f, r, *plane, B, 4, (1, 3), mode)
        step = PR.step32(h, f, *plane)
        old = [TP.apply_(t, h, f)[1].clone(), TP.residual_(t, h, f, 0.625)[1].clone(), TP.update_(t, h, f, step)[1].clone()]
        q_old = old[1]
        t["q"].fill_(float("nan")), t["out"].fill_(float("nan"))
        rc, a = apply_xy(t, h, h, f)
        assert rc == 0 and torch.equal(a, old[0])
        rc, q = residual_xy(t, h, h, f, 0.625)
        assert rc == 0 and torch.equal(q, old[1])
        rc, out = update_xy(t, h, h, f, step, q=q_old)
        assert rc == 0 and torch.equal(out, old[2])
        link = _bound(t, h, h, f, 0.625, 2)
        assert link.step == TP._bound(t, h, f, 0.625, 2).step
        assert torch.equal(link.project(0, t["p"]), TP._bound(t, h, f, 0.625, 2).project(0, t["p"]))
    onehot = np.zeros((2, 4), np.float32)
    onehot[0, 1] = onehot[1, 3] = 1.0
    for R, G in ((onehot, np.ascontiguousarray(onehot.T)), (TM._matrix(2, 4, f + r), TM._matrix(4, 2, f + r + 1))):
        for mode in ("full", "nomask"):
            t = TM._tensors(f, r, 4, 2, plane, 2, mode)
            old = [TM.apply_mix(t, h, f, R)[1].clone(), TM.residual_mix(t, h, f, 0.625, R)[1].clone()]
            old.append(TM.update_mix(t, h, f, 0.9, G, q=old[1])[1].clone())
            t["q"].fill_(float("nan")), t["out"].fill_(float("nan"))
            rc, a = apply_xy(t, h, h, f, R)
            assert rc == 0 and torch.equal(a, old[0]), _lib.lib().eod_last_error()
            rc, q = residual_xy(t, h, h, f, 0.625, R)
            assert rc == 0 and torch.equal(q, old[1])
            rc, out = update_xy(t, h, h, f, 0.9, G, q=old[1])
            assert rc == 0 and torch.equal(out, old[2])
            if R is onehot:                                              # ... which are those of the plain pair with that channel list
                tp = dict(t, cs=(1, 3), q=_nan(*t["q"].shape), out=_nan(*t["out"].shape))
                if "mask" in t:
                    tp["mask"] = t["mask"]
                assert torch.equal(residual_xy(tp, h, h, f, 0.625)[1], old[1])


# ------------------------------------------------------------------------------------------------------------ 3. orientation on the device
@pytest.mark.parametrize("x0", [5, 32])
def test_orientation_on_the_device(x0):
    """f = 1 (tiles of 32): an impulse at an interior pixel and at the first pixel of the second tile, so its neighbour lies across the border"""
    H, W, y0 = 40, 72, x0
    u = torch.zeros(1, 1, H, W)
    u[0, 0, y0, x0] = 1.0
    side, point = np.array([0.0, 0.75, 0.25], np.float32), np.array([1.0], np.float32)
    t = dict(p=u.to(DEV), q=_nan(1, 1, H, W), out=_nan(1, 1, H, W), cs=(0,))
    zero = torch.zeros(1, 1, H, W, device=DEV)
    for hy, hx, dy, dx in ((point, side, 0, 1), (side, point, 1, 0)):
        rc, a = apply_xy(t, hy, hx, 1)
        a = a.cpu()[0, 0]
        assert rc == 0 and a[y0, x0] == 0.75 and a[y0 - dy, x0 - dx] == 0.25 and a[y0 + dy, x0 + dx] == 0.0 and float(a.sum()) == 1.0
        assert torch.equal(a, XY.apply(u, hy, hx, 1)[0, 0])
        rc, o = update_xy(t, hy, hx, 1, 1.0, p=zero, q=t["p"])                          # out = 0 - A^T q
        o = -o.cpu()[0, 0]
        assert rc == 0 and o[y0, x0] == 0.75 and o[y0 + dy, x0 + dx] == 0.25 and o[y0 - dy, x0 - dx] == 0.0 and float(o.sum()) == 1.0


# ------------------------------------------------------------------------------------------------------------ 4. batch and stride
@pytest.mark.parametrize("mode", ["full", "bcast"])
@pytest.mark.parametrize("f,ry,rx,plane", [XY.CASES[1], XY.CASES[3], XY.CASES[5], XY.CASES[7]])
def test_member_b_of_a_batch_equals_the_launch_on_its_slice(f, ry, rx, plane, mode):
    hy, hx = XY.family("shift", f, ry, rx)
    t = TP._tensors(f, 0, *plane, 3, 4, (1, 3), mode)
    step = XY.step32(hy, hx, f, *plane)
    rc1, q = residual_xy(t, hy, hx, f, 0.75)
    rc2, out = update_xy(t, hy, hx, f, step)
    assert (rc1, rc2) == (0, 0)
    for b in range(3):
        one = {k: (v[b:b + 1].contiguous() if torch.is_tensor(v) and v.shape[0] == 3 else v) for k, v in t.items()}
        one["q"], one["out"] = _nan(1, *q.shape[1:]), _nan(1, *out.shape[1:])
        rc1, q1 = residual_xy(one, hy, hx, f, 0.75)
        rc2, o1 = update_xy(one, hy, hx, f, step)
        assert (rc1, rc2) == (0, 0) and torch.equal(q1, q[b:b + 1]) and torch.equal(o1, out[b:b + 1])


def test_a_plane_beyond_the_grid_cap_is_walked_by_the_stride_loop():
    """f = 5 (tiles of 20 x 20), one row of tiles: more tiles than EOD_PSF_GRID_BLOCKS workgroups; ry = 2, rx = 5"""
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "eodiff.h")).read()
    cap = int(re.search(r"#define EOD_PSF_GRID_BLOCKS (\d+)", hdr).group(1))
    H, W = 20, 20 * (cap + 37)
    hy, hx = XY.family("shift", 5, 2, 5)
    _check(TP._tensors(5, 0, H, W, 1, 1, None, "bcast"), hy, hx, 5, iters=(1,))


# ------------------------------------------------------------------------------------------------------------ 5. the reach of a non-finite pixel
@pytest.mark.parametrize("f,ry,rx,plane", [XY.CASES[1], XY.CASES[4], XY.CASES[7]], ids=[CASE_IDS[1], CASE_IDS[4], CASE_IDS[7]])
def test_a_non_finite_pixel_reaches_exactly_its_neighbourhood(f, ry, rx, plane):
    """one NaN in p: the apply is non-finite exactly at the coarse pixels whose blocks come within (ry, rx) of it, the update (finite q)
    exactly at the pixel itself, and with a NaN in q exactly within (ry, rx) of its block -- a shorter vector padded with zero taps to the
    longer radius would reach further (0 * NaN)"""
    H, W = plane
    hy, hx = XY.family("sym", f, ry, rx)                                                     # (a far tap that rounds to 0 still carries a NaN: 0 * NaN)
    y0, x0 = H // 2 + 1, W // 2 + 3
    t = TP._tensors(f, 0, H, W, 1, 1, None, "nomask")
    t["p"][0, 0, y0, x0] = float("nan")
    rc, a = apply_xy(t, hy, hx, f)
    fine = torch.zeros(H, W, dtype=torch.bool)
    fine[max(0, y0 - ry):y0 + ry + 1, max(0, x0 - rx):x0 + rx + 1] = True                     # the outputs of the blur that see the pixel
    want = fine.view(H // f, f, W // f, f).any(3).any(1)
    emu = XY.apply(t["p"].cpu(), hy, hx, f)
    assert rc == 0 and torch.equal(~torch.isfinite(a.cpu()[0, 0]), want) and torch.equal(~torch.isfinite(emu[0, 0]), want)
    q = synth_input("nq", (1, 1, H // f, W // f), 3).to(DEV)
    rc, out = update_xy(t, hy, hx, f, 0.5, q=q)
    only = torch.zeros(H, W, dtype=torch.bool)
    only[y0, x0] = True
    emu = XY.update(t["p"].cpu(), q.cpu(), hy, hx, f, None, 0.5)
    assert rc == 0 and torch.equal(~torch.isfinite(out.cpu()[0, 0]), only) and torch.equal(~torch.isfinite(emu[0, 0]), only)
    clean = TP._tensors(f, 0, H, W, 1, 1, None, "nomask")
    q[0, 0, y0 // f, x0 // f] = float("inf")
    rc, out = update_xy(clean, hy, hx, f, 0.5, q=q)
    block = torch.zeros(H, W, dtype=torch.bool)
    by, bx = y0 // f * f, x0 // f * f
    block[max(0, by - ry):by + f + ry, max(0, bx - rx):bx + f + rx] = True
    emu = XY.update(clean["p"].cpu(), q.cpu(), hy, hx, f, None, 0.5)
    assert rc == 0 and torch.equal(~torch.isfinite(out.cpu()[0, 0]), block) and torch.equal(~torch.isfinite(emu[0, 0]), block)


# ------------------------------------------------------------------------------------------------------------ 6. bad arguments
def test_bad_arguments_return_the_error_and_leave_the_outputs_alone():
    f = 2
    good = np.array([0.2, 0.5, 0.3], np.float32)
    t = TP._tensors(f, 1, 16, 16, 2, 3, (0, 2), "full")
    shape, L = tuple(t["p"].shape), _lib.lib()
    nq, n = t["q"].numel(), t["p"].numel()
    buf = _nan(2 * n)
    R, G = np.asarray(TM.R32, np.float32), TM._matrix(3, 2, 5)
    calls = []
    args = lambda hy, hx: (_floats(hy), len(hy) // 2, _floats(hx), len(hx) // 2)

    def res(hy=good, hx=good, cs=_ints((0, 2)), M=None, K=2, p=None, q=None, ry=None, rx=None, mask_c1=0, lam=1.0, f=f):
        a = list(args(hy, hx))
        a[1], a[3] = a[1] if ry is None else ry, a[3] if rx is None else rx
        calls.append(L.eod_psf_residual_xy(_lib.ptr(t["p"] if p is None else p), _lib.ptr(t["values"]), _lib.ptr(t["mask"]), lam, *a, f, cs, M, K,
                                           *shape, 0, 0, mask_c1, _lib.ptr(t["q"] if q is None else q), _stream()))

    def app(hy=good, hx=good, cs=_ints((0, 2)), M=None, K=2, x=None, out=None, ry=None, rx=None):
        a = list(args(hy, hx))
        a[1], a[3] = a[1] if ry is None else ry, a[3] if rx is None else rx
        calls.append(L.eod_psf_apply_xy(_lib.ptr(t["p"] if x is None else x), *a, f, cs, M, K, _lib.ptr(t["q"] if out is None else out), *shape, _stream()))

    def upd(hy=good, hx=good, cs=_ints((0, 2)), M=None, K=2, p=None, q=None, out=None, ry=None, rx=None, step=0.5, f=f):
        a = list(args(hy, hx))
        a[1], a[3] = a[1] if ry is None else ry, a[3] if rx is None else rx
        calls.append(L.eod_psf_update_xy(_lib.ptr(t["p"] if p is None else p), _lib.ptr(t["values"] if q is None else q), step, *a, f, cs, M, K, *shape,
                                         _lib.ptr(t["out"] if out is None else out), _stream()))

    wide = np.full(27, 1 / 27, np.float32)
    for run, M in ((res, _floats(R.ravel())), (app, _floats(R.ravel())), (upd, _floats(G.ravel()))):
        run(M=M)                                                                          # both the channel list and the matrix
        run(cs=None)                                                                      # neither
        run(ry=13, hy=wide), run(rx=13, hx=wide), run(ry=-1), run(rx=-1)                 # r 13 (and -1) on either axis
        for bad in ([0.5, 0.0, 0.5], [0.0, 0.0, 1.0], [-0.1, 1.2, -0.1], [0.2, 0.9, -0.1], [-0.0, 1.0, 0.0], [0.25, float("nan"), 0.25], [0.25, float("inf"), 0.25]):
            run(hy=np.asarray(bad, np.float32)), run(hx=np.asarray(bad, np.float32))      # centre tap 0; a negative tap; a negative zero; non-finite
        run(cs=_ints((2, 0))), run(cs=_ints((0, 3))), run(K=0), run(K=4)                  # the refusals of the old entry points
        run(cs=None, M=M, K=9), run(cs=None, M=M, K=0)                                    # with a matrix: K outside 1 .. min(C, 8)
    res(cs=None, M=_floats(R.ravel()), mask_c1=0)                                         # with R the mask is one plane
    res(f=3), res(f=0), res(f=9), upd(f=3), upd(f=0)
    for lam in (-0.25, 1.5, float("nan")):
        res(lam=lam)
    for step in (0.0, -1.0, float("nan"), float("inf")):
        upd(step=step)
    # overlapping buffers
    res(q=t["p"].view(-1)[:nq].view(t["q"].shape)), res(q=t["values"]), res(q=t["mask"])
    res(p=buf[:n].view(shape), q=buf[n - 4:n - 4 + nq].view(t["q"].shape))
    app(x=t["p"], out=t["p"])
    upd(out=t["p"]), upd(p=buf[:n].view(shape), out=buf[n // 2:n // 2 + n].view(shape))
    upd(q=buf[n - 4:n - 4 + nq].view(t["q"].shape), out=buf[:n].view(shape))
    torch.cuda.synchronize()
    assert calls and all(rc == -1 for rc in calls), calls
    for z in (t["q"], t["out"], buf):
        assert bool(torch.isnan(z).all())
    for z in (t["p"], t["values"], t["mask"]):                                            # (no input was written)
        assert bool(torch.isfinite(z).all())
    with pytest.raises(EodError):
        _lib.check(calls[0], "eod_psf_residual_xy")
    calls.clear()                                                                         # (the good arguments are taken)
    res(), app(), upd(), res(cs=None, M=_floats(R.ravel()), mask_c1=1), upd(cs=None, M=_floats(G.ravel()))
    torch.cuda.synchronize()
    assert calls == [0] * 5, (calls, L.eod_last_error())


# ------------------------------------------------------------------------------------------------------------ 7. the exact projection
CG_CASES = [(4, 6, 3, (32, 32)), (2, 3, 7, (12, 28))]


def _cg_distance(f, hy, hx, data_hy, data_hx, plane, form):
    """(max |p_gpu - p_64|, max |m (A_data x - y)|): BoundPsf.project with solver="cg", iters=48 under the taps (hy, hx) against the dense
    float64 solve of the same system, and the result re-observed through the operator (data_hy, data_hx) that made the values"""
    H, W = plane
    B, C = 2, 3
    truth = synth_input("ct", (B, C, H, W), f, uniform=True) * 2 - 1
    p = synth_input("cp", (B, C, H, W), f + 1)
    R = np.asarray(TM.R32, np.float32) if form == "response" else None
    cs = None if R is not None else (0, 2)
    y = torch.from_numpy(XY.apply64(truth.numpy(), data_hy, data_hx, f, cs, R).astype(np.float32))
    mask = TM._binary("cm", (B, 1, H // f, W // f), f + 2) if form == "mask" else None
    kw = dict(response=R) if R is not None else dict(channels=cs)
    o = PsfObservation(y, SeparablePsf(hx, hy), f, mask=mask, iters=48, solver="cg", **kw)
    link = bind([o], "test", (B, C, H, W), 1, torch.device(DEV)).links[0]
    got = link.project(0, p.to(DEV)).cpu().numpy().astype(np.float64)
    m = np.ones((B, 1, H // f, W // f)) if mask is None else mask.numpy().astype(np.float64)
    Ay, Ax = XY.line64(hy, H, f)[0], XY.line64(hx, W, f)[0]
    c = m * (XY.apply64(p.numpy(), hy, hx, f, cs, R) - y.numpy().astype(np.float64))
    z = m * GR.dense64(c, Ay @ Ay.T, Ax @ Ax.T, np.broadcast_to(m, c.shape))
    back = XY.adjoint64(z, hy, hx, f, H, W)
    want = p.numpy().astype(np.float64)
    if R is not None:
        want -= np.einsum("ck,bkhw->bchw", np.linalg.pinv(R.astype(np.float64)), back)
    else:
        want[:, list(cs)] -= back
    left = m * (XY.apply64(got, data_hy, data_hx, f, cs, R) - y.numpy().astype(np.float64))
    return float(np.abs(got - want).max()), float(np.abs(left).max())


@pytest.mark.parametrize("form", ["mask", "response"])
@pytest.mark.parametrize("f,ry,rx,plane", CG_CASES)
def test_the_exact_projection_under_an_anisotropic_shifted_psf(f, ry, rx, plane, form):
    """The distance to the dense float64 solve may be at most 2 x the distance the same test measures with the symmetric gaussian_psf(f) on
    both axes at the same shape (the Gram conditioning differs between taps).  And the point of it all: the values come from the shifted
    operator; projected with that operator the result re-observes them more closely than projected with the unshifted one."""
    hy, hx = gaussian_psf(f, 0.3, radius=ry, shift=0.37 * f), gaussian_psf(f, 0.5, radius=rx, shift=-0.37 * f)
    sym = gaussian_psf(f)
    d_sym, _ = _cg_distance(f, sym, sym, sym, sym, plane, form)
    d_xy, left_shifted = _cg_distance(f, hy, hx, hy, hx, plane, form)
    uy, ux = gaussian_psf(f, 0.3, radius=ry), gaussian_psf(f, 0.5, radius=rx)
    _, left_unshifted = _cg_distance(f, uy, ux, hy, hx, plane, form)
    print(f"cg f={f} ry={ry} rx={rx} {form}: max |p - p64| symmetric {d_sym:.3e}, anisotropic + shifted {d_xy:.3e}; "
          f"max |A x - y| under the shifted operator {left_shifted:.3e}, under the unshifted one {left_unshifted:.3e}")
    assert d_xy <= 2.0 * d_sym
    assert left_shifted < left_unshifted


# ------------------------------------------------------------------------------------------------------------ 8. whole calls
T_CALL, S_CALL = TS.T_CALL, TS.S_CALL
HY4, HX4 = XY.gaussian(4, 0.3, radius=6, shift=1.48), XY.gaussian(4, 0.5, radius=3, shift=-1.48)


def _links(shape, n_eval, seed, f=4, hy=HY4, hx=HX4):
    """one link: channels 0 and 2 through the anisotropic, shifted PSF at f under a soft coarse mask, 2 Landweber steps, one weight per evaluation"""
    B, C, H, W = shape
    truth = synth_input("lt", shape, seed, uniform=True) * 2 - 1
    w = [float(np.float32(v)) for v in np.linspace(1.0, 0.5, n_eval)]
    psf = SeparablePsf(hx, hy)
    step = float(np.float32(CO.psf_tau(psf, f, H, W) / (f * f)))
    assert abs(step - XY.step32(hy, hx, f, H, W)) <= EPS * step
    return [dict(values=XY.apply(truth, hy, hx, f, (0, 2)), hy=hy, hx=hx, f=f, channels=(0, 2), iters=2, step=step,
                 mask=synth_input("lm", (B, 1, H // f, W // f), seed, uniform=True), weights=w)]


def _observation(links, sl=None):
    sl = sl or (lambda z: z)
    return [PsfObservation(sl(l["values"]), SeparablePsf(l["hx"], l["hy"]), l["f"], l["channels"], sl(l["mask"]), l["weights"], l["iters"]) for l in links]


def _cpu_links(links, k):
    return [XY.psf_link(l["values"], l["hy"], l["hx"], l["f"], l["channels"], l["mask"], l["weights"][k], l["iters"], l["step"]) for l in links]


def test_ddim_call_vs_cpu_loop():
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    steps = TC._ddim_steps()
    c = TC._call_case(len(steps), seed=97)
    links = _links((2, 3, 16, 16), len(steps), 97)
    dd = SCH.ddim_tables(TC._tables()["alphas_cumprod"], steps, 0.5)
    ref, ref_p0 = XR.ddim_sampled(TC._tables(), dd, steps, _eps_tiny()[2], c["x_T"], c["step_noises"], lambda k: _cpu_links(links, k), None, None, None, None,
                                  c["jump_noises"])
    out, inter = DDIMSampler(_model("fp32x3", T=T_CALL)).sample(S_CALL, 2, (3, 16, 16), eta=0.5, verbose=False, progress=False, log_every_t=1, x_T=c["x_T"],
                                                                step_noises=c["step_noises"], observation=_observation(links))
    e_out, e_p0 = rel_l2(out.cpu(), ref), rel_l2(inter["pred_x0"][-1].cpu(), ref_p0)
    print(f"DDIM + SeparablePsf [fp32x3]: rel-L2 vs the CPU loop: out {e_out:.3e}, last pred_x0 {e_p0:.3e} (gate {TRAJ_TOL['fp32x3']:g})")
    assert e_out < TRAJ_TOL["fp32x3"] and e_p0 < TRAJ_TOL["fp32x3"]


def test_dpm_call_vs_cpu_loop():
    from eo_diffusion_amd.diffusion.dpm_solver import DPMSolverSampler
    levels = TC._dpm_levels()
    c = TC._call_case(len(levels), seed=97)
    links = _links((2, 3, 16, 16), len(levels), 97)
    ref, ref_p0 = XR.dpm_sampled(TC._tables(), levels, _eps_tiny()[2], c["x_T"], lambda k: _cpu_links(links, k), 2, True, None, None, None, None, c["jump_noises"])
    free, _ = XR.dpm_sampled(TC._tables(), levels, _eps_tiny()[2], c["x_T"], lambda k: [], 2, True, None, None, None, None, c["jump_noises"])
    out, inter = DPMSolverSampler(_model("fp32x3", T=T_CALL)).sample(S_CALL, 2, (3, 16, 16), clip_denoised=True, x_T=c["x_T"], progress=False, log_every_t=1,
                                                                     observation=_observation(links))
    e_out, e_p0 = rel_l2(out.cpu(), ref), rel_l2(inter["pred_x0"][-1].cpu(), ref_p0)
    print(f"DPM-Solver++ + SeparablePsf [fp32x3]: rel-L2 vs the CPU loop: out {e_out:.3e}, last pred_x0 {e_p0:.3e} (gate {TRAJ_TOL['fp32x3']:g})")
    assert e_out < TRAJ_TOL["fp32x3"] and e_p0 < TRAJ_TOL["fp32x3"]
    assert rel_l2(free, ref) > 10 * TRAJ_TOL["fp32"]                                        # (the observation matters)


def test_ancestral_sampling_call_vs_cpu_loop():
    T = 20
    hy, hx = XY.gaussian(2, 0.3, radius=3, shift=0.74), XY.gaussian(2, 0.5, radius=1, shift=-0.74)
    links = _links((2, 3, 16, 16), T, 71, f=2, hy=hy, hx=hx)
    x_T, noises = synth_input("qx", (2, 3, 16, 16), 71), synth_input("qn", (T, 2, 3, 16, 16), 71)
    ref = AR.ddpm_sampled(SCH.eo_cosine_tables(T), _tiny(), x_T, noises, lambda k: _cpu_links(links, k), True)
    free = AR.ddpm_sampled(SCH.eo_cosine_tables(T), _tiny(), x_T, noises, lambda k: [], True)
    out = _model("fp32x3", T=T).sampling(2, clipped_reverse_diffusion=True, device=DEV, x_T=x_T, noises=noises, progress=False, observation=_observation(links))
    err = rel_l2(out.cpu(), ref)
    print(f"ancestral + SeparablePsf [fp32x3]: rel-L2 vs the CPU loop = {err:.3e} (gate {TRAJ_TOL['fp32x3']:g})")
    assert bool(torch.isfinite(out).all()) and err < TRAJ_TOL["fp32x3"]
    assert rel_l2(free, ref) > 10 * TRAJ_TOL["fp32"]


def _emulate_last(smp, seen, links, k):
    x, e_t, hist, index, clip, obs = seen[-1]
    assert index == 0                                              # (lower-order final: first order)
    return XR.dpm_step(x.cpu(), e_t.cpu(), None, smp.ddim_alphas[index], smp.dpm_sqrt_one_minus_alphas[index], *smp.dpm_first[index], clip, _cpu_links(links, k))


def test_a_scene_footprint_across_a_tile_border_and_a_stack_of_scenes():
    """overlap 8, tile 16, scene 24 x 36, f = 4, (ry, rx) = (6, 3): the footprints cross tile edges.  The recorded inputs of the last
    evaluation go through the emulation, which the scene equals bit for bit; with n_scenes = 2 member b equals the single-scene call"""
    s, S, H, W, B = 16, 5, 24, 36, 2
    plan = TilePlan(H, W, s, 8)
    assert len(plan.origins_x) > 2
    smp = TC._samplers(_diffusion("fp32x3", False, 20, s=s))["dpm"]
    n = len(smp.make_dpm_schedule(S))
    links = _links((B, 3, H, W), n, 86)
    kw = TC._scene_kw("dpm", n, H, W, 86, B)
    stack, inter = smp.sample_scene(S, (H, W), overlap=8, progress=False, n_scenes=B, observation=_observation(links), **kw)
    assert stack.shape == (B, 3, H, W) and bool(torch.isfinite(stack).all()) and not torch.equal(stack[:1], stack[1:])
    for b in range(B):
        one_kw = {k: (v[b:b + 1] if k == "x_T" else v) for k, v in kw.items()}
        seen = TS._record(smp, "dpm") if b == 0 else None
        one, inter1 = smp.sample_scene(S, (H, W), overlap=8, progress=False, observation=_observation(links, lambda z: z[b:b + 1]), **one_kw)
        assert torch.equal(stack[b:b + 1], one) and torch.equal(inter["pred_x0"][-1][b:b + 1], inter1["pred_x0"][-1])
        if b == 0:
            assert len(seen) == n and seen[-1][0].shape == (1, 3, H, W) and seen[-1][-1] is not None
            cut = [dict(l, values=l["values"][:1], mask=l["mask"][:1]) for l in links]
            want_x, want = _emulate_last(smp, seen, cut, n - 1)
            assert torch.equal(inter1["pred_x0"][-1].cpu(), want) and torch.equal(one.cpu(), want_x)
            smp = TC._samplers(_diffusion("fp32x3", False, 20, s=s))["dpm"]                 # (an unwrapped sampler for the second member)
            smp.make_dpm_schedule(S)


def test_skip_known_is_still_refused_before_any_launch():
    from eo_diffusion_amd.diffusion.model import EODiffusion

    class Never(torch.nn.Module):
        def forward(self, x, t, cond=None, y=None):
            raise AssertionError("the network was reached")

    s, T, S, H, W = 16, 20, 5, 32, 48
    m = EODiffusion(Never(), timesteps=T, image_size=s, in_channels=3, device=DEV).to(DEV)
    z = torch.zeros
    ok = PsfObservation(z(1, 3, H // 4, W // 4), SeparablePsf(HX4, HY4), 4)
    with Calls(m.model) as calls, Launches() as n:
        for which, smp in TC._samplers(m).items():
            extra = dict(verbose=False) if which == "ddim" else {}
            for kw in (dict(observation=ok, skip_known=True, mask=torch.ones(H, W), x0=z(1, 3, H, W)), dict(observation=[ok], skip_known=True),
                       dict(observation=PsfObservation(z(1, 3, 4, 4), SeparablePsf(HX4, HY4), 4))):                 # ... and one that is not scene-sized
                with pytest.raises(EodError):
                    smp.sample_scene(S, (H, W), progress=False, **extra, **kw)
        assert calls.batches == [] and sum(n.counts.values()) == 0


# ------------------------------------------------------------------------------------------------------------ 9. bare taps: the launches of before
class Launches:
    """wrappers on the bound PSF symbols that count their calls"""
    NAMES = ("eod_psf_residual", "eod_psf_apply", "eod_psf_update", "eod_psf_residual_mix", "eod_psf_apply_mix", "eod_psf_update_mix",
             "eod_psf_residual_xy", "eod_psf_apply_xy", "eod_psf_update_xy", "eod_psf_cg")

    def __enter__(self):
        self.lib, self.counts = _lib.lib(), {k: 0 for k in self.NAMES}
        self.real = {k: getattr(self.lib, k) for k in self.NAMES}
        for k in self.NAMES:
            def counted(*a, _k=k):
                self.counts[_k] += 1
                return self.real[_k](*a)
            setattr(self.lib, k, counted)
        return self

    def __exit__(self, *exc):
        for k, fn in self.real.items():
            setattr(self.lib, k, fn)

    def taken(self):
        return {k: v for k, v in self.counts.items() if v}


@pytest.mark.parametrize("solver", ["landweber", "cg"])
def test_bare_taps_take_the_launches_they_took_before(solver):
    """a bare array-like psf: iters x (eod_psf_residual, eod_psf_update), or eod_psf_residual -> eod_psf_cg -> eod_psf_update, made directly
    and counted; with a response the _mix pair; a SeparablePsf of the same taps: the _xy pair, the same count and the same bits"""
    f, r, plane, lam, iters = 4, 6, (32, 32), 0.625, 3
    h = TP._taps(f, r)
    t = TP._tensors(f, r, *plane, 2, 4, (1, 3), "k1")
    t["mask"] = (t["mask"] > 0.3).float()
    values, mask = _cpu(t, "values", "mask")
    shape = tuple(t["p"].shape)
    kw = dict(solver="cg", damping=0.05) if solver == "cg" else {}
    dev = torch.device(DEV)
    bare = bind([PsfObservation(values, h, f, t["cs"], mask, lam, iters, **kw)], "test", shape, 1, dev).links[0]
    sep = bind([PsfObservation(values, SeparablePsf(h), f, t["cs"], mask, lam, iters, **kw)], "test", shape, 1, dev).links[0]
    assert not bare.xy and sep.xy
    if solver == "landweber":
        p, bufs = t["p"], [_nan(*shape), _nan(*shape)]
        for it in range(iters):
            rc1, q = TP.residual_(t, h, f, lam, p=p)
            rc2, p = TP.update_(t, h, f, bare.step, p=p, q=q, out=bufs[it % 2])
            assert (rc1, rc2) == (0, 0)
        n_pair, n_cg = iters, 0
    else:
        from tests import test_gpu_psf_cg as TG
        rc1, c = TP.residual_(t, h, f, 1.0)
        tc = dict(d=c, c=c, mask=t["mask"], gy=bare.gy, gx=bare.gx, b=bare.band, q=_nan(*c.shape), ws=TG._workspace(*c.shape))
        rc2, q = TG.cg_(tc, 0.05, lam, iters)
        rc3, p = TP.update_(t, h, f, 1.0 / (f * f), q=q)
        assert (rc1, rc2, rc3) == (0, 0, 0)
        n_pair, n_cg = 1, 1
    cg = {"eod_psf_cg": n_cg} if n_cg else {}
    with Launches() as n:
        got = bare.project(0, t["p"])
        assert n.taken() == {"eod_psf_residual": n_pair, "eod_psf_update": n_pair, **cg} and torch.equal(got, p)
    with Launches() as n:
        got = sep.project(0, t["p"])
        assert n.taken() == {"eod_psf_residual_xy": n_pair, "eod_psf_update_xy": n_pair, **cg} and torch.equal(got, p)
    R = np.asarray([[0.3, 0.2, 0.4, 0.1], [0.0, 0.5, -0.25, 0.25]], np.float32)
    tm = TM._tensors(f, r, 4, 2, plane, 2, "bcast")
    tm["mask"] = (tm["mask"] > 0.3).float()
    values, mask = _cpu(tm, "values", "mask")
    mixed = [bind([PsfObservation(values, psf, f, None, mask, lam, iters, response=R, **kw)], "test", shape, 1, dev).links[0] for psf in (h, SeparablePsf(h))]
    with Launches() as n:
        a = mixed[0].project(0, tm["p"])
        assert n.taken() == {"eod_psf_residual_mix": n_pair, "eod_psf_update_mix": n_pair, **cg}
    with Launches() as n:
        b = mixed[1].project(0, tm["p"])
        assert n.taken() == {"eod_psf_residual_xy": n_pair, "eod_psf_update_xy": n_pair, **cg} and torch.equal(a, b)
    with Launches() as n:
        x = synth_input("ox", (2, 4, 24, 32), 3).to(DEV)
        psf_observe(x, h, 4, [1, 3]), psf_observe(x, h, 4, response=R)
        assert n.taken() == {"eod_psf_apply": 1, "eod_psf_apply_mix": 1}
        psf_observe(x, SeparablePsf(h), 4, [1, 3]), psf_observe(x, SeparablePsf(h), 4, response=R)
        assert n.taken() == {"eod_psf_apply": 1, "eod_psf_apply_mix": 1, "eod_psf_apply_xy": 2}
