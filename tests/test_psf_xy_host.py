"""CPU: anisotropic and shifted PSFs (diffusion/consistency.py SeparablePsf / gaussian_psf(shift=) / psf_gram(symmetric=False) / psf_gram_pair,
tests/psf_xy_ref.py): every refusal that needs no GPU and what is accepted; the orientation pinned by hand; the
adjoint identity of the float64 reference (the reversal); the fp32 emulation against float64; the Gram tables, the step size and the padding
of the narrower table; the new phase bodies compiled for the host and run under the address and undefined-behaviour sanitizers as a
stand-alone program whose dumped outputs are compared with the emulation."""
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from eo_diffusion_amd._lib import EodError
from eo_diffusion_amd.diffusion import consistency as CO
from eo_diffusion_amd.diffusion.consistency import PsfObservation, SeparablePsf, bind, gaussian_psf, psf_cmax, psf_gram, psf_gram_pair, psf_observe, psf_tau
from tests import psf_cg_ref as GR
from tests import psf_ref as PR
from tests import psf_xy_ref as XY
from tests import spectral_ref as XR
from tests.helpers import bits_equal
from tests.synth import synth_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = XR.EPS
CASE_IDS = [f"f{f}-ry{ry}-rx{rx}-{H}x{W}" for f, ry, rx, (H, W) in XY.CASES]


def _v(*shape):
    return torch.zeros(*shape)


# ------------------------------------------------------------------------------------------------ refusals and acceptance
BAD_TAPS = [
    [[0.25, 0.5, 0.25]],                                      # not 1-D
    [], [0.5, 0.5],                                           # an even number of taps
    np.full(27, 1 / 27),                                      # r = 13
    "gauss", [True], np.ones(3, np.complex64),
    [0.25, float("nan"), 0.25], [float("inf")], [1e300],
    [-0.1, 1.2, -0.1], [-0.0, 1.0, -0.0], [0.5, 1.0, -0.0],   # negative, and a negative zero
    [0.5, 0.0, 0.5], [0.0, 0.0, 1.0],                         # centre tap 0
]


@pytest.mark.parametrize("bad", BAD_TAPS, ids=[str(i) for i in range(len(BAD_TAPS))])
def test_separable_psf_refuses_on_either_axis(bad):
    good = [0.2, 0.5, 0.3]
    for kw in (dict(x=bad), dict(x=good, y=bad), dict(x=bad, y=good)):
        with pytest.raises(EodError):
            SeparablePsf(**kw)
    with pytest.raises(EodError):
        SeparablePsf(SeparablePsf(good))


def test_what_is_accepted_and_what_bare_taps_still_refuse():
    s = SeparablePsf([0.2, 0.5, 0.3])                                                        # asymmetric, one vector for both axes
    assert s.taps_x.dtype == np.float32 and s.taps_x.tolist() == [float(np.float32(v)) for v in (0.2, 0.5, 0.3)] and s.taps_y is s.taps_x
    assert s.radii == (1, 1)
    s = SeparablePsf(gaussian_psf(2, radius=2), np.full(25, 0.04))                           # different radii
    assert s.radii == (12, 2)
    assert SeparablePsf([1.0], [0.1, 0.2, 0.4, 0.2, 0.1]).radii == (2, 0) and SeparablePsf(torch.tensor([0.0, 0.6, 0.4]), [1]).radii == (0, 1)
    one = SeparablePsf([0.0, 0.6, 0.4])                                                      # one-sided
    o = PsfObservation(_v(1, 2, 3, 4), one, 4, [0, 2], _v(1, 1, 3, 4), [0.0, 1.0], 8)
    assert o.psf is one and o.taps is None and o.iters == 8
    PsfObservation(_v(1, 2, 3, 4), SeparablePsf(gaussian_psf(4, shift=1.5), gaussian_psf(4, 0.5, shift=-0.2)), 4, solver="cg", iters=16)
    PsfObservation(_v(1, 2, 3, 4), SeparablePsf([0.1, 0.6, 0.3]), 4, response=[[0.5, 0.25, 0.25], [0.0, 1.0, -1.0]], mask=_v(1, 1, 3, 4))
    for bad in ([0.2, 0.5, 0.3], [0.3, 0.4, np.nextafter(np.float32(0.3), np.float32(1))], [0.0, 0.6, 0.4]):
        with pytest.raises(EodError):                                                        # bare asymmetric taps: still refused
            PsfObservation(_v(1, 2, 3, 4), bad, 4)
        with pytest.raises(EodError):
            psf_observe(_v(1, 3, 12, 12), bad, 2)
        with pytest.raises(EodError):
            psf_gram(bad, 2, 8)
        with pytest.raises(EodError):
            psf_gram(bad, 2, 8, symmetric=True)
        psf_gram(bad, 2, 8, symmetric=False)
    with pytest.raises(EodError):                                                            # (a CPU tensor: the kernel is mandatory)
        psf_observe(_v(1, 3, 12, 12), SeparablePsf([0.2, 0.5, 0.3]), 2)
    for kw in (dict(factor=5), dict(factor=2, channels=[3]), dict(factor=2, channels=[0], response=[[1.0, 0.0, 0.0]]), dict(factor=2, response=[[1.0, 0.0]])):
        with pytest.raises(EodError):
            psf_observe(_v(1, 3, 12, 12), SeparablePsf([0.2, 0.5, 0.3]), **kw)


def test_gaussian_shift():
    for f in range(1, 9):
        for mtf in (0.1, 0.3, 0.6, 1.0):
            assert bits_equal(torch.from_numpy(gaussian_psf(f, mtf, shift=0.0)), torch.from_numpy(gaussian_psf(f, mtf)))
            assert bits_equal(torch.from_numpy(gaussian_psf(f, mtf, None, 0.0)), torch.from_numpy(PR.gaussian(f, mtf) if mtf < 1 else np.ones(1, np.float32)))
        assert np.array_equal(gaussian_psf(f, radius=3, shift=0), gaussian_psf(f, radius=3))
    for kw in (dict(shift=2.01), dict(shift=-2.5), dict(shift=float("nan")), dict(shift=float("inf")), dict(shift="a"), dict(shift=True), dict(shift=None),
               dict(shift=0.5, mtf_nyquist=1.0), dict(shift=0.5, mtf_nyquist=1.0 - 1e-12), dict(shift=-0.3, mtf_nyquist=0.999999, radius=2)):
        with pytest.raises(EodError):                                     # (the last two: sigma so small that every tap underflows -- refused, not NaN taps)
            gaussian_psf(4, **kw)
    for f, mtf, shift in ((4, 0.3, 1.48), (4, 0.3, -2.0), (2, 0.5, 0.74), (8, 0.3, -2.96), (1, 0.3, 0.37)):
        h = gaussian_psf(f, mtf, shift=shift)
        r = h.size // 2
        assert h.dtype == np.float32 and np.array_equal(h, XY.gaussian(f, mtf, shift=shift)) and (h > 0).all() and h[r] > 0
        assert abs(float(h.astype(np.float64).sum()) - 1.0) <= 2 * EPS * h.size
        centroid = float((h.astype(np.float64) * np.arange(-r, r + 1)).sum())
        assert centroid * shift > 0 and abs(centroid - shift) <= (0.05 if 3 * CO.gaussian_sigma(f, mtf) + abs(shift) <= 12 else 0.5)   # the orientation: mass towards t > r for shift > 0
        assert np.array_equal(gaussian_psf(f, mtf, shift=-shift), h[::-1])                      # the mirror image, bit for bit
        SeparablePsf(h)
        with pytest.raises(EodError):
            PsfObservation(_v(1, 2, 3, 4), h, 4)


def test_bind_makes_an_xy_link():
    shape = (2, 3, 12, 16)
    hy, hx = gaussian_psf(4, shift=1.48), gaussian_psf(4, 0.5, radius=3, shift=-1.48)
    o = PsfObservation(_v(1, 2, 3, 4), SeparablePsf(hx, hy), 4, [0, 2], iters=3)
    link = bind(o, "call", shape, 3, "cpu").links[0]
    assert isinstance(link, CO.BoundPsf) and link.xy and (link.ry, link.rx) == (hy.size // 2, 3) and link.K == 2 and link.iters == 3
    assert link.tau == psf_tau(SeparablePsf(hx, hy), 4, 12, 16) and abs(link.tau - XY.tau64(hy, hx, 4, 12, 16)) <= 1e-13 * link.tau
    assert link.step == float(np.float32(link.tau / 16))
    bare = bind(PsfObservation(_v(1, 2, 3, 4), gaussian_psf(4), 4, [0, 2]), "call", shape, 3, "cpu").links[0]
    assert not bare.xy and bare.r == 6
    cg = bind(PsfObservation(_v(1, 2, 3, 4), SeparablePsf(hx, hy), 4, [0, 2], solver="cg", iters=16), "call", shape, 3, "cpu").links[0]
    b = max(-((-2 * (hy.size // 2)) // 4), 2)
    assert cg.band == b and tuple(cg.gy.shape) == (3, 2 * b + 1) and tuple(cg.gx.shape) == (4, 2 * b + 1)
    h = gaussian_psf(4)                                                                       # equal symmetric taps: today's tables, nothing padded
    same = bind(PsfObservation(_v(1, 2, 3, 4), SeparablePsf(h), 4, [0, 2], solver="cg", iters=16), "call", shape, 3, "cpu").links[0]
    old = bind(PsfObservation(_v(1, 2, 3, 4), h, 4, [0, 2], solver="cg", iters=16), "call", shape, 3, "cpu").links[0]
    assert same.band == old.band and bits_equal(same.gy, old.gy) and bits_equal(same.gx, old.gx) and same.step == old.step and same.tau == old.tau
    from eo_diffusion_amd.dropin.diffusion import consistency as D
    assert D.SeparablePsf is SeparablePsf and D.psf_gram_pair is psf_gram_pair


# ------------------------------------------------------------------------------------------------ orientation, by hand
def test_orientation_pinned_by_hand():
    H, W, y0, x0 = 7, 9, 3, 4
    u = torch.zeros(1, 1, H, W)
    u[0, 0, y0, x0] = 1.0
    side, point = np.array([0.0, 0.75, 0.25], np.float32), np.array([1.0], np.float32)
    a = XY.apply(u, point, side, 1)[0, 0]                                  # along x
    assert a[y0, x0] == 0.75 and a[y0, x0 - 1] == 0.25 and a[y0, x0 + 1] == 0.0 and float(a.sum()) == 1.0
    t = -XY.update(torch.zeros_like(u), u, point, side, 1)[0, 0]           # A^T of a coarse impulse (p = 0, step = 1: out = -A^T q)
    assert t[y0, x0] == 0.75 and t[y0, x0 + 1] == 0.25 and t[y0, x0 - 1] == 0.0 and float(t.sum()) == 1.0
    a = XY.apply(u, side, point, 1)[0, 0]                                  # the same along y
    assert a[y0, x0] == 0.75 and a[y0 - 1, x0] == 0.25 and a[y0 + 1, x0] == 0.0 and float(a.sum()) == 1.0
    t = -XY.update(torch.zeros_like(u), u, side, point, 1)[0, 0]
    assert t[y0, x0] == 0.75 and t[y0 + 1, x0] == 0.25 and t[y0 - 1, x0] == 0.0 and float(t.sum()) == 1.0
    a64 = XY.apply64(u.numpy(), point, side, 1)[0, 0]                      # the float64 reference agrees
    assert a64[y0, x0] == 0.75 and a64[y0, x0 - 1] == 0.25 and a64[y0, x0 + 1] == 0.0
    t64 = XY.adjoint64(u.numpy(), point, side, 1, H, W)[0, 0]
    assert t64[y0, x0] == 0.75 and t64[y0, x0 + 1] == 0.25 and t64[y0, x0 - 1] == 0.0


# ------------------------------------------------------------------------------------------------ float64: the adjoint
@pytest.mark.parametrize("fam", XY.FAMILIES)
@pytest.mark.parametrize("f,ry,rx,plane", XY.CASES, ids=CASE_IDS)
def test_adjoint_identity(f, ry, rx, plane, fam):
    """<A x, q> = <x, A^T q> with A^T = (N^-1 B0)^T D^T built from the orientation rule; and A^T by the contract's formula, the correlation
    with the REVERSED taps of (replicate(q) / f^2) / n -- with the forward taps in its place the identity fails for asymmetric taps"""
    H, W = plane
    hy, hx = XY.family(fam, f, ry, rx)
    rng = np.random.default_rng(f * 100 + ry)
    p, q = rng.standard_normal((2, 3, H, W)), rng.standard_normal((2, 3, H // f, W // f))
    lhs, rhs = float((XY.apply64(p, hy, hx, f) * q).sum()), float((p * XY.adjoint64(q, hy, hx, f, H, W)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1.0)
    ny, nx = XY.line64(hy, H, 1)[1], XY.line64(hx, W, 1)[1]
    w = np.repeat(np.repeat(q, f, 2), f, 3) / (f * f) / (ny[:, None] * nx[None, :])
    conv = lambda h, L: XY.line64(h, L, 1)[0] * XY.line64(h, L, 1)[1][:, None]                       # B0 of the taps h
    by_contract = np.einsum("yh,bkhw,xw->bkyx", conv(hy[::-1], H), w, conv(hx[::-1], W))
    want = XY.adjoint64(q, hy, hx, f, H, W)
    assert np.abs(by_contract - want).max() <= 1e-13 * max(1.0, np.abs(want).max())
    if fam != "sym" and max(ry, rx) > 0:
        wrong = np.einsum("yh,bkhw,xw->bkyx", conv(hy, H), w, conv(hx, W))
        assert np.abs(wrong - want).max() > 1e-3 * np.abs(want).max()
    assert np.abs(XY.apply64(np.full((1, 2, H, W), 0.625), hy, hx, f) - 0.625).max() <= 1e-13


# ------------------------------------------------------------------------------------------------ the emulation against float64
def _case32(f, ry, rx, H, W, B=2, C=3, channels=(0, 2)):
    p = synth_input("xp", (B, C, H, W), f + ry)
    K = len(channels)
    values = synth_input("xv", (B, K, H // f, W // f), f + rx + 1, uniform=True) * 2 - 1
    mask = synth_input("xm", (B, 1, H // f, W // f), f + ry + 2, uniform=True)
    return p, values, mask


@pytest.mark.parametrize("fam", XY.FAMILIES)
@pytest.mark.parametrize("f,ry,rx,plane", XY.CASES, ids=CASE_IDS)
def test_emulation_follows_float64(f, ry, rx, plane, fam):
    """the bound of tests/test_psf_host.py test_emulation_follows_float64 (64 eps max(1, |p|), three Landweber steps, weight 0.75, a soft mask),
    whose cases reach f = 8 and r = 12 as these do"""
    H, W = plane
    hy, hx = XY.family(fam, f, ry, rx)
    p, values, mask = _case32(f, ry, rx, H, W)
    bound = 64 * EPS * max(1.0, float(p.abs().max()))
    assert np.abs(XY.apply(p, hy, hx, f, (0, 2)).numpy() - XY.apply64(p.numpy(), hy, hx, f, (0, 2))).max() <= bound
    q = synth_input("xq", (2, 2, H // f, W // f), 5)
    got = XY.update(p, q, hy, hx, f, (0, 2), 0.5)
    want = p.numpy().astype(np.float64)
    want[:, [0, 2]] -= 0.5 * f * f * XY.adjoint64(q.numpy(), hy, hx, f, H, W)
    assert np.abs(got.numpy() - want).max() <= bound
    assert bits_equal(got[:, 1], p[:, 1])
    got = XY.project(p, values, hy, hx, f, (0, 2), mask, 0.75, iters=3)
    want = XY.landweber64(p.numpy(), values.numpy(), hy, hx, f, (0, 2), mask.numpy(), 0.75, iters=3)
    assert np.abs(got.numpy() - want).max() <= bound
    assert bits_equal(XY.project(p, values, hy, hx, f, (0, 2), mask, 0.0, iters=2), p)


def test_emulation_with_equal_symmetric_taps_is_the_symmetric_emulation():
    for f, r, H, W in ((2, 3, 12, 28), (4, 6, 32, 32), (8, 12, 8, 40)):
        h = PR.gaussian(f, 0.3, radius=r)
        p, values, mask = _case32(f, r, r, H, W)
        assert bits_equal(XY.apply(p, h, h, f, (0, 2)), PR.apply(p, h, f, (0, 2)))
        assert bits_equal(XY.project(p, values, h, h, f, (0, 2), mask, 0.75, iters=2, step=PR.step32(h, f, H, W)),
                          PR.project(p, values, h, f, (0, 2), mask, 0.75, iters=2))
        assert abs(XY.tau64(h, h, f, H, W) - PR.tau64(h, f, H, W)) <= 1e-13


# ------------------------------------------------------------------------------------------------ Gram, step size, padding
def _axis_taps():
    out = []
    for f, ry, rx, _ in XY.CASES:
        for fam in XY.FAMILIES:
            hy, hx = XY.family(fam, f, ry, rx)
            out += [(f, hy), (f, hx)]
    return out


def test_psf_gram_of_asymmetric_taps_is_a1_a1t():
    """the tolerance of tests/test_psf_cg_host.py test_psf_gram_is_a1_a1t: 1e-7 relative per entry plus fp32's subnormal spacing"""
    for f, h in _axis_taps():
        r = h.size // 2
        for L in (f, 3 * f, 13 * f):
            bands, b = psf_gram(h, f, L, symmetric=False)
            A1 = XY.line64(h, L, f)[0]
            G = A1 @ A1.T
            assert b == -((-2 * r) // f) and bands.dtype == np.float32 and bands.shape == (L // f, 2 * b + 1)
            want = GR.bands_of(G, b)
            assert np.all(np.abs(bands - want) <= 1e-7 * np.abs(want) + 2.0 ** -149)
            i, j = np.indices(G.shape)
            assert np.all(G[np.abs(i - j) > b] == 0.0)
            D = GR.dense_of(bands)
            assert np.array_equal(D, D.T)                                       # symmetric bit for bit
            assert np.all(bands[GR.bands_of(np.ones_like(G), b) == 0.0] == 0.0)


def test_psf_gram_symmetric_output_is_unchanged():
    """symmetric=True (and the default) takes the lines it took: the np.convolve form of n, spelled out here"""
    for f in range(1, 9):
        for r in (0, 1, 5, 12):
            h = PR.gaussian(f, 0.3, radius=r)
            for L in (f, 4 * f, 13 * f):
                a, b = psf_gram(h, f, L)
                a2, b2 = psf_gram(h, f, L, symmetric=True)
                a3, b3 = psf_gram(h, f, L, True)
                assert b == b2 == b3 and a.tobytes() == a2.tobytes() == a3.tobytes()
                h64, Lc, w = h.astype(np.float64), L // f, f + 2 * r
                n = np.convolve(np.ones(L), h64)[r:r + L]
                rows = np.zeros((Lc, w))
                for k in range(f):
                    inv = 1.0 / n[k::f]
                    for t in range(h64.size):
                        rows[:, k + t] += h64[t] * inv
                x = np.arange(Lc)[:, None] * f - r + np.arange(w)[None, :]
                rows[(x < 0) | (x >= L)] = 0.0
                rows /= f
                want = np.zeros((Lc, 2 * b + 1))
                for k in range(min(b, Lc - 1) + 1):
                    g = (rows[:Lc - k, k * f:] * rows[k:, :w - k * f]).sum(axis=1)
                    want[np.arange(Lc - k), b + k] = g
                    want[np.arange(k, Lc), b - k] = g
                assert a.tobytes() == want.astype(np.float32).tobytes()
                c, _ = psf_gram(h, f, L, symmetric=False)                         # the general form of n: the same table to rounding
                assert np.all(np.abs(c.astype(np.float64) - a) <= 1e-7 * np.abs(a) + 2.0 ** -149)


def test_psf_cmax_is_the_largest_column_sum():
    for f, h in _axis_taps():
        for L in (1, 2, h.size // 2 + 1, h.size, 3 * h.size + 1):
            want = XY.cmax_dense(h, L)
            assert abs(psf_cmax(h, L) - want) <= 1e-13 * want and want >= 1.0 - 1e-14
            assert abs(XY.cmax64(h, L) - want) <= 1e-13 * want                  # (the reference's own short form, used at scene widths)


@pytest.mark.parametrize("fam", XY.FAMILIES)
@pytest.mark.parametrize("f,ry,rx,plane", XY.CASES[:7], ids=CASE_IDS[:7])
def test_step_size_bounds_the_operator_norm(f, ry, rx, plane, fam):
    """tau ||A||_2^2 <= 1 by dense SVDs: ||A|| = ||A1(hy, H)|| ||A1(hx, W)|| (a Kronecker product), and the Kronecker matrix itself where small"""
    H, W = plane
    hy, hx = XY.family(fam, f, ry, rx)
    tau = psf_tau(SeparablePsf(hx, hy), f, H, W)
    assert abs(tau - XY.tau64(hy, hx, f, H, W)) <= 1e-13 * tau
    Ay, Ax = XY.line64(hy, H, f)[0], XY.line64(hx, W, f)[0]
    norm2 = float(np.linalg.svd(Ay, compute_uv=False)[0] * np.linalg.svd(Ax, compute_uv=False)[0]) ** 2
    assert tau * norm2 <= 1.0 + 1e-12
    if H * W <= 400:
        assert tau * float(np.linalg.svd(np.kron(Ay, Ax), compute_uv=False)[0]) ** 2 <= 1.0 + 1e-12
    assert psf_tau(hx, f, H, W) == float(f * f) / (psf_cmax(hx, H) * psf_cmax(hx, W))          # bare taps: the form it had


@pytest.mark.parametrize("fam", XY.FAMILIES)
@pytest.mark.parametrize("f,ry,rx,plane", XY.CASES, ids=CASE_IDS)
def test_the_padded_tables_are_the_kronecker_gram(f, ry, rx, plane, fam):
    H, W = plane
    hy, hx = XY.family(fam, f, ry, rx)
    gy, gx, b = psf_gram_pair(SeparablePsf(hx, hy), f, H, W)
    by, bx = -((-2 * ry) // f), -((-2 * rx) // f)
    assert b == max(by, bx) and gy.shape == (H // f, 2 * b + 1) and gx.shape == (W // f, 2 * b + 1) and gy.dtype == gx.dtype == np.float32
    assert gy.flags["C_CONTIGUOUS"] and gx.flags["C_CONTIGUOUS"]
    sym = lambda h: h.tobytes() == h[::-1].tobytes()
    assert gy[:, b - by:b + by + 1].tobytes() == psf_gram(hy, f, H, symmetric=sym(hy))[0].tobytes()      # the tables themselves, between zero columns
    assert gx[:, b - bx:b + bx + 1].tobytes() == psf_gram(hx, f, W, symmetric=sym(hx))[0].tobytes()
    assert not gy[:, :b - by].any() and not gy[:, b + by + 1:].any() and not gx[:, :b - bx].any() and not gx[:, b + bx + 1:].any()
    Ay, Ax = XY.line64(hy, H, f)[0], XY.line64(hx, W, f)[0]
    Gy, Gx = GR.dense_of(gy), GR.dense_of(gx)
    assert np.all(np.abs(Gy - Ay @ Ay.T) <= 1e-7 * np.abs(Ay @ Ay.T) + 2.0 ** -149) and np.all(np.abs(Gx - Ax @ Ax.T) <= 1e-7 * np.abs(Ax @ Ax.T) + 2.0 ** -149)
    if (H // f) * (W // f) <= 300:                                        # G_H (x) G_W = A A^T on the dense operator
        A = np.kron(Ay, Ax)
        want = A @ A.T
        assert np.all(np.abs(np.kron(Gy, Gx) - want) <= 2.5e-7 * np.abs(want) + 2.0 ** -149)
    rng = np.random.default_rng(f)                                        # and as an operator on a coarse plane, any size
    d = rng.standard_normal((H // f, W // f))
    want = XY.apply64(XY.adjoint64(d[None, None], hy, hx, f, H, W), hy, hx, f)[0, 0]
    assert np.abs(Gy @ d @ Gx.T - want).max() <= 1e-6 * max(1.0, np.abs(want).max())


# ------------------------------------------------------------------------------------------------ the kernels' bodies on the host
def _read_case(path):
    raw = open(path, "rb").read()
    f, ry, rx, H, W, B, C, K, mixed, mask_form = np.frombuffer(raw, np.int32, 10).tolist()
    data = np.frombuffer(raw, np.float32, offset=40)
    pos = [0]

    def take(*shape):
        n = int(np.prod(shape))
        out = data[pos[0]:pos[0] + n].reshape(shape).copy()
        pos[0] += n
        return out
    c = dict(f=f, ry=ry, rx=rx, H=H, W=W, mixed=mixed, mask_form=mask_form)
    c["hy"], c["hx"] = take(2 * ry + 1), take(2 * rx + 1)
    c["lam"], c["step"] = float(take(1)[0]), float(take(1)[0])
    Hc, Wc = H // f, W // f
    c["p"] = torch.from_numpy(take(B, C, H, W))
    c["values"] = torch.from_numpy(take(1 if mask_form == 1 else B, K, Hc, Wc))
    c["mask"] = None if mask_form == 3 else torch.from_numpy(take(1 if mask_form in (1, 2) else B, 1 if (mask_form == 2 or mixed) else K, Hc, Wc))
    c["R"], c["G"] = (take(K, C), take(C, K)) if mixed else (None, None)
    c["apply"], c["q"], c["out"] = (torch.from_numpy(take(B, K, Hc, Wc)), torch.from_numpy(take(B, K, Hc, Wc)), torch.from_numpy(take(B, C, H, W)))
    assert pos[0] == data.size
    return c


def test_phase_bodies_run_clean_under_sanitizers_and_match_the_emulation(tmp_path):
    """tests/psf_xy_host_check.cc: the per-axis phase bodies of csrc/psf_body.h compiled for the host with -fsanitize=address,undefined and run
    as a program of its own (nothing is loaded into this interpreter) over the shape list, three tap families, the plain and the mixed
    form, every access form, exactly sized buffers; what it dumps is compared bit for bit with the torch emulation"""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cxx = next((c for c in (os.path.join(rocm, "lib", "llvm", "bin", "clang++"), shutil.which("clang++"), shutil.which("g++")) if c and os.path.exists(c)), None)
    # no skip: this is the only out-of-bounds check of the per-axis phase bodies, and a machine that built the library has a C++ compiler
    assert cxx is not None, "no host C++ compiler (ROCm's clang++, clang++ or g++) to build tests/psf_xy_host_check.cc with"
    exe = str(tmp_path / "psf_xy_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "psf_xy_host_check.cc"), "-o", exe], check=True, capture_output=True, timeout=300)
    dump = tmp_path / "dump"
    dump.mkdir()
    run = subprocess.run([exe, str(dump)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.startswith("ok "), run.stdout[-2000:] + run.stderr[-2000:]
    files = sorted(glob.glob(str(dump / "case*.bin")))
    assert len(files) == len(XY.CASES) * 3 * 2
    seen = set()
    for path in files:
        c = _read_case(path)
        seen.add((c["f"], c["ry"], c["rx"], (c["H"], c["W"])))
        cs = None if c["mixed"] else (0, 2)
        assert bits_equal(c["apply"], XY.apply(c["p"], c["hy"], c["hx"], c["f"], cs, c["R"])), path
        q = XY.residual(c["p"], c["values"], c["hy"], c["hx"], c["f"], cs, c["mask"], c["lam"], c["R"])
        assert bits_equal(c["q"], q), path
        assert bits_equal(c["out"], XY.update(c["p"], q, c["hy"], c["hx"], c["f"], cs, c["step"], c["G"])), path
    assert seen == set(XY.CASES)
