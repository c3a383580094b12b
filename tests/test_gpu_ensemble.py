"""GPU: the ensemble statistics (csrc/ensemble.hip eod_scene_quantiles / eod_ensemble_stats, tiling.scene_quantiles, metrics.ensemble;
DESIGN.md section 9.14) against the emulation tests/ensemble_ref.py: the quantiles and the CRPS map bit for bit, every count exactly, every
float64 sum within the bound of a reordered sum, n * 2^-53 * sum |terms| (derived, not measured), at every member count that changes the
network, at the edges of a workgroup's share and of the vector width, on aligned and misaligned pointers; slices, repeatability, dirty
buffers, NaN locality, band independence, every refusal; and the module against torch.median / torch.quantile, scene_stats and a sampled
stack."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from eo_diffusion_amd import _lib
from eo_diffusion_amd import metrics as M
from eo_diffusion_amd.engine import quantile_rank
from eo_diffusion_amd.tiling import scene_quantiles, scene_stats
from tests import ensemble_ref as ER
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu
U = 2.0 ** -53

ENS_THREADS = 256                 # csrc/ensemble.hip ENS_THREADS: one pixel (scalar form) or ENS_VEC pixels (vector form) per thread and trip
ENS_VEC = 4                       # csrc/ensemble.hip ENS_VEC: the vector form (n % 4 == 0, 16-byte aligned pointers, B <= 16)
ENS_CHUNK = 512                   # csrc/ensemble.hip ENS_CHUNK: the pixels of one workgroup's share of a band (256 threads x 2)
ENS_GRID = 4096                   # csrc/ensemble.hip ENS_GRID: a band gets ceil(ENS_GRID / C) workgroups at most; with more chunks each walks several
QUANT_N = (1, ENS_VEC - 1, ENS_VEC, ENS_VEC + 1, 255, 256, 257, ENS_THREADS * ENS_VEC - 1, ENS_THREADS * ENS_VEC, ENS_THREADS * ENS_VEC + 1)
QS = (0.0, 1.0, 0.5, 0.05, 0.95, 1.0 / 3.0)
Q8 = (0.0, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99, 1.0)
MEMBERS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32, 33, 63, 64)


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _dev(a, off=False):
    """a (numpy or torch) on the device, 16-byte aligned or (off) 4 bytes behind a 16-byte boundary; the buffer ends within 12 bytes of the
    view's end (at it where the sizes allow), so that under EOD_TEST_EFENCE=1 the guard range follows the data"""
    if a is None:
        return None
    t = torch.as_tensor(a)
    start = 1 if off else 0
    buf = torch.empty((start + t.numel() + 3) // 4 * 4, dtype=t.dtype, device=DEV)
    v = buf[start:start + t.numel()]
    assert t.element_size() == 4 and v.data_ptr() % 16 == 4 * start
    v.copy_(t.reshape(-1))
    return v.view(t.shape)


def same(got, want):
    """bit for bit, a NaN for a NaN"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    nan = np.isnan(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def ranks_of(qs, B):
    return [quantile_rank(q, B) for q in qs]


def _data(B, n, seed):
    return (np.random.default_rng(seed).standard_normal((B, n)) * 2).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- eod_scene_quantiles
def call_quant(x, ranks, off=False, out_off=None, over=()):
    """x [B, n] numpy; returns (rc, out [Q, n] numpy, prefilled with -7)"""
    B, n = x.shape
    Q = len(ranks)
    xd = _dev(x, off)
    out = _dev(np.full((max(Q, 1), n), -7.0, dtype=np.float32), off if out_off is None else out_off)
    ks = (ctypes.c_int32 * max(Q, 1))(*[k for k, _ in ranks])
    fr = (ctypes.c_float * max(Q, 1))(*[f for _, f in ranks])
    kw = dict(x=xd.data_ptr(), out=out.data_ptr(), B=B, n=n, k=ks, frac=fr, Q=Q)
    kw.update(over)
    rc = _lib.lib().eod_scene_quantiles(kw["x"], kw["out"], kw["B"], kw["n"], kw["k"], kw["frac"], kw["Q"], _stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def check_quant(x, qs, off=False, out_off=None):
    ranks = ranks_of(qs, x.shape[0])
    rc, got = call_quant(x, ranks, off, out_off)
    assert rc == 0, _lib.lib().eod_last_error()
    assert same(got, ER.scene_quantiles(x, ranks)), (x.shape, qs, off)
    return got


@pytest.mark.parametrize("B", MEMBERS)
def test_quantiles_at_every_member_count(B):
    """n = 1031 (the scalar form) and 1032 (the vector form where B <= 16), aligned and 4 bytes off; the six quantiles and a Q = 8 call"""
    for n, off in ((1031, False), (1031, True), (1032, False), (1032, True)):
        x = _data(B, n, 10 * B + n)
        check_quant(x, QS, off)
    check_quant(_data(B, 1032, B), Q8)
    check_quant(_data(B, 1031, B), Q8, off=False, out_off=True)
    check_quant(_data(B, 77, B), (0.5,))


@pytest.mark.parametrize("B", (5, 64))
@pytest.mark.parametrize("n", QUANT_N)
def test_quantiles_at_the_edges_of_a_share_and_of_the_vector_width(B, n):
    x = _data(B, n, 1000 * B + n)
    a = check_quant(x, QS, off=False)
    b = check_quant(x, QS, off=True)
    assert same(a, b)


@pytest.mark.parametrize("B", (2, 5, 9, 16, 64))
def test_quantiles_of_equal_members_and_special_values(B):
    n = 64
    rng = np.random.default_rng(B)
    x = _data(B, n, 50 + B)
    x[:, 0] = 1.25                                              # equal members
    x[:, 1] = -0.0
    x[::2, 2], x[1::2, 2] = 0.0, -0.0                           # both zeros: -0.0 sorts below +0.0
    x[:, 3] = np.inf
    x[0, 4], x[-1, 4] = np.inf, -np.inf
    x[B // 2, 5] = np.nan                                       # one NaN: it sorts last
    x[:, 6] = np.nan                                            # all NaN
    x[:, 7] = (rng.integers(1, 1000, B).astype(np.uint32)).view(np.float32)        # denormals
    x[:, 8] = -(rng.integers(1, 1000, B).astype(np.uint32)).view(np.float32)
    x[0, 9] = -np.nan if B > 1 else 0.0                         # a NaN with the sign bit set
    x[:, 10] = np.float32(3.4e38)
    x[0, 10] = -np.float32(3.4e38)                              # hi - lo overflows
    for off in (False, True):
        got = check_quant(x, QS, off)
        check_quant(x, Q8, off)
    top = QS.index(1.0)
    assert np.isnan(got[top, 5]) and np.isnan(got[:, 6]).all() and (got[:, 0] == 1.25).all()
    assert np.signbit(got[QS.index(0.0), 2]) and not np.signbit(got[top, 2])


def test_a_slice_of_the_pixels_and_a_second_call_give_the_same_bits():
    for B in (5, 16, 64):
        x = _data(B, 4096 + 7, B)
        full = check_quant(x, QS)
        assert same(check_quant(x, QS), full)
        for a, b in ((0, 1000), (1024, 2049), (4000, 4103), (13, 14)):
            part = check_quant(np.ascontiguousarray(x[:, a:b]), QS, off=bool(a % 2))
            assert same(part, full[:, a:b])


def test_quantile_refusals_return_minus_one_with_a_message():
    x = _data(4, 64, 1)
    L = _lib.lib()
    xd = _dev(x)
    for ranks, over in (([(0, 0.0)], dict(x=0)), ([(0, 0.0)], dict(out=0)), ([(0, 0.0)], dict(k=None)), ([(0, 0.0)], dict(frac=None)),
                        ([(0, 0.0)], dict(B=0)), ([(0, 0.0)], dict(B=65)), ([(0, 0.0)], dict(n=0)), ([], dict()), ([(0, 0.0)] * 9, dict()),
                        ([(4, 0.0)], dict()), ([(-1, 0.0)], dict()), ([(1, 1.0)], dict()), ([(1, -0.25)], dict()), ([(1, math.nan)], dict()),
                        ([(3, 0.5)], dict()),                                       # x_(k+1) does not exist
                        ([(0, 0.0)], dict(out=xd.data_ptr() + 4 * 64)), ([(0, 0.0), (1, 0.0)], dict(out=xd.data_ptr() - 4 * 64 - 16))):
        if "out" in over and over["out"]:
            over = dict(over, x=xd.data_ptr())
        rc, got = call_quant(x, ranks, over=over)
        assert rc == -1, (ranks, over)
        assert L.eod_last_error()
        assert (got == -7.0).all()
    rc, got = call_quant(x, [(3, 0.0), (2, 0.5)])
    assert rc == 0 and same(got, ER.scene_quantiles(x, [(3, 0.0), (2, 0.5)]))


# ---------------------------------------------------------------------------------------------------------------- eod_ensemble_stats
def levels_of(ps, B):
    return [(quantile_rank((1 - p) / 2, B), quantile_rank((1 + p) / 2, B)) for p in ps]


LEVELS = {0: (), 2: (0.5, 0.9), 4: (0.0, 0.5, 0.9, 1.0)}


def call_stats(x, y, w, levels, off=False, want_map=True, ws=None, sums=None, counts=None, cmap=None, over=()):
    """x [B, C, H, W], y [C, H, W], w [H, W] or None (numpy).  Returns (rc, sums, counts, map) as device tensors, prefilled with rubbish"""
    B, C, H, W = x.shape
    L = _lib.lib()
    nl = len(levels)
    nc = 2 + B + 1 + nl
    if ws is None:
        size = int(L.eod_ensemble_stats_workspace_size(B, C, H, W))
        assert size > 0
        ws = torch.empty(size + 16, dtype=torch.uint8, device=DEV)[4 if off else 0:][:size]
    if sums is None:
        sums = torch.full((C, 5), -7.0, dtype=torch.float64, device=DEV)
    if counts is None:
        counts = torch.full((C, nc), 12345, dtype=torch.int64, device=DEV)
    if cmap is None and want_map:
        cmap = torch.full((C, H, W), -7.0, dtype=torch.float32, device=DEV)
    lk = (ctypes.c_int32 * max(2 * nl, 1))(*[k for lo, hi in levels for k in (lo[0], hi[0])])
    lf = (ctypes.c_float * max(2 * nl, 1))(*[f for lo, hi in levels for f in (lo[1], hi[1])])
    xd, yd, wd = _dev(x, off), _dev(y, off), _dev(w, off)
    kw = dict(x=xd.data_ptr(), truth=yd.data_ptr(), where=_lib.ptr(wd), B=B, C=C, H=H, W=W, level_k=lk, level_frac=lf, L=nl, sums=sums.data_ptr(),
              counts=counts.data_ptr(), map=_lib.ptr(cmap), ws=ws.data_ptr(), ws_bytes=ws.numel())
    kw.update(over)
    rc = L.eod_ensemble_stats(kw["x"], kw["truth"], kw["where"], kw["B"], kw["C"], kw["H"], kw["W"], kw["level_k"], kw["level_frac"], kw["L"],
                              kw["sums"], kw["counts"], kw["map"], kw["ws"], kw["ws_bytes"], _stream())
    torch.cuda.synchronize()
    return rc, sums, counts, cmap


def check_stats(x, y, w=None, levels=(), off=False, **kw):
    rc, sums, counts, cmap = call_stats(x, y, w, levels, off, **kw)
    assert rc == 0, _lib.lib().eod_last_error()
    want, mag, wcnt, wmap = ER.ensemble_stats(x, y, w, levels)
    got, gcnt = sums.cpu().numpy(), counts.cpu().numpy()
    assert np.array_equal(gcnt, wcnt), (gcnt, wcnt)
    bound = wcnt[:, :1] * U * mag
    fin = np.isfinite(want)
    err = np.abs(got - want)
    print(f"ensemble_stats {x.shape} L={len(levels)}: worst sum error {float(err[fin].max()) if fin.any() else 0.0:.3e} "
          f"(bound {float(bound[fin].max()) if fin.any() else 0.0:.3e})")
    assert np.array_equal(np.isnan(got), np.isnan(want)) and (err[fin] <= bound[fin]).all(), (err, bound)
    if cmap is not None:
        assert same(cmap.cpu().numpy(), wmap)
    return got, gcnt, None if cmap is None else cmap.cpu().numpy()


def _ensemble(B, C, H, W, seed):
    """draws around a truth, the truth inside their spread at most pixels"""
    rng = np.random.default_rng(seed)
    y = rng.random((C, H, W)).astype(np.float32)
    x = (y[None] + 0.1 * rng.standard_normal((B, C, H, W)) + 0.05 * rng.standard_normal((1, C, H, W))).astype(np.float32)
    return x, y


def _where(H, W, seed):
    return (np.random.default_rng(seed).random((H, W)) > 0.3).astype(np.float32)


@pytest.mark.parametrize("hw", ((1, 1), (5, 7), (33, 65), (7, 73), (16, 32), (19, 27)))
def test_stats_plane_sizes(hw):
    """1 x 1, odd planes (33 x 65: five workgroups per band), and one workgroup's share - 1 (7 x 73 = 511), the share (16 x 32) and the share
    + 1 (19 x 27 = 513)"""
    H, W = hw
    assert (H * W) in (1, 35, 2145, ENS_CHUNK - 1, ENS_CHUNK, ENS_CHUNK + 1)
    for i, (B, C, nl) in enumerate(((9, 3, 2), (2, 1, 0), (33, 3, 4), (1, 1, 2))):
        x, y = _ensemble(B, C, H, W, 100 * H + i)
        lv = levels_of(LEVELS[nl] if B > 1 else (0.0,) * nl, B)
        check_stats(x, y, None, lv, off=bool(i % 2))
        check_stats(x, y, _where(H, W, i), lv, off=not i % 2)


@pytest.mark.parametrize("B", (1, 2, 9, 33, 64))
def test_stats_member_counts_bands_and_levels(B):
    for C, (H, W), nl in ((13, (5, 7), 4), (3, (33, 65), 2), (1, (33, 65), 0)):
        x, y = _ensemble(B, C, H, W, B + C)
        lv = levels_of(LEVELS[nl], B)
        w = _where(H, W, B)
        got, cnt, cmap = check_stats(x, y, w, lv, off=True)
        assert (cnt[:, 0] == int(w.sum())).all() and (cnt[:, 2:2 + B + 1].sum(1) == cnt[:, 0]).all()
        g2, c2, _ = check_stats(x, y, w, lv, want_map=False)                        # a NULL map; aligned pointers: the same bits
        assert np.array_equal(got, g2) and np.array_equal(cnt, c2)
        _, c0, m0 = check_stats(x, y, np.zeros((H, W), np.float32), lv)             # nothing counted
        assert (c0 == 0).all() and np.isnan(m0).all()
        g1, c1, _ = check_stats(x, y, np.full((H, W), -2.5, np.float32), lv)        # any value but 0 counts (and where = NULL is that)
        gn, cn, _ = check_stats(x, y, None, lv)
        assert np.array_equal(g1, gn) and np.array_equal(c1, cn)


def test_stats_with_more_chunks_than_workgroups():
    """C = 32: 128 workgroups per band; 257 x 257 pixels are 130 chunks, so two workgroups walk two chunks each and keep their counts between
    them.  The first band has the bits of its single-band call, where every chunk has a workgroup of its own"""
    B, C, H, W = 2, 32, 257, 257
    assert -(-H * W // ENS_CHUNK) > -(-ENS_GRID // C)
    x, y = _ensemble(B, C, H, W, 21)
    w = _where(H, W, 21)
    lv = levels_of((0.5,), B)
    s, c, m = check_stats(x, y, w, lv)
    s1, c1, m1 = check_stats(x[:, :1], y[:1], w, lv)
    assert np.array_equal(s[0], s1[0]) and np.array_equal(c[0], c1[0]) and same(m[0], m1[0])


def test_stats_ties_and_the_ends_of_the_rank_histogram():
    B, C, H, W = 9, 2, 12, 11
    x, y = _ensemble(B, C, H, W, 3)
    y[0, 0, :] = x[4, 0, 0, :]                                   # the truth IS a member: ties
    y[0, 1, :] = x.min(0)[0, 1, :] - 1                           # below every member: rank 0
    y[0, 2, :] = x.max(0)[0, 2, :] + 1                           # above every member: rank B
    y[1, 3, :] = x.min(0)[1, 3, :]                               # the smallest member: rank 0 and a tie, covered by the 100 % interval
    x[:, 1, 4, :] = 0.5
    y[1, 4, :] = 0.5                                             # every member equals the truth
    y[1, 5, 0], x[0, 1, 5, 0] = 0.0, -0.0                        # -0.0 is below +0.0 in the key order: no tie
    y[1, 5, 1], x[:, 1, 5, 1] = np.nan, 0.25                     # a NaN truth: above every member, no tie, not covered
    lv = levels_of((0.5, 1.0), B)
    w = np.zeros((H, W), np.float32)
    w[0:3] = 1
    _, cnt, _ = check_stats(x, y, w, lv)
    assert cnt[0, 0] == 3 * W and cnt[0, 1] == W and cnt[0, 2] >= W and cnt[0, 2 + B] == W and cnt[0, 2 + B + 2] == W
    w[:] = 0
    w[3:5] = 1
    _, cnt, cmap = check_stats(x, y, w, lv)
    assert cnt[1, 1] == 2 * W and cnt[1, 2] == 2 * W and cnt[1, 2 + B + 2] == 2 * W and (cmap[1, 4] == 0).all()
    w[:] = 0
    w[5, :2] = 1
    got, cnt, _ = check_stats(x, y, w, lv)
    assert cnt[1, 0] == 2 and cnt[1, 1] == 0 and cnt[1, 2 + B] >= 1 and cnt[1, 2 + B + 1] <= 1                # (g and s2 do not see the truth)
    assert np.isnan(got[1, [0, 2, 4]]).all() and not np.isnan(got[1, [1, 3]]).any() and not np.isnan(got[0]).any()


def test_stats_dirty_buffers_repeatability_nan_locality_and_band_independence():
    B, C, H, W = 9, 13, 47, 45                                   # 2115 pixels: five workgroups per band
    x, y = _ensemble(B, C, H, W, 8)
    w = _where(H, W, 8)
    lv = levels_of((0.5, 0.9), B)
    L = _lib.lib()
    size = int(L.eod_ensemble_stats_workspace_size(B, C, H, W))
    ws = torch.full((size + 16,), 255, dtype=torch.uint8, device=DEV)[4:4 + size]        # 0xFF bytes, 4 bytes off, then reused
    s0, c0, m0 = check_stats(x, y, w, lv, ws=ws)
    sums = torch.full((C, 5), math.nan, dtype=torch.float64, device=DEV)
    counts = torch.full((C, 2 + B + 1 + 2), -1, dtype=torch.int64, device=DEV)
    cmap = torch.full((C, H, W), 3.0, dtype=torch.float32, device=DEV)
    for _ in range(2):                                           # the outputs and the workspace of the call before
        s1, c1, m1 = check_stats(x, y, w, lv, ws=ws, sums=sums, counts=counts, cmap=cmap)
        assert np.array_equal(s0, s1) and np.array_equal(c0, c1) and same(m0, m1)
    for c in (0, 6, 12):                                         # a band of the 13-band call has the bits of its single-band call
        sb, cb, mb = check_stats(x[:, c:c + 1], y[c:c + 1], w, lv, off=True)
        assert np.array_equal(sb[0], s0[c]) and np.array_equal(cb[0], c0[c]) and same(mb[0], m0[c])
    bad = x.copy()
    iy, ix = np.argwhere(w != 0)[5]
    bad[2, 4, iy, ix] = np.nan                                   # poisons band 4's sums, no other band's
    sn, cn, mn = check_stats(bad, y, w, lv)
    keep = [c for c in range(C) if c != 4]
    assert np.isnan(sn[4]).all() and np.array_equal(sn[keep], s0[keep]) and np.array_equal(cn[keep], c0[keep]) and same(mn[keep], m0[keep])
    assert cn[4, 0] == c0[4, 0] and cn[4, 2:2 + B + 1].sum() == c0[4, 0]
    ybad = y.copy()
    ybad[7, iy, ix] = np.nan                                     # and a NaN of the truth
    sn, cn, _ = check_stats(x, ybad, w, lv)
    keep = [c for c in range(C) if c != 7]
    assert np.isnan(sn[7, [0, 2, 4]]).all() and np.array_equal(sn[keep], s0[keep]) and np.array_equal(cn[keep], c0[keep])


def test_stats_refusals_return_minus_one_and_leave_the_outputs_untouched():
    B, C, H, W = 4, 3, 8, 8
    x, y = _ensemble(B, C, H, W, 2)
    w = np.ones((H, W), np.float32)
    lv = levels_of((0.5,), B)
    L = _lib.lib()
    sums = torch.full((C, 5), -7.0, dtype=torch.float64, device=DEV)
    counts = torch.full((C, 2 + B + 1 + 1), 12345, dtype=torch.int64, device=DEV)
    cmap = torch.full((C, H, W), -7.0, dtype=torch.float32, device=DEV)
    odd = torch.empty(1024, dtype=torch.uint8, device=DEV)
    xd = _dev(x)

    def lev(k_lo, f_lo, k_hi, f_hi):
        return dict(level_k=(ctypes.c_int32 * 2)(k_lo, k_hi), level_frac=(ctypes.c_float * 2)(f_lo, f_hi))

    for over in (dict(x=0), dict(truth=0), dict(sums=0), dict(counts=0), dict(ws=0), dict(level_k=None), dict(level_frac=None),
                 dict(B=0), dict(B=65), dict(C=0), dict(C=33), dict(H=0), dict(W=-1), dict(L=5), dict(L=-1),
                 lev(4, 0.0, 3, 0.0), lev(0, 0.0, -1, 0.0), lev(0, 1.0, 3, 0.0), lev(0, -0.5, 3, 0.0), lev(0, 0.0, 2, math.nan), lev(0, 0.0, 3, 0.5),
                 dict(ws_bytes=16), dict(sums=odd.data_ptr() + 4), dict(counts=odd.data_ptr() + 4), dict(counts=sums.data_ptr() + 8),
                 dict(x=xd.data_ptr(), map=xd.data_ptr()), dict(map=sums.data_ptr())):
        rc, _, _, _ = call_stats(x, y, w, lv, sums=sums, counts=counts, cmap=cmap, over=over)
        assert rc == -1, over
        assert L.eod_last_error()
    assert bool((sums.cpu() == -7.0).all()) and bool((counts.cpu() == 12345).all()) and bool((cmap.cpu() == -7.0).all())
    assert L.eod_ensemble_stats_workspace_size(0, 3, 8, 8) == -1 and L.eod_ensemble_stats_workspace_size(65, 3, 8, 8) == -1
    assert L.eod_ensemble_stats_workspace_size(4, 33, 8, 8) == -1 and L.eod_ensemble_stats_workspace_size(4, 3, 0, 8) == -1
    rc, s, c, _ = call_stats(x, y, w, lv, sums=sums, counts=counts, cmap=cmap)       # (and the same buffers are good arguments)
    assert rc == 0 and bool((c.cpu()[:, 0] == H * W).all())


# ---------------------------------------------------------------------------------------------------------------- the module
def test_scene_quantiles_against_torch_median_and_torch_quantile():
    for B in (1, 5, 9, 33):                                      # odd B: the median is a member
        x = torch.from_numpy(_data(B, 3 * 20 * 23, B).reshape(B, 3, 20, 23)).to(DEV)
        med = scene_quantiles(x, (0.5,))
        assert tuple(med.shape) == (1, 3, 20, 23) and torch.equal(med[0], torch.median(x, 0).values)
        assert torch.equal(scene_quantiles(x, 0.5), med)
    x = torch.from_numpy(_data(8, 3 * 32 * 32, 8).reshape(8, 3, 32, 32)).to(DEV)
    q = (0.05, 0.5, 0.95)
    out = torch.full((3, 3, 32, 32), math.nan, device=DEV)
    got = scene_quantiles(x, q, out=out)
    assert got.data_ptr() == out.data_ptr()
    want = torch.quantile(x.double(), torch.tensor(q, dtype=torch.float64, device=DEV), dim=0)
    bound = 4 * 2.0 ** -24 * float(x.abs().max())
    assert float((got.double() - want).abs().max()) <= bound
    assert float((got - torch.quantile(x, torch.tensor(q, device=DEV), dim=0)).abs().max()) <= 2 * bound      # torch's own fp32 form
    assert same(got.cpu().numpy().reshape(3, -1), ER.scene_quantiles(x.cpu().numpy().reshape(8, -1), ranks_of(q, 8)))
    view = x[:, :, ::2]                                          # a non-contiguous stack is copied, not refused
    assert torch.equal(scene_quantiles(view, q), scene_quantiles(view.contiguous(), q))
    for kw in (dict(out=x[:3]), dict(out=x.view(-1)[5:5 + 3 * 3 * 32 * 32].view(3, 3, 32, 32))):
        with pytest.raises(_lib.EodError, match="overlaps"):
            scene_quantiles(x, q, **kw)


@functools.lru_cache(maxsize=None)
def _sampled_stack():
    """four unconditional draws of a 40 x 57 scene by a tiny model (as tests/test_gpu_scene_stack.py builds one): shared, never written to"""
    from tests.test_gpu_scene_skip import _diffusion
    m = _diffusion("fp32x3", False, 6, None, s=16)
    stack = m.sampling_scene((40, 57), True, DEV, overlap=4, seed=5, progress=False, n_scenes=4)
    assert tuple(stack.shape) == (4, 3, 40, 57) and bool(torch.isfinite(stack).all())
    return stack


def test_ensemble_on_a_sampled_stack_agrees_with_the_emulation():
    stack = _sampled_stack()
    B, C, H, W = stack.shape
    rng = np.random.default_rng(4)
    truth = torch.from_numpy((stack.cpu().numpy().mean(0, keepdims=True) + 0.2 * rng.standard_normal((1, C, H, W))).astype(np.float32)).to(DEV)
    mask = torch.ones(1, 1, H, W, device=DEV)
    mask[0, 0, 10:30, 20:50] = 0
    hole = M.hole_of(mask)
    e, cmap = M.ensemble(stack, truth, where=hole, levels=(0.5, 0.9), return_map=True)
    lv = levels_of((0.5, 0.9), B)
    want, _, wcnt, wmap = ER.ensemble_stats(stack.cpu().numpy(), truth.cpu().numpy()[0], hole.cpu().numpy()[0, 0], lv)
    n = 20 * 30
    assert tuple(cmap.shape) == (1, C, H, W) and same(cmap.cpu().numpy()[0], wmap)
    assert (e.n == n).all() and np.array_equal(e.rank_hist, wcnt[:, 2:2 + B + 1]) and np.array_equal(e.ties, wcnt[:, 1])
    assert np.array_equal(e.coverage, wcnt[:, 2 + B + 1:] / n) and e.levels.tolist() == [0.5, 0.9]
    mae, rmse = want[:, 0] / n, np.sqrt(want[:, 2] / n)
    for got, ref, scale in ((e.crps, (want[:, 0] - want[:, 1]) / n, mae), (e.mae_members, mae, mae), (e.rmse_mean, rmse, rmse),
                            (e.spread, np.sqrt(want[:, 3] / n), rmse), (e.bias_mean, want[:, 4] / n, rmse),
                            (e.crps_fair, (want[:, 0] - want[:, 1] * B / (B - 1)) / n, mae)):
        assert got.dtype == np.float64 and got.shape == (C,) and (np.abs(got - ref) <= 1e-12 * scale).all()     # (600 terms: 600 * 2^-53 = 7e-14)
    assert (e.crps <= e.mae_members).all() and (e.crps_fair <= e.crps).all()
    assert np.allclose(e.spread_skill, math.sqrt((B + 1) / B) * e.spread / e.rmse_mean, rtol=1e-14)
    assert np.allclose(e.reliability_index, np.abs(e.rank_hist / n - 1 / (B + 1)).sum(1), rtol=1e-14)
    plain = M.ensemble(stack, truth, where=hole)
    assert all(np.array_equal(getattr(plain, f), getattr(e, f)) for f in M.Ensemble.FIELDS)
    assert "4 members" in M.describe_ensemble(e)
    none = M.ensemble(stack, truth, where=M.hole_of(torch.ones(1, 1, H, W, device=DEV)), levels=())     # an empty region: NaN, no error
    assert (none.n == 0).all() and np.isnan(none.crps).all() and none.coverage.shape == (C, 0)


def test_ensemble_of_one_member_and_the_spread_against_scene_stats():
    stack = _sampled_stack()
    B, C, H, W = stack.shape
    truth = stack[1:2] * 0.5
    one, cmap = M.ensemble(stack[:1], truth, levels=(), return_map=True)
    diff = (stack[:1].double() - truth.double()).abs()
    assert torch.equal(cmap, diff.float()) and np.isnan(one.crps_fair).all() and (one.spread == 0).all()
    assert np.abs(one.crps - diff.mean((0, 2, 3)).cpu().numpy()).max() <= 1e-12 and np.array_equal(one.crps, one.mae_members)
    e = M.ensemble(stack, truth)
    _, std = scene_stats(stack)
    want = (std.double() ** 2).sum((0, 2, 3)).cpu().numpy()
    got = e.spread ** 2 * e.n
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max(), (got, want)
