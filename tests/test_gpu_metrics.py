"""GPU: the image-quality metrics (csrc/metrics.hip eod_ssim / eod_band_stats, eo_diffusion_amd/metrics.py) against
the float64 emulation tests/metrics_ref.py: the SSIM map bit for bit, every count exactly, every float64 sum within the bound of a reordered
sum, n * 2^-53 * sum |terms| (derived, not measured), at every tile and chunk edge; batch independence, repeatability, a dirty workspace,
misaligned base pointers, every refusal; and the module against harness.ssim / harness.psnr, the oracle and the independent host formulas."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from eo_diffusion_amd import _lib
from eo_diffusion_amd import harness as H_
from eo_diffusion_amd import metrics as M
from oracle import harness_ref as R
from tests import metrics_ref as MR
from tests.gpu_util import DEV
from tests.helpers import bits_equal
from tests.synth import synth_input

pytestmark = pytest.mark.gpu
U = 2.0 ** -53

SSIM_TILE = 32        # csrc/ssim_body.h SSIM_TILE: window positions per tile edge
# valid-region extents 1, one below, at and one above the tile edge, and two tiles plus one (H = extent + 2r: 11, 41, 42, 43, 75 at r = 5)
SSIM_EXTENTS = (1, SSIM_TILE - 1, SSIM_TILE, SSIM_TILE + 1, 2 * SSIM_TILE + 1)
BST_CHUNK = 2048      # csrc/metrics.hip BST_CHUNK: the pixels of one workgroup's share (256 threads x 8)
BST_PIXELS = (1, 255, 256, 257, BST_CHUNK - 1, BST_CHUNK, BST_CHUNK + 1)


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _dev(t, off=False):
    """t on the device, 16-byte aligned or (off) 4 bytes behind a 16-byte boundary"""
    if t is None:
        return None
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=DEV)
    v = buf[1:1 + t.numel()] if off else buf[:t.numel()]
    assert v.data_ptr() % 16 == (4 if off else 0)
    v.copy_(t.reshape(-1))
    return v.view(t.shape)


def _ws(size, fill=None, off=False):
    assert size > 0
    buf = torch.empty(size + 16, dtype=torch.uint8, device=DEV) if fill is None else torch.full((size + 16,), fill, dtype=torch.uint8, device=DEV)
    return buf[4:4 + size] if off else buf[:size]


def _taps(r, sigma=1.5):
    return np.ascontiguousarray(MR.gauss(2 * r + 1, sigma))


def call_ssim(p, t, w, taps, a=1.0, b=0.0, c1=1e-4, c2=9e-4, want_map=True, ws=None, sums=None, smap=None, over=()):
    """p, t, w: device tensors; over: arguments of the C call to replace.  Returns (rc, map [B, C, H, W] prefilled with NaN or None, sums [B, C, 2] prefilled with -7)"""
    B, C, H, W = p.shape
    r = (len(taps) - 1) // 2
    L = _lib.lib()
    if ws is None:
        ws = _ws(int(L.eod_ssim_workspace_size(B, C, H, W, r)))
    if smap is None and want_map:
        smap = torch.full((B, C, H, W), math.nan, dtype=torch.float32, device=DEV)
    if sums is None:
        sums = torch.full((B, C, 2), -7.0, dtype=torch.float64, device=DEV)
    kw = dict(pred=p.data_ptr(), ref=t.data_ptr(), where=_lib.ptr(w), B=B, ref_B=t.shape[0], where_B=1 if w is None else w.shape[0], C=C, H=H, W=W,
              taps=taps.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), r=r, a=a, b=b, c1=c1, c2=c2, map=_lib.ptr(smap), sums=sums.data_ptr(),
              ws=ws.data_ptr(), ws_bytes=ws.numel())
    kw.update(over)
    rc = L.eod_ssim(kw["pred"], kw["ref"], kw["where"], kw["B"], kw["ref_B"], kw["where_B"], kw["C"], kw["H"], kw["W"], kw["taps"], kw["r"], kw["a"],
                    kw["b"], kw["c1"], kw["c2"], kw["map"], kw["sums"], kw["ws"], kw["ws_bytes"], _stream())
    return rc, smap, sums


def check_ssim(p, t, w=None, r=5, a=1.0, b=0.0, c1=1e-4, c2=9e-4, off=False, **kw):
    """one call against the emulation: the map's valid region bit for bit, NaN (untouched) outside, n exact, the sum within the bound"""
    taps = _taps(r)
    rc, smap, sums = call_ssim(_dev(p, off), _dev(t, off), _dev(w, off), taps, a, b, c1, c2, **kw)
    assert rc == 0, _lib.lib().eod_last_error()
    want = MR.ssim_map(p, t, taps, c1, c2, a, b)
    B, C, Hh, W = p.shape
    s, n, mag = MR.ssim_sums(want, w, r)
    got = sums.cpu()
    assert torch.equal(got[..., 1], n), (got[..., 1], n)
    err, bound = (got[..., 0] - s).abs(), n * U * mag
    print(f"ssim {tuple(p.shape)} r={r}: sum error {float(err.max()):.3e} (bound {float(bound.max()):.3e})")
    assert bool((err <= bound).all()), (err, bound)
    if smap is not None:
        m = smap.cpu()
        assert bits_equal(m[:, :, r:Hh - r, r:W - r], want.float())
        outside = torch.ones(Hh, W, dtype=torch.bool)
        outside[r:Hh - r, r:W - r] = False
        assert bool(torch.isnan(m[:, :, outside]).all())
    return smap, sums


def _pair(tag, shape, ref_b=None, seed=1):
    gt = synth_input(tag + "_t", (ref_b or shape[0],) + tuple(shape[1:]), seed, uniform=True)
    return (gt + 0.05 * synth_input(tag + "_n", shape, seed + 1)).clip(0, 1), gt


# ---------------------------------------------------------------------------------------------------------------- eod_ssim
def test_ssim_valid_region_edges_on_both_axes():
    """r = 5: H and W independently over 11, 41, 42, 43, 75 -- the valid region ends at 1, one below, at and one above the tile edge and
    past two tiles; alternating base-pointer alignment"""
    i = 0
    for eh in SSIM_EXTENTS:
        for ew in SSIM_EXTENTS:
            p, t = _pair("gm_edge", (1, 2, eh + 10, ew + 10), seed=i)
            check_ssim(p, t, off=bool(i % 2))
            i += 1


@pytest.mark.parametrize("r", (0, 1, 5, 12))
def test_ssim_radii_batches_and_bands(r):
    """B in {1, 3}, C in {1, 3, 13}, a batch-1 truth, odd W, base pointers 4 bytes off a 16-byte boundary, the affine, a large data range"""
    Hh, W = SSIM_TILE + 1 + 2 * r, SSIM_TILE + 5 + 2 * r          # 2 x 2 tiles, W odd
    for B, C, ref_b, off in ((1, 1, None, False), (3, 3, 1, True), (1, 13, None, True), (3, 13, 1, False), (3, 1, None, True)):
        p, t = _pair(f"gm_rad{r}", (B, C, Hh, W), ref_b)
        check_ssim(p, t, r=r, off=off)
    p, t = _pair(f"gm_aff{r}", (3, 3, Hh, W), 1)
    check_ssim(p * 2 - 1, t * 2 - 1, r=r, a=0.5, b=0.5, off=True)
    check_ssim(p * 1e4, t * 1e4, r=r, c1=1e4, c2=9e4)
    check_ssim(p, t, r=r, want_map=False)                         # a NULL map pointer


def test_ssim_where_variants():
    B, C, Hh, W, r = 3, 3, 47, 51, 5
    p, t = _pair("gm_wh", (B, C, Hh, W), 1)
    m0, s0 = check_ssim(p, t)
    m1, s1 = check_ssim(p, t, torch.ones(B, 1, Hh, W))                       # all ones: where=None, bit for bit
    assert bits_equal(s0.cpu(), s1.cpu()) and bits_equal(m0.cpu()[:, :, r:-r, r:-r], m1.cpu()[:, :, r:-r, r:-r])
    _, s1 = check_ssim(p, t, torch.full((1, 1, Hh, W), -2.5), off=True)      # batch-1, any non-zero value counts
    assert bits_equal(s0.cpu(), s1.cpu())
    one = torch.zeros(B, 1, Hh, W)
    one[1, 0, r + 33, r + 2] = 1.0                                           # one counted pixel, in the second tile row
    one[0, 0, 2, 2] = 1.0                                                    # (outside the valid region: never counted)
    m, s = check_ssim(p, t, one)
    s = s.cpu()
    assert s[1, :, 1].tolist() == [1.0] * C and s[0, :, 1].tolist() == [0.0] * C
    assert torch.equal(s[1, :, 0], MR.ssim_map(p, t, _taps(r), 1e-4, 9e-4)[1, :, 33, 2])        # the sum of one term IS the term
    _, s = check_ssim(p, t, torch.zeros(1, 1, Hh, W))                        # none counted
    assert bool((s.cpu() == 0).all())
    w = (synth_input("gm_whm", (1, 1, Hh, W), 3, uniform=True) > 0.4).float()
    _, sa = check_ssim(p, t, w)                                              # a batch-1 where against B = 3
    _, sb = check_ssim(p, t, w.expand(B, 1, Hh, W).contiguous())
    assert bits_equal(sa.cpu(), sb.cpu())
    nan = w.clone()
    nan[0, 0, 20, 20] = math.nan                                             # NaN is not 0: counted
    _, sn = check_ssim(p, t, nan)
    assert float(sn.cpu()[0, 0, 1]) == float(sa.cpu()[0, 0, 1]) + (0.0 if w[0, 0, 20, 20] else 1.0)


def test_ssim_batch_independence_repeatability_and_a_dirty_workspace():
    B, C, Hh, W, r = 3, 3, 75, 44, 5
    p = synth_input("gm_bi_p", (B, C, Hh, W), 1, uniform=True)
    t = synth_input("gm_bi_t", (B, C, Hh, W), 2, uniform=True)
    w = (synth_input("gm_bi_w", (B, 1, Hh, W), 3, uniform=True) > 0.3).float()
    taps = _taps(r)
    pd, td, wd = _dev(p), _dev(t), _dev(w)
    size = int(_lib.lib().eod_ssim_workspace_size(B, C, Hh, W, r))
    ws = _ws(size, fill=255, off=True)                                       # 0xFF bytes, 4 bytes off, then reused
    rc, m0, s0 = call_ssim(pd, td, wd, taps, ws=ws)
    rc1, m1, s1 = call_ssim(pd, td, wd, taps, ws=ws)
    assert rc == 0 and rc1 == 0 and bits_equal(m0.cpu(), m1.cpu()) and bits_equal(s0.cpu(), s1.cpu())
    check_ssim(p, t, w, ws=ws)
    for b in range(B):                                                       # member b of the stack has the bits of its single call
        rc, mb, sb = call_ssim(_dev(p[b:b + 1], True), _dev(t[b:b + 1]), _dev(w[b:b + 1], True), taps)
        assert rc == 0 and bits_equal(mb.cpu(), m0.cpu()[b:b + 1]) and bits_equal(sb.cpu(), s0.cpu()[b:b + 1])


def test_ssim_nan_stays_visible_and_local():
    p, t = _pair("gm_nan", (2, 2, 40, 40), None)
    p[1, 0, 20, 20] = math.nan
    rc, m, s = call_ssim(_dev(p), _dev(t), None, _taps(5))
    s = s.cpu()
    assert rc == 0 and math.isnan(float(s[1, 0, 0])) and float(s[1, 0, 1]) == 900.0
    assert not bool(torch.isnan(s[0]).any()) and not math.isnan(float(s[1, 1, 0]))


def test_ssim_refusals_leave_the_outputs_untouched():
    p, t = _pair("gm_ref", (2, 3, 24, 24), None)
    pd, td, wd = _dev(p), _dev(t), _dev(torch.ones(2, 1, 24, 24))
    taps = _taps(5)
    bad_taps = taps.copy()
    bad_taps[3] = math.nan
    sums = torch.full((2, 3, 2), -7.0, dtype=torch.float64, device=DEV)
    smap = torch.full((2, 3, 24, 24), math.nan, dtype=torch.float32, device=DEV)
    odd = torch.empty(2 * 3 * 2 * 8 + 8, dtype=torch.uint8, device=DEV)
    for over in (dict(pred=0), dict(ref=0), dict(sums=0), dict(ws=0), dict(taps=None), dict(B=0), dict(C=0), dict(C=33), dict(H=0), dict(W=-1),
                 dict(ref_B=3), dict(where_B=3), dict(r=-1), dict(r=13), dict(H=10), dict(W=10), dict(a=math.nan), dict(b=math.inf),
                 dict(c1=math.nan), dict(c2=math.inf), dict(ws_bytes=16), dict(sums=odd.data_ptr() + 4), dict(map=pd.data_ptr()),
                 dict(taps=bad_taps.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))):
        rc, _, _ = call_ssim(pd, td, wd, taps, sums=sums, smap=smap, over=over)
        assert rc == -1, over
        assert _lib.lib().eod_last_error()
    torch.cuda.synchronize()
    assert bool((sums.cpu() == -7.0).all()) and bool(torch.isnan(smap.cpu()).all())
    L = _lib.lib()
    assert L.eod_ssim_workspace_size(2, 3, 10, 24, 5) == -1 and L.eod_ssim_workspace_size(2, 33, 24, 24, 5) == -1
    assert L.eod_ssim_workspace_size(2, 3, 24, 24, 13) == -1 and L.eod_ssim_workspace_size(0, 3, 24, 24, 5) == -1
    rc, _, s = call_ssim(pd, td, wd, taps, sums=sums, smap=smap)              # (and the same buffers are good arguments)
    assert rc == 0 and bool((s.cpu()[..., 1] == 14 * 14).all())


# ---------------------------------------------------------------------------------------------------------------- eod_band_stats
def call_bst(p, t, w, a=1.0, b=0.0, ws=None, band=None, sample=None, over=()):
    B, C, H, W = p.shape
    L = _lib.lib()
    if ws is None:
        ws = _ws(int(L.eod_band_stats_workspace_size(B, C, H, W)))
    if band is None:
        band = torch.full((B, C, 8), -7.0, dtype=torch.float64, device=DEV)
    if sample is None:
        sample = torch.full((B, 3), -7.0, dtype=torch.float64, device=DEV)
    kw = dict(pred=p.data_ptr(), ref=t.data_ptr(), where=_lib.ptr(w), B=B, ref_B=t.shape[0], where_B=1 if w is None else w.shape[0], C=C, H=H, W=W,
              a=a, b=b, band=band.data_ptr(), sample=sample.data_ptr(), ws=ws.data_ptr(), ws_bytes=ws.numel())
    kw.update(over)
    rc = L.eod_band_stats(kw["pred"], kw["ref"], kw["where"], kw["B"], kw["ref_B"], kw["where_B"], kw["C"], kw["H"], kw["W"], kw["a"], kw["b"],
                          kw["band"], kw["sample"], kw["ws"], kw["ws_bytes"], _stream())
    return rc, band, sample


def check_bst(p, t, w=None, a=1.0, b=0.0, off=False, **kw):
    rc, band, sample = call_bst(_dev(p, off), _dev(t, off), _dev(w, off), a, b, **kw)
    assert rc == 0, _lib.lib().eod_last_error()
    want, bound = MR.band_stats(p, t, w, a, b)
    got = band.cpu()
    assert torch.equal(got[..., 0], want[..., 0]) and torch.equal(got[..., 7], want[..., 7])       # n and max |p - t|: exact
    err = (got[..., 1:7] - want[..., 1:7]).abs()
    assert bool((err <= bound[..., 1:7]).all()), (err.max(), bound[..., 1:7].max())
    ws_, bs = MR.sample_stats(p, t, w, a, b)
    gs = sample.cpu()
    assert torch.equal(gs[:, 1:], ws_[:, 1:])                                                      # n_theta, n_undefined: exact
    assert bool(((gs[:, 0] - ws_[:, 0]).abs() <= bs).all()), (gs[:, 0], ws_[:, 0], bs)
    print(f"band_stats {tuple(p.shape)}: worst sum error {float(err.max()):.3e}, angle sum error {float((gs[:, 0] - ws_[:, 0]).abs().max()):.3e}")
    return band, sample


@pytest.mark.parametrize("pixels", BST_PIXELS)
def test_band_stats_pixel_counts(pixels):
    """1 pixel, the thread-count edges 255 / 256 / 257 and one workgroup's share +- 1; with and without where, a batch-1 truth, the affine"""
    Hh, W = (1, pixels) if pixels % 3 else (3, pixels // 3)
    p, t = _pair(f"gm_bs{pixels}", (2, 3, Hh, W), 1)
    p[0, :, 0, 0] = 0.0                                                      # a zero spectrum: no angle
    check_bst(p, t, off=True)
    w = (synth_input(f"gm_bw{pixels}", (2, 1, Hh, W), 3, uniform=True) > 0.3).float()
    w[1, 0, 0, 0] = 1.0
    check_bst(p * 2 - 1, t * 2 - 1, w, a=0.5, b=0.5)
    check_bst(p, t, torch.zeros(1, 1, Hh, W))                                # nothing counted: n = 0 and every sum 0


@functools.lru_cache(maxsize=None)
def _stack():
    """the 3 x 13 x 96 x 80 stack in [-1, 1] against a batch-1 truth, a batch-1 where: shared, never written to"""
    shape = (3, 13, 96, 80)
    gt = synth_input("gm_st_t", (1,) + shape[1:], 1, uniform=True) * 2 - 1
    p = (gt + 0.1 * synth_input("gm_st_n", shape, 2)).clip(-1, 1)
    w = (synth_input("gm_st_w", (1, 1, 96, 80), 3, uniform=True) > 0.25).float()
    return p, gt, w


def test_band_stats_stack_batch_independence_repeatability_and_a_dirty_workspace():
    p, t, w = _stack()
    ws = _ws(int(_lib.lib().eod_band_stats_workspace_size(*p.shape)), fill=255, off=True)
    b0, s0 = check_bst(p, t, w, a=0.5, b=0.5, ws=ws)
    b1, s1 = check_bst(p, t, w, a=0.5, b=0.5, ws=ws)
    assert bits_equal(b0.cpu(), b1.cpu()) and bits_equal(s0.cpu(), s1.cpu())
    for b in range(3):
        rc, bb, sb = call_bst(_dev(p[b:b + 1], True), _dev(t), _dev(w, True), 0.5, 0.5)
        assert rc == 0 and bits_equal(bb.cpu(), b0.cpu()[b:b + 1]) and bits_equal(sb.cpu(), s0.cpu()[b:b + 1])
    tb = t.expand_as(p).contiguous()                                         # the truth repeated is the batch-1 truth
    rc, bb, sb = call_bst(_dev(p), _dev(tb), _dev(w.expand(3, 1, 96, 80).contiguous()), 0.5, 0.5)
    assert rc == 0 and bits_equal(bb.cpu(), b0.cpu()) and bits_equal(sb.cpu(), s0.cpu())


def test_identical_inputs_and_a_nan_element():
    p, _, _ = _stack()
    pd = p.to(DEV)
    q = M.quality(pd, pd, affine=(0.5, 0.5))
    assert (q.rmse == 0).all() and np.isinf(q.psnr).all() and np.isinf(q.psnr_all).all() and (q.sam_deg == 0.0).all() and (q.max_abs == 0).all()
    assert (q.ssim == 1.0).all() and (q.ssim_all == 1.0).all() and (q.n == 96 * 80).all() and M.psnr(pd, pd) == math.inf
    x = p.clone()
    x[1, 4, 50, 7] = math.nan                                                # poisons band 4 of sample 1 (and that sample's angle), nothing else
    rc, band, sample = call_bst(_dev(x), _dev(p), None)
    band, sample = band.cpu(), sample.cpu()
    bad = torch.isnan(band)
    assert rc == 0 and bool(bad[1, 4, [1, 3, 5, 6, 7]].all()) and int(bad.sum()) == 5      # every sum and the maximum that p enters; n, sum t, sum t^2 stay
    assert math.isnan(float(sample[1, 0])) and not bool(torch.isnan(sample[[0, 2]]).any()) and sample[:, 1].tolist() == [7680.0] * 3
    rc, clean, _ = call_bst(_dev(p), _dev(p), None)
    assert rc == 0 and bits_equal(torch.where(bad, torch.zeros((), dtype=torch.float64), band), torch.where(bad, torch.zeros((), dtype=torch.float64), clean.cpu()))


def test_band_stats_refusals_leave_the_outputs_untouched():
    p, t = _pair("gm_bref", (2, 3, 8, 8), None)
    pd, td, wd = _dev(p), _dev(t), _dev(torch.ones(2, 1, 8, 8))
    band = torch.full((2, 3, 8), -7.0, dtype=torch.float64, device=DEV)
    sample = torch.full((2, 3), -7.0, dtype=torch.float64, device=DEV)
    odd = torch.empty(2 * 3 * 8 * 8 + 8, dtype=torch.uint8, device=DEV)
    for over in (dict(pred=0), dict(ref=0), dict(band=0), dict(sample=0), dict(ws=0), dict(B=0), dict(C=0), dict(C=33), dict(H=0), dict(W=0),
                 dict(ref_B=0), dict(ref_B=3), dict(where_B=3), dict(a=math.nan), dict(b=-math.inf), dict(ws_bytes=8), dict(band=odd.data_ptr() + 4),
                 dict(sample=odd.data_ptr() + 4), dict(sample=band.data_ptr() + 8)):
        rc, _, _ = call_bst(pd, td, wd, band=band, sample=sample, over=over)
        assert rc == -1, over
    torch.cuda.synchronize()
    assert bool((band.cpu() == -7.0).all()) and bool((sample.cpu() == -7.0).all())
    L = _lib.lib()
    assert L.eod_band_stats_workspace_size(2, 33, 8, 8) == -1 and L.eod_band_stats_workspace_size(2, 3, 0, 8) == -1
    rc, bnd, _ = call_bst(pd, td, wd, band=band, sample=sample)
    assert rc == 0 and bool((bnd.cpu()[..., 0] == 64).all())


# ---------------------------------------------------------------------------------------------------------------- the module
def test_module_ssim_and_psnr_against_the_harness_and_the_oracle():
    gt = synth_input("m_gt", (2, 3, 40, 48), 1, uniform=True)
    pred = (gt + 0.05 * synth_input("m_nz", (2, 3, 40, 48), 2)).clip(0, 1)
    pd, gd = pred.to(DEV), gt.to(DEV)
    got = M.ssim(pd, gd)
    assert abs(got - H_.ssim(pd, gd)) <= 1e-9 and abs(got - R.ssim(pred, gt)) <= 1e-9
    assert abs(M.ssim(pd * 2 - 1, gd * 2 - 1, 2.0, 7, 1.0, 0.02, 0.05) - R.ssim(pred * 2 - 1, gt * 2 - 1, 2.0, 7, 1.0, 0.02, 0.05)) <= 1e-9
    assert abs(M.ssim(pd * 2 - 1, gd * 2 - 1, affine=(0.5, 0.5)) - MR.ssim_mean(pred * 2 - 1, gt * 2 - 1, a=0.5, b=0.5)) <= 1e-12
    mean, smap = M.ssim(pd, gd, return_map=True)
    assert mean == got and tuple(smap.shape) == (2, 3, 30, 38) and bits_equal(smap.cpu(), MR.ssim_map(pred, gt, MR.gauss(), 1e-4, 9e-4).float())
    assert M.ssim(gd, gd) == 1.0
    assert abs(M.psnr(pd, gd) - H_.psnr(pd, gd)) <= 1e-4 and abs(M.psnr(pd, gd) - R.psnr(pred, gt)) <= 1e-12 * R.psnr(pred, gt)
    assert abs(M.psnr(pd * 2 - 1, gd * 2 - 1, 2.0) - H_.psnr(pd * 2 - 1, gd * 2 - 1, 2.0)) <= 1e-4
    hole = M.hole_of(torch.ones(2, 1, 40, 48, device=DEV))
    assert math.isnan(M.psnr(pd, gd, where=hole)) and math.isnan(M.ssim(pd, gd, where=hole))       # an empty region: NaN, no error
    band, sample = M.band_stats(pd, gd[:1])
    assert band.is_cuda and band.dtype == torch.float64 and tuple(band.shape) == (2, 3, 8) and tuple(sample.shape) == (2, 3)


def test_quality_field_by_field_and_a_stack_against_its_draws():
    """quality() on the 3 x 13 x 96 x 80 stack with where and affine = (0.5, 0.5) against tests/metrics_ref.quality_ref (centred moments, from
    the definitions): 1e-9 relative -- the raw-moment variances lose E[x^2] / var, about 4, against the centred ones and both sides carry
    n * 2^-53 = 7e-13 of summation error; counts are exact"""
    p, t, w = _stack()
    pd, td, wd = p.to(DEV), t.to(DEV), w.to(DEV)
    q = M.quality(pd, td, where=wd, affine=(0.5, 0.5), ratio=2)
    want = MR.quality_ref(p, t, w, 1.0, (0.5, 0.5), 2.0)
    for f in M.Quality.FIELDS:
        got, ref = getattr(q, f), want[f]
        assert got.dtype == np.float64 and got.shape == ref.shape, f
        assert np.abs(got - ref).max() <= 1e-9 * np.abs(ref).max(), (f, np.abs(got - ref).max())
    assert np.array_equal(q.n, want["n"]) and np.array_equal(q.sam_undefined, want["sam_undefined"])
    for b in range(3):                                                       # a stack against a batch-1 truth is its draws, one by one
        one = M.quality(pd[b:b + 1], td, where=wd, affine=(0.5, 0.5), ratio=2)
        for f in M.Quality.FIELDS:
            assert np.array_equal(getattr(one, f)[0], getattr(q, f)[b], equal_nan=True), (f, b)
    no = M.quality(pd, td, ssim=False)
    assert no.ssim is None and no.ssim_all is None and no.ergas is None and (no.n == 96 * 80).all()
