"""CPU: tests/big_index_ref.py, the host side of tests/test_gpu_big_index.py -- the window scheme, the cuts, the threshold's constructed
multiset against tests/threshold_ref.py, and the band blend against a blend of the whole plane."""
import numpy as np
import pytest
import torch

from eo_diffusion_amd.tiling import TilePlan
from tests import big_index_ref as BR
from tests import threshold_ref as TR

SHAPE_I = 2 ** 31 + 2 ** 16 + 4
CHW_II = 13 * 7424 * 7424


def _inside(spans, e):
    return any(lo <= e < hi for lo, hi in spans)


@pytest.mark.parametrize("numel,units", [(SHAPE_I, ()), (SHAPE_I - 1, ()), (3 * CHW_II, (CHW_II, 7424 * 7424)), (2 ** 24, (4096,)), (1000, (10,))])
def test_windows_hold_every_offset_and_the_boundaries_nearest_them(numel, units):
    w = BR.windows(numel, units)
    assert all(0 <= lo < hi <= numel for lo, hi in w) and all(a[1] < b[0] for a, b in zip(w, w[1:]))
    assert _inside(w, 0) and _inside(w, numel - 1) and _inside(w, min(BR.EDGE, numel) - 1) and _inside(w, max(0, numel - BR.EDGE))
    for o in BR.OFFSETS:
        if o < numel:
            assert _inside(w, o - 1) and _inside(w, o) and _inside(w, max(0, o - BR.HALF)) and _inside(w, min(numel, o + BR.HALF) - 1)
    for u in units:
        for a in BR.anchors(numel):
            b = min(range(0, numel + u, u), key=lambda m: (abs(m - a), -m)) if numel // u < 10 ** 5 else None
            if b is not None and 0 < b < numel:
                assert _inside(w, b - 1) and _inside(w, b), (u, a, b)
    assert sum(hi - lo for lo, hi in w) <= (2 + 2 * (1 + len(units)) * 5) * BR.EDGE       # small: only these travel to the host


def test_shape_ii_has_its_sample_boundary_and_2_to_the_31_in_different_samples():
    w = BR.windows(3 * CHW_II, (CHW_II, 7424 * 7424))
    assert 2 * CHW_II < 2 ** 31 < 3 * CHW_II and CHW_II < 2 ** 30 < 2 * CHW_II           # 2^30 lies in sample 1, 2^31 in sample 2
    assert _inside(w, 2 * CHW_II - 1) and _inside(w, 2 * CHW_II) and _inside(w, CHW_II)


def test_cuts_and_chunks():
    spans = [(5, 25), (30, 31), (39, 61)]
    cut = BR.cut_at(spans, 10)
    assert cut == [(5, 10), (10, 20), (20, 25), (30, 31), (39, 40), (40, 50), (50, 60), (60, 61)]
    for numel, size, unit in [(SHAPE_I, BR.CHUNK, None), (3 * CHW_II, BR.CHUNK, 7424 * 7424), (100, 7, 10), (64, 8, None)]:
        ch = BR.chunks(numel, size, unit)
        assert ch[0][0] == 0 and ch[-1][1] == numel and all(a[1] == b[0] for a, b in zip(ch, ch[1:]))
        assert all(0 < hi - lo <= size for lo, hi in ch)
        assert unit is None or all(lo // unit == (hi - 1) // unit for lo, hi in ch)


def test_row_bands_lie_in_their_plane_and_hold_every_offset():
    B, C, H, W = 3, 13, 7424, 7424
    bands = BR.row_bands(B, C, H, W)
    assert all(0 <= b < B and 0 <= c < C and 0 <= ya < yb <= H and yb - ya == 4 for b, c, ya, yb in bands)
    def held(e):
        p, y = divmod(e // W, H)
        return any((b, c) == divmod(p, C) and ya <= y < yb for b, c, ya, yb in bands)
    numel = B * C * H * W
    assert all(held(e) for e in (0, numel - 1, 2 ** 29 - 1, 2 ** 29, 2 ** 30 - 1, 2 ** 30, 2 ** 31 - 1, 2 ** 31))
    hw = H * W
    assert held(2 * C * hw - 1) and held(2 * C * hw) and held(C * hw) and held((2 ** 31 // hw) * hw - 1) and held((2 ** 31 // hw) * hw)
    assert (B - 1, C - 1, H - 4, H) in bands and (0, 0, 0, 4) in bands and len(bands) < 60
    al = BR.row_bands(3, 13, 7440, 7440, 24, align=24)
    assert all(ya % 24 == 0 and yb - ya == 24 and yb <= 7440 for _, _, ya, yb in al) and (2, 12, 7440 - 24, 7440) in al
    e = 2 ** 31
    assert any((b, c) == divmod(e // 7440 // 7440, 13) and ya <= (e // 7440) % 7440 < yb for b, c, ya, yb in al)


# ------------------------------------------------------------------------------------------------ the multiset
@pytest.mark.parametrize("q", [0.5, 0.9, 0.995, 1.0])
@pytest.mark.parametrize("a,scale", [(5, 1.0), (1048573 | 1, 8.0)])
def test_multiset_order_statistic_is_the_sorted_one(q, a, scale):
    """M = 2^10, R = 65: threshold_ref.threshold_kf on the whole multiset against the closed form, bit for bit -- the scale, the value
    and the output"""
    M, R = 2 ** 10, 65
    n = M * R
    scale = scale * 2.0 ** 12                           # (so that the statistic exceeds 1 and the clamp does something)
    x = BR.multiset_x(np.arange(n), a, M, scale)
    mags, counts = np.unique(np.abs(x), return_counts=True)
    assert mags.size == M and (counts == R).all() and (x[:M] > 0).all() and (x[M:2 * M] < 0).all()
    k, frac = TR.rank(q, n)
    for cap in (np.inf, 1.5):
        out, s, v = TR.threshold_kf(torch.from_numpy(x)[None], k, frac, cap)
        s_cf, v_cf = BR.multiset_scale(k, frac, R, M, scale, cap)
        assert np.float32(v[0]).tobytes() == v_cf.tobytes() and np.float32(s[0]).tobytes() == s_cf.tobytes(), (q, cap, float(v[0]), v_cf)
        assert np.array_equal(out[0].numpy().view(np.uint32), BR.threshold_apply(x, s_cf).view(np.uint32))
    assert BR.multiset_order_stat(0, R, scale) == np.float32(scale * 2.0 ** -22)
    assert BR.multiset_order_stat(n - 1, R, scale) == np.float32(M * scale * 2.0 ** -22)


def test_multiset_is_exact_at_the_sizes_of_the_gpu_test():
    """M = 2^24: i a stays below 2^63 for i < 2^32 and a < 2^24, every magnitude (m + 1) 2^-22 with m < 2^24 is an fp32 number"""
    M, a = 2 ** 24, 11400713
    i = np.array([0, 1, M - 1, M, 65 * M - 1, 65 * M, 2 * 65 * M - 1, 127 * M - 1], np.int64)
    x = BR.multiset_x(i, a, M)
    want = [(((int(v) * a) % M) + 1) / 2.0 ** 22 * (1 if (int(v) // M) % 2 == 0 else -1) for v in i]
    assert x.astype(np.float64).tolist() == want
    assert a % 2 == 1 and (2 ** 32) * a < 2 ** 63


# ------------------------------------------------------------------------------------------------ the band blend
@pytest.mark.parametrize("H,W,tile,overlap", [(300, 257, 64, 16), (145, 152, 64, 24), (128, 128, 64, 0)])
def test_blend_band_is_the_whole_blend(H, W, tile, overlap):
    """every band of 4 rows equals the rows of the whole plane's blend, formed tile by tile as tests/test_gpu_scene.py blend_emulated
    forms it (torch fp32: w = wy * wx, p = w * e, left to right in ascending tile index)"""
    plan = TilePlan(H, W, tile, overlap)
    g = torch.Generator().manual_seed(H + W)
    tiles = torch.randn((plan.n_tiles, tile, tile), generator=g)
    acc = torch.full((H, W), float("nan"))
    seen = torch.zeros((H, W), dtype=torch.bool)
    for i, (y0, x0) in enumerate(plan.origins()):
        p = torch.from_numpy(plan.weight(i)) * tiles[i]
        reg, sn = acc[y0:y0 + tile, x0:x0 + tile], seen[y0:y0 + tile, x0:x0 + tile]
        acc[y0:y0 + tile, x0:x0 + tile] = torch.where(sn, reg + p, p)
        seen[y0:y0 + tile, x0:x0 + tile] = True
    whole = acc.numpy()
    tn = tiles.numpy()
    rows_of = lambda iy, ix, d0, d1: tn[iy * plan.ntx + ix, d0:d1]
    for ya in list(range(0, H - 3, 37)) + [H - 4]:
        band = BR.blend_band(rows_of, plan.origins_y, plan.origins_x, plan.wy, plan.wx, tile, W, ya, ya + 4)
        assert np.array_equal(band.view(np.uint32), whole[ya:ya + 4].view(np.uint32)), ya
    assert BR.tiles_covering(plan.origins_y, tile, 0, 1) == [0] and BR.tiles_covering(plan.origins_y, tile, H - 1, H) == [plan.nty - 1]


def test_philox_window_is_the_range_of_the_whole_draw():
    from tests import sampler_edge_ref as R
    key = dict(seed=(0x1234 << 32) | 0x9abcdef1, sample0=3, step=7, stream_id=1)
    ur, ua = R.philox_uniforms(2, 4000, **key)
    for n in (0, 1):
        wr, wa = BR.philox_uniforms_at(123, 877, key["seed"], key["sample0"] + n, key["step"], key["stream_id"])
        assert np.array_equal(wr[0], ur[n, 123:877]) and np.array_equal(wa[0], ua[n, 123:877])
    a = BR.philox_uniforms_at(2 ** 29 - 2, 2 ** 29 + 2, 5, 0, 0, 0)[0]        # quad 2^29 is element 2^31: not the draw of quad 0
    b = BR.philox_uniforms_at(0, 4, 5, 0, 0, 0)[0]
    assert not np.array_equal(a[0, 2:], b[0, :2])
