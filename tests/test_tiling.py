"""CPU: the tile plan of whole-scene sampling (eo_diffusion_amd/tiling.py) -- coverage, origins, and the fp32 blend weights as a
partition of unity.  Bounds: every weight is ONE rounding to fp32 of a float64 value in (0, 1], i.e. off by at most 2^-25; the
weights of the m tiles covering a coordinate, summed in float64, are therefore within m * 2^-25 (+ float64 noise) of one -- the
test holds them to m * 2^-24."""
import itertools

import numpy as np
import pytest

from eo_diffusion_amd._lib import EodError
from eo_diffusion_amd.tiling import TilePlan, axis_plan, tile_slots

AXES = [(512, 256, 0), (600, 256, 32), (1000, 256, 64), (300, 256, 128), (1000, 64, 32), (257, 256, 16), (777, 64, 24)]
# 2-D plans from pairs of the axes above that share tile and overlap, plus square ones
PLANS_2D = [(512, 512, 256, 0), (600, 600, 256, 32), (257, 257, 256, 16), (1000, 1000, 64, 32), (777, 777, 64, 24),
            (300, 300, 256, 128), (1000, 1000, 256, 64)]


def _cover(origins, tile, L):
    n = np.zeros(L, dtype=np.int64)
    for o in origins:
        n[o:o + tile] += 1
    return n


@pytest.mark.parametrize("L,tile,overlap", AXES)
def test_axis_origins_cover_the_axis(L, tile, overlap):
    o, w = axis_plan(L, tile, overlap)
    assert o.dtype == np.int32 and w.dtype == np.float32 and w.shape == (len(o), tile)
    assert o[0] == 0 and o[-1] == L - tile
    assert (np.diff(o) > 0).all() if len(o) > 1 else True          # non-decreasing (strictly: no tile is repeated)
    stride = tile - overlap
    for i, v in enumerate(o):
        assert v == min(i * stride, L - tile)
    assert len(o) == 1 or o[-2] + tile < L                          # ... "until the axis is covered": no tile beyond that
    cov = _cover(o, tile, L)
    assert cov.min() >= 1, "a coordinate is covered by no tile"
    assert cov.max() <= 3
    if overlap == 0 and L % tile == 0:
        assert len(o) == L // tile and cov.max() == 1               # disjoint tiles


@pytest.mark.parametrize("L,tile,overlap", AXES)
def test_axis_weights_are_an_fp32_partition_of_unity(L, tile, overlap):
    o, w = axis_plan(L, tile, overlap)
    cov = _cover(o, tile, L)
    assert (w > 0).all() and (w <= 1).all()
    total = np.zeros(L, dtype=np.float64)
    for i, v in enumerate(o):
        total[v:v + tile] += w[i].astype(np.float64)
        single = cov[v:v + tile] == 1
        assert (w[i][single] == np.float32(1.0)).all(), "a coordinate covered by one tile must weigh exactly 1.0f"
    err = np.abs(total - 1.0)
    print(f"axis ({L}, {tile}, {overlap}): {len(o)} tiles, max cover {cov.max()}, max |sum w - 1| = {err.max():.3e}")
    assert (err <= cov * 2.0 ** -24).all()


@pytest.mark.parametrize("L,tile,overlap", AXES)
def test_axis_ramps_rise_towards_the_interior(L, tile, overlap):
    """the weights are applied where they should be: across the pixels tile i shares with tile i + 1 the weight of i falls and
    that of i + 1 rises (strictly), a tile's last shared pixel weighs less than its neighbour's there"""
    o, w = axis_plan(L, tile, overlap)
    for i in range(len(o) - 1):
        sh = o[i] + tile - o[i + 1]
        if sh == 0:
            continue
        assert sh >= overlap
        a, b = w[i][tile - sh:].astype(np.float64), w[i + 1][:sh].astype(np.float64)
        if len(o) == 2 or _cover(o, tile, L)[o[i + 1]:o[i] + tile].max() == 2:   # (a third tile in the range bends the ramps)
            assert (np.diff(a) < 0).all() and (np.diff(b) > 0).all()
        assert a[-1] < b[-1] and b[0] < a[0]


@pytest.mark.parametrize("H,W,tile,overlap", PLANS_2D + [(300, 1000, 256, 64), (777, 1000, 64, 24), (257, 600, 256, 16)])
def test_plan_2d(H, W, tile, overlap):
    p = TilePlan(H, W, tile, overlap)
    assert p.n_tiles == p.nty * p.ntx and len(p.origins()) == p.n_tiles
    assert p.origins() == [(int(y), int(x)) for y, x in itertools.product(p.origins_y, p.origins_x)]   # row-major
    cov = p.cover_count()
    assert cov.shape == (H, W) and cov.min() >= 1 and cov.max() <= 9
    total = np.zeros((H, W), dtype=np.float64)
    brute = np.zeros((H, W), dtype=np.int64)
    for i, (y0, x0) in enumerate(p.origins()):
        w2 = p.weight(i)
        assert w2.dtype == np.float32 and w2.shape == (tile, tile) and (w2 > 0).all() and (w2 <= 1).all()
        total[y0:y0 + tile, x0:x0 + tile] += w2.astype(np.float64)
        brute[y0:y0 + tile, x0:x0 + tile] += 1
        assert (w2[cov[y0:y0 + tile, x0:x0 + tile] == 1] == np.float32(1.0)).all()
    assert (brute == cov).all()
    # per axis m_a * 2^-25 relative, one more rounding for the product: (1 + my 2^-25)(1 + mx 2^-25)(1 + 2^-25) - 1 summed over the tiles
    assert (np.abs(total - 1.0) <= (cov + 3) * 2.0 ** -24).all()


def test_tile_slots():
    p = TilePlan(128, 192, 64, 0)
    assert p.n_tiles == 6
    assert tile_slots(p, 16) == (6, 6) and tile_slots(p, 4) == (4, 8) and tile_slots(p, 1) == (1, 6) and tile_slots(p, 6) == (6, 6)
    with pytest.raises(EodError):
        tile_slots(p, 0)


@pytest.mark.parametrize("args", [(255, 512, 256, 0), (512, 100, 256, 0), (512, 512, 256, 129), (512, 512, 256, -1), (512, 512, 0, 0),
                                  (64, 64, 65, 0)])
def test_bad_arguments_raise(args):
    with pytest.raises(EodError):
        TilePlan(*args)


def test_scene_entry_points_exist_and_refuse_the_cpu():
    """the public methods are there and refuse a non-GPU device before anything else happens"""
    import torch
    from eo_diffusion_amd.diffusion.model import EODiffusion
    from eo_diffusion_amd.tiling import blend_tiles, gather_tiles

    class Zero(torch.nn.Module):
        def forward(self, x, t, cond=None, y=None):
            raise AssertionError("the network must not be reached")

    m = EODiffusion(Zero(), timesteps=4, image_size=16, in_channels=3)
    with pytest.raises(EodError):
        m.sampling_scene((32, 32), device="cpu", progress=False)
    p = TilePlan(32, 32, 16, 4)
    with pytest.raises(EodError):
        gather_tiles(torch.zeros(1, 3, 32, 32), p)
    with pytest.raises(EodError):
        blend_tiles(torch.zeros(p.n_tiles, 3, 16, 16), p)
