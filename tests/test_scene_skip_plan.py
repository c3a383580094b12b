"""CPU: the host side of skip_known (eo_diffusion_amd/tiling.py) -- TilePlan.active_tiles, TilePlan.subset / TileSubset -- against a
brute-force loop over tiles and pixels.

Rule: a pixel is a HOLE when its mask value is anything but exactly 1 in any mask channel (soft values and NaN included); a tile is
ACTIVE iff its window holds a hole pixel; a pixel is ESTIMATED iff every tile covering it is active."""
import numpy as np
import pytest

from eo_diffusion_amd._lib import EodError
from eo_diffusion_amd.tiling import TilePlan, TileSubset

# (H, W, tile, overlap, holes [y0, y1, x0, x1], active tiles, hole / estimated-known / not-estimated px, of the last: partly covered)
CASES = [
    (200, 264, 64, 16, [(70, 100, 100, 150)], [7, 8, 9, 13, 14, 15], (1500, 7716, 43584, 8704)),
    (200, 264, 64, 16, [(70, 100, 100, 150), (190, 200, 0, 5)], [7, 8, 9, 13, 14, 15, 18], (1550, 9586, 41664, 10496)),
    (128, 192, 64, 0, [(10, 30, 100, 150)], [1, 2], (1000, 7192, 16384, 0)),
    (150, 217, 64, 8, [(60, 70, 60, 70)], [0, 1, 4, 5], (100, 9532, 22918, 4768)),
    (40, 57, 16, 4, [(14, 20, 10, 30)], [0, 1, 2, 5, 6, 7], (120, 744, 1416, 256)),
]
# the plan shapes of tests/test_gpu_scene.py (copied: that module needs a GPU)
SQUARE = [(512, 256, 0), (600, 256, 32), (1000, 256, 64), (300, 256, 128), (1000, 64, 32), (257, 256, 16), (777, 64, 24)]
PLANS = [(L, L, t, o) for L, t, o in SQUARE] + [(300, 257, 256, 16), (128, 777, 64, 24), (777, 192, 64, 24), (145, 152, 64, 16)]


def rect_holes(H, W, holes):
    m = np.ones((H, W), dtype=np.float32)
    for y0, y1, x0, x1 in holes:
        m[y0:y1, x0:x1] = 0.0
    return m


def brute_active(plan, mask):
    """tile by tile, pixel by pixel"""
    m = np.asarray(mask).reshape(-1, plan.H, plan.W)
    out = []
    for i, (y0, x0) in enumerate(plan.origins()):
        hit = False
        for c in range(m.shape[0]):
            for v in m[c, y0:y0 + plan.tile, x0:x0 + plan.tile].ravel().tolist():
                if not (v == 1.0):
                    hit = True
                    break
            if hit:
                break
        if hit:
            out.append(i)
    return np.asarray(out, dtype=np.int32)


def brute_estimated(plan, active):
    """per pixel: covered by no inactive tile (every tile of a plan covers something, and every pixel is covered)"""
    listed = set(int(i) for i in active)
    n_cover = np.zeros((plan.H, plan.W), dtype=np.int64)
    n_active = np.zeros((plan.H, plan.W), dtype=np.int64)
    for i, (y0, x0) in enumerate(plan.origins()):
        n_cover[y0:y0 + plan.tile, x0:x0 + plan.tile] += 1
        if i in listed:
            n_active[y0:y0 + plan.tile, x0:x0 + plan.tile] += 1
    assert np.array_equal(n_cover, plan.cover_count())
    return n_active == n_cover, n_active


def random_mask(kind, H, W, seed):
    rng = np.random.default_rng(seed)
    if kind == "binary":
        m = np.ones((H, W), dtype=np.float32)
        for _ in range(int(rng.integers(1, 4))):
            y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
            m[y0:y0 + int(rng.integers(1, max(2, H // 5))), x0:x0 + int(rng.integers(1, max(2, W // 5)))] = 0.0
        return m
    if kind == "soft":
        m = np.ones((H, W), dtype=np.float32)
        for v in (0.5, np.float32(1.0) - np.float32(2.0 ** -24), np.nan, 1.5):
            m[int(rng.integers(0, H)), int(rng.integers(0, W))] = v
        return m
    assert kind == "channels"
    m = np.ones((3, H, W), dtype=np.float32)
    for c in range(3):
        y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
        m[c, y0:y0 + int(rng.integers(1, 9)), x0:x0 + int(rng.integers(1, 9))] = 0.0
    return m


@pytest.mark.parametrize("H,W,tile,overlap,holes,active,counts", CASES)
def test_the_listed_masks_classify_as_listed(H, W, tile, overlap, holes, active, counts):
    plan = TilePlan(H, W, tile, overlap)
    mask = rect_holes(H, W, holes)
    got = plan.active_tiles(mask)
    assert got.dtype == np.int32 and got.tolist() == active
    assert np.array_equal(got, brute_active(plan, mask))
    sub = plan.subset(got)
    assert isinstance(sub, TileSubset) and sub.plan is plan and sub.n_tiles == len(active)
    est = sub.estimated()
    want, n_active = brute_estimated(plan, got)
    assert est.dtype == bool and np.array_equal(est, want)
    hole = mask != 1
    assert bool(est[hole].all())
    figures = (int(hole.sum()), int((est & ~hole).sum()), int((~est).sum()), int((~est & (n_active > 0)).sum()))
    assert figures == counts


@pytest.mark.parametrize("kind", ["binary", "soft", "channels"])
@pytest.mark.parametrize("H,W,tile,overlap", PLANS + [c[:4] for c in CASES[1:]])
def test_active_tiles_and_estimated_vs_brute_force(H, W, tile, overlap, kind):
    plan = TilePlan(H, W, tile, overlap)
    mask = random_mask(kind, H, W, 1000 + H + 7 * W + tile + overlap)
    got = plan.active_tiles(mask)
    assert np.array_equal(got, brute_active(plan, mask))
    assert got.size >= 1 and np.all(np.diff(got) > 0)
    sub = plan.subset(got)
    est = sub.estimated()
    assert np.array_equal(est, brute_estimated(plan, got)[0])
    hole = (np.asarray(mask) != 1).reshape(-1, H, W).any(axis=0)
    assert bool(est[hole].all())                                     # every hole pixel is estimated
    assert np.array_equal(sub.index, got)
    assert np.array_equal(np.flatnonzero(sub.slot_of >= 0), got) and np.array_equal(sub.slot_of[got], np.arange(got.size))
    for k in (0, got.size - 1):
        assert sub.origin(k) == plan.origin(got[k])


def test_nan_and_soft_values_are_holes_and_one_is_not():
    plan = TilePlan(40, 57, 16, 4)
    ones = np.ones((40, 57), dtype=np.float32)
    assert plan.active_tiles(ones).size == 0
    assert plan.active_tiles(np.ones((2, 3, 40, 57))).size == 0
    for v in (np.nan, 0.5, 0.0, -1.0, 2.0, np.float32(1.0) + np.float32(2.0 ** -23)):
        m = ones.copy()
        m[39, 56] = v                                                # the last pixel: the last tile alone
        assert plan.active_tiles(m).tolist() == [plan.n_tiles - 1], v
    m = np.ones((3, 40, 57), dtype=np.float32)
    m[2, 0, 0] = 0.5                                                 # any channel counts
    assert plan.active_tiles(m).tolist() == [0]
    assert plan.active_tiles(np.zeros((40, 57))).tolist() == list(range(plan.n_tiles))


@pytest.mark.parametrize("H,W,tile,overlap", PLANS[:3] + [(40, 57, 16, 4)])
def test_a_subset_of_every_tile_is_estimated_everywhere(H, W, tile, overlap):
    plan = TilePlan(H, W, tile, overlap)
    sub = plan.subset(range(plan.n_tiles))
    assert sub.n_tiles == plan.n_tiles and bool(sub.estimated().all())
    assert np.array_equal(sub.slot_of, np.arange(plan.n_tiles))
    one = plan.subset([plan.n_tiles - 1])
    est = one.estimated()
    y0, x0 = plan.origin(plan.n_tiles - 1)
    assert not bool(est[:y0].any()) and not bool(est[:, :x0].any())  # only pixels of the listed tile can be estimated
    assert bool(est[H - 1, W - 1]) == (plan.cover_count()[H - 1, W - 1] == 1)


def test_bad_lists_are_refused():
    plan = TilePlan(200, 264, 64, 16)
    for bad in ([3, 1], [1, 1], [-1, 2], [0, plan.n_tiles], [], [[1, 2]], [0.5], np.asarray([1.0, 2.0])):
        with pytest.raises(EodError):
            plan.subset(bad)
    with pytest.raises(EodError):
        TileSubset(plan.subset([1, 2]), [1])                         # a subset of a subset is not a thing
    with pytest.raises(EodError):
        plan.active_tiles(np.ones((200, 263)))
    with pytest.raises(EodError):
        plan.active_tiles(np.ones(264))
    assert plan.subset(np.asarray([2, 5], dtype=np.int64)).index.dtype == np.int32
    assert plan.subset((2, 5)).index.tolist() == [2, 5]


def test_tile_slots_counts_the_listed_tiles():
    from eo_diffusion_amd.tiling import tile_slots
    plan = TilePlan(200, 264, 64, 16)
    sub = plan.subset([7, 8, 9, 13, 14, 15])
    assert tile_slots(plan, 16) == (16, 32)
    assert tile_slots(sub, 16) == (6, 6) and tile_slots(sub, 4) == (4, 8) and tile_slots(sub, 1) == (1, 6)
    with pytest.raises(EodError):
        tile_slots(sub, 0)
