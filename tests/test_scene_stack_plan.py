"""CPU: the host side of scene stacks (eo_diffusion_amd/tiling.py TileStack) and of their sharding (eo_diffusion_amd/dist.py
shard_bounds), against brute-force loops.

A stack is B scenes of one TilePlan; tile i of scene b has the global number g = b * plan.n_tiles + i.  A listed stack names some
global tiles in ascending order; a pixel of scene b is ESTIMATED iff every tile of scene b that covers it is listed."""
import numpy as np
import pytest

from eo_diffusion_amd._lib import EodError
from eo_diffusion_amd.dist import shard_bounds
from eo_diffusion_amd.tiling import TilePlan, TileStack, TileSubset, tile_slots

PLANS = [(40, 57, 16, 4), (200, 264, 64, 16), (128, 192, 64, 0), (150, 217, 64, 8), (300, 257, 256, 16)]


def brute_estimated(plan, B, listed):
    """pixel by pixel: covered by a tile of its scene, and every covering tile of its scene is listed"""
    listed = set(int(g) for g in listed)
    est = np.zeros((B, plan.H, plan.W), dtype=bool)
    for b in range(B):
        cover = [[[] for _ in range(plan.W)] for _ in range(plan.H)]
        for i, (y0, x0) in enumerate(plan.origins()):
            for y in range(y0, y0 + plan.tile):
                for x in range(x0, x0 + plan.tile):
                    cover[y][x].append(b * plan.n_tiles + i)
        for y in range(plan.H):
            for x in range(plan.W):
                est[b, y, x] = len(cover[y][x]) > 0 and all(g in listed for g in cover[y][x])
    return est


def ragged(plan, B, seed):
    """global numbers with: scene 0 some tiles, scene 1 none, scene 2 all, the others a random pick (B >= 3)"""
    rng = np.random.default_rng(seed)
    nt = plan.n_tiles
    out = sorted(rng.choice(nt, size=max(1, nt // 3), replace=False).tolist())
    out += [2 * nt + i for i in range(nt)]
    for b in range(3, B):
        out += [b * nt + i for i in sorted(rng.choice(nt, size=int(rng.integers(1, nt + 1)), replace=False).tolist())]
    return out


@pytest.mark.parametrize("H,W,tile,overlap", PLANS)
def test_a_full_stack_lists_every_tile_of_every_scene(H, W, tile, overlap):
    plan = TilePlan(H, W, tile, overlap)
    for B in (1, 2, 5):
        st = TileStack(plan, B)
        assert (st.n_scenes, st.n_tiles, st.listed) == (B, B * plan.n_tiles, False)
        assert (st.H, st.W, st.tile, st.overlap) == (H, W, tile, overlap)
        assert st.index.dtype == np.int32 and st.index.tolist() == list(range(B * plan.n_tiles))
        assert st.slot_of.tolist() == list(range(B * plan.n_tiles))
        assert st.estimated().shape == (B, H, W) and bool(st.estimated().all())
        for k in (0, st.n_tiles - 1, st.n_tiles // 2):
            b, i = divmod(k, plan.n_tiles)
            assert st.scene_of(k) == (b, i) and st.origin(k) == plan.origin(i)


@pytest.mark.parametrize("H,W,tile,overlap", PLANS)
def test_a_listed_stack_numbers_its_slots(H, W, tile, overlap):
    plan = TilePlan(H, W, tile, overlap)
    B, nt = 4, plan.n_tiles
    listed = ragged(plan, B, H + W)
    st = TileStack(plan, B, listed)
    assert st.listed and st.n_tiles == len(listed) and st.index.dtype == np.int32 and st.index.tolist() == listed
    assert st.slot_of.shape == (B * nt,) and st.slot_of.dtype == np.int32
    for g in range(B * nt):
        assert st.slot_of[g] == (listed.index(g) if g in listed else -1)
    per = st.per_scene()
    assert len(per) == B and per[1].size == 0 and per[2].tolist() == list(range(nt))
    assert sum(p.size for p in per) == st.n_tiles
    assert [int(b * nt + i) for b, p in enumerate(per) for i in p] == listed
    for k in range(st.n_tiles):
        assert st.scene_of(k) == divmod(listed[k], nt) and st.origin(k) == plan.origin(listed[k] % nt)
    assert TileStack(plan, B, np.asarray(listed, dtype=np.int64)).index.tolist() == listed


@pytest.mark.parametrize("H,W,tile,overlap", [(40, 57, 16, 4), (33, 48, 16, 8), (32, 32, 16, 0), (50, 61, 18, 5)])
def test_estimated_is_per_scene(H, W, tile, overlap):
    plan = TilePlan(H, W, tile, overlap)
    B = 4
    listed = ragged(plan, B, 3 * H + W)
    st = TileStack(plan, B, listed)
    est = st.estimated()
    assert est.shape == (B, H, W) and est.dtype == bool
    assert np.array_equal(est, brute_estimated(plan, B, listed))
    assert not est[1].any() and est[2].all()
    for b, p in enumerate(st.per_scene()):                           # scene by scene it is the TileSubset's rule
        want = TileSubset(plan, p).estimated() if p.size else np.zeros((H, W), dtype=bool)
        assert np.array_equal(est[b], want)


def test_a_stack_of_one_scene_is_the_subset():
    plan = TilePlan(200, 264, 64, 16)
    sub = plan.subset([7, 8, 9, 13, 14, 15])
    st = TileStack(plan, 1, [7, 8, 9, 13, 14, 15])
    assert st.index.tolist() == sub.index.tolist() and st.slot_of.tolist() == sub.slot_of.tolist() and st.n_tiles == sub.n_tiles
    assert np.array_equal(st.estimated()[0], sub.estimated())


def test_refusals():
    plan = TilePlan(40, 57, 16, 4)
    nt = plan.n_tiles
    for bad in ([], [3, 1], [1, 1], [-1, 2], [0, 2 * nt], [[0, 1]], [0.5, 1.5]):
        with pytest.raises(EodError):
            TileStack(plan, 2, bad)
    with pytest.raises(EodError):
        TileStack(plan, 1, [nt])                                      # in range for two scenes, not for one
    assert TileStack(plan, 2, [nt]).scene_of(0) == (1, 0)
    for n in (0, -1, 1.5, None, True):
        with pytest.raises(EodError):
            TileStack(plan, n)
    with pytest.raises(EodError):
        TileStack(plan.subset([0]), 2)
    with pytest.raises(EodError):
        TileStack(plan, 2).active_tiles(np.ones((3, 40, 57), dtype=np.float32))
    with pytest.raises(EodError):
        TileStack(plan, 2).active_tiles(np.ones((40, 57), dtype=np.float32))
    # TilePlan and TileSubset keep their own refusals
    with pytest.raises(EodError):
        plan.subset([])
    with pytest.raises(EodError):
        plan.subset([nt])


def test_tile_slots_on_a_ragged_list():
    plan = TilePlan(40, 57, 16, 4)                                  # 15 tiles per scene
    nt = plan.n_tiles
    listed = [0, 1, 2, 5, 6, 7] + [2 * nt + i for i in range(nt)] + [3 * nt + 14]   # 6 + 0 + 15 + 1 = 22
    st = TileStack(plan, 4, listed)
    assert st.n_tiles == 22
    assert tile_slots(st, 16) == (16, 32) and tile_slots(st, 4) == (4, 24) and tile_slots(st, 1) == (1, 22) and tile_slots(st, 64) == (22, 22)
    assert tile_slots(TileStack(plan, 4), 16) == (16, 64) and tile_slots(TileStack(plan, 3), 16) == (16, 48)
    # one sequence of chunks for the whole stack, not one per scene
    per_scene = sum(-(-p.size // min(16, p.size)) for p in st.per_scene() if p.size)
    assert tile_slots(st, 16)[1] // 16 == 2 < per_scene == 3
    with pytest.raises(EodError):
        tile_slots(st, 0)


def test_active_tiles_of_a_stacked_mask_are_global_numbers():
    plan = TilePlan(40, 57, 16, 4)
    nt = plan.n_tiles
    m = np.ones((4, 1, 40, 57), dtype=np.float32)
    m[0, 0, 14:20, 10:30] = 0.0                                      # tiles 0, 1, 2, 5, 6, 7 of scene 0
    m[2] = 0.0                                                       # every tile of scene 2
    m[3, 0, 39, 56] = np.nan                                         # the last tile of scene 3
    st = TileStack(plan, 4)
    got = st.active_tiles(m)
    assert got.dtype == np.int32
    assert got.tolist() == [0, 1, 2, 5, 6, 7] + [2 * nt + i for i in range(nt)] + [3 * nt + 14]
    for b in range(4):
        assert np.array_equal(got[(got >= b * nt) & (got < (b + 1) * nt)] - b * nt, plan.active_tiles(m[b]))
    listed = TileStack(plan, 4, got)
    hole = (m != 1).any(axis=1)
    assert bool(listed.estimated()[hole].all())                      # every hole pixel is estimated


@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("world", [1, 2, 4, 8])
def test_scene_shards_cover_the_stack_once(B, world):
    seen = []
    sizes = []
    for r in range(world):
        lo, hi = shard_bounds(B, world, r)
        assert 0 <= lo <= hi <= B
        sizes.append(hi - lo)
        seen += list(range(lo, hi))
    assert seen == list(range(B))                                    # in order, each scene exactly once
    assert max(sizes) - min(sizes) <= 1 and sum(1 for n in sizes if n == 0) == max(0, world - B)


def test_scene_arguments_are_checked_on_the_host_for_every_rank():
    """EODiffusion.check_scene_args refuses from the arguments alone (no GPU, nothing launched), and dist.sharded_sampling_scene
    runs it on the GLOBAL arguments before it looks at its shard: a rank with an empty shard refuses with the others"""
    import torch
    from eo_diffusion_amd.diffusion.model import EODiffusion
    from eo_diffusion_amd.dist import sharded_sampling_scene

    class Never(torch.nn.Module):
        def forward(self, x, t, cond=None, y=None):
            raise AssertionError("the network was reached")

    m = EODiffusion(Never(), timesteps=4, image_size=16, in_channels=3, cond_type="sum", device="cpu")
    size, ok = (32, 48), torch.ones(3, 4, 32, 48)
    m.check_scene_args(size, "cuda:0", n_scenes=3, cond=ok, y=torch.tensor([1, 2, 3]), overlap=4, skip_known=True, resample=(2, 2))
    m.check_scene_args(size, "cuda:0", n_scenes=np.int64(3), cond=ok[:1], y=torch.tensor([1]))        # numpy integers, broadcast inputs
    assert m._scene_count("x", np.int64(4)) == 4 and type(m._scene_count("x", np.int32(2))) is int
    for kw in (dict(n_scenes=0), dict(n_scenes=True), dict(n_scenes=1.5), dict(n_scenes=3, cond=ok[:2]), dict(n_scenes=3, cond=ok, y=torch.tensor([1, 2])),
               dict(n_scenes=3, cond=ok, tile_batch=0), dict(n_scenes=3, cond=ok, overlap=9), dict(n_scenes=3, skip_known=True),
               dict(n_scenes=3, cond=ok[:, :3]), dict(n_scenes=3, cond=ok, resample=(2,)), dict(n_scenes=3, cond=ok, x_T=torch.zeros(2, 3, 32, 48)),
               dict(n_scenes=3, cond=ok, rng="numpy")):
        with pytest.raises(EodError):
            m.check_scene_args(size, "cuda:0", **kw)
    with pytest.raises(EodError):
        m.check_scene_args(size, "cpu", n_scenes=3, cond=ok)
    with pytest.raises(EodError):
        m.check_scene_args((8, 48), "cuda:0", n_scenes=3, cond=ok)
    for kw in (dict(cond=ok[:2]), dict(cond=ok, y=torch.tensor([1, 2])), dict(cond=ok, tile_batch=0), dict(skip_known=True)):
        with pytest.raises(EodError):
            sharded_sampling_scene(m, size, 3, device="cuda:0", **kw)


def test_sampling_scene_itself_refuses_before_it_touches_a_device():
    """Every bad-argument case that this file, test_ancestral_host.py and test_threshold_host.py put to check_scene_args, put to
    sampling_scene itself, as one scene and as a stack of three where the case leaves that open.  The model's buffers are on the host and
    there may be no GPU at all: the first thing the device half of the call does is refuse the buffers' device ("call .to(device)
    first"), so a refusal with any OTHER text was made from the arguments alone, before anything was copied or launched."""
    import torch
    from eo_diffusion_amd.diffusion.consistency import Observation, PsfObservation, SpectralObservation, gaussian_psf
    from eo_diffusion_amd.diffusion.model import EODiffusion
    from eo_diffusion_amd.diffusion.threshold import DynamicThreshold

    class Never(torch.nn.Module):
        def forward(self, x, t, cond=None, y=None):
            raise AssertionError("the network was reached")

    def refused(m, size, device="cuda:0", **kw):
        with pytest.raises(EodError) as e:
            m.sampling_scene(size, device=device, progress=False, **kw)
        assert "call .to(device) first" not in str(e.value), (kw, str(e.value))

    T, H, W = 20, 32, 48
    m4, m20 = (EODiffusion(Never(), timesteps=t, image_size=16, in_channels=3, cond_type="sum", device="cpu") for t in (4, T))
    v = lambda *shape: torch.zeros(*shape)
    ok = Observation(v(1, 3, H, W), (1, 2, 4))
    psf = lambda *shape, **kw: PsfObservation(v(*shape), gaussian_psf(4), 4, **kw)
    spec = lambda *shape, **kw: SpectralObservation(v(*shape), [[.2, .5, .3]], **kw)
    for B in (1, 3):
        cond = torch.ones(B, 4, H, W)
        with pytest.raises(EodError, match="call .to\\(device\\) first"):                                   # good arguments get as far as the device half
            m4.sampling_scene((H, W), device="cuda:0", progress=False, n_scenes=B, cond=cond, y=torch.arange(B), overlap=4, skip_known=True,
                              resample=(2, 2))
        # tests/test_scene_stack_plan.py
        for kw in (dict(cond=torch.ones(2, 4, H, W)), dict(cond=cond, y=torch.tensor([1, 2])), dict(cond=cond, tile_batch=0), dict(cond=cond, overlap=9),
                   dict(skip_known=True), dict(cond=cond[:, :3]), dict(cond=cond, resample=(2,)), dict(cond=cond, x_T=torch.zeros(2, 3, H, W)),
                   dict(cond=cond, rng="numpy")):
            refused(m4, (H, W), n_scenes=B, **kw)
        refused(m4, (H, W), device="cpu", n_scenes=B, cond=cond)
        refused(m4, (8, W), n_scenes=B, cond=cond)
        # tests/test_ancestral_host.py (the cases that name n_scenes themselves follow below)
        for kw in (dict(observation=ok, skip_known=True), dict(observation=[ok], skip_known=True),
                   dict(observation=Observation(v(1, 4, H, W), (1, 2, 4, 1))), dict(observation=SpectralObservation(v(1, 1, H, W), [[.5, .5]])),
                   dict(observation=psf(1, 4, H // 4, W // 4)), dict(observation=psf(1, 2, H // 4, W // 4, channels=[1, 3])),
                   dict(observation=Observation(v(2, 3, H, W), (1, 2, 4))), dict(observation=Observation(v(1, 3, H, W), (1, 2, 4), mask=v(2, 1, H, W))),
                   dict(observation=psf(2, 3, H // 4, W // 4)), dict(observation=Observation(v(1, 3, 16, 16), (1, 2, 4))), dict(observation=psf(1, 3, H, W)),
                   dict(observation=Observation(v(1, 3, H, W), (1, 2, 4), weight=[0.5] * (T + 1))),
                   dict(observation=Observation(v(1, 3, H, W), (1, 2, 4), weight=[0.5] * T), resample=(4, 3)),
                   dict(observation=[ok, spec(1, 1, H, W, weight=[0.5] * 51)], resample=(4, 3)),
                   dict(observation=[ok] * 5), dict(observation=[ok, None]), dict(observation="obs"), dict(observation=[])):
            refused(m20, (H, W), "cuda", n_scenes=B, cond=v(1, 4, H, W), **kw)
        # tests/test_threshold_host.py
        for kw in (dict(skip_known=True, threshold=DynamicThreshold(0.9)), dict(threshold=0.9)):
            refused(m4, (24, 24), n_scenes=B, cond=torch.zeros(1, 4, 24, 24), overlap=8, **kw)
    for n in (0, True, 1.5):
        refused(m4, (H, W), n_scenes=n)
    for o in (Observation(v(3, 3, H, W), (1, 2, 4)), spec(3, 1, H, W)):
        refused(m20, (H, W), "cuda", n_scenes=2, cond=v(1, 4, H, W), observation=o)
