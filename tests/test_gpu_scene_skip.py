"""GPU: skip_known -- the UNet runs only on the scene tiles whose window holds a hole pixel of the RePaint mask.
eod_scene_tile_active / eod_scene_gather_list / eod_scene_blend_list / eod_scene_keep_known (csrc/scene.hip), TileSubset
(eo_diffusion_amd/tiling.py), EODiffusion.sampling_scene(skip_known=True) and DDIMSampler.sample_scene(skip_known=True).

The claim is BIT equality, so every comparison is torch.equal: the skipping call equals the full call at every estimated pixel (a
pixel whose covering tiles are all active: every hole pixel and the known pixels around it) and is the known image itself at every
other pixel.  A whole-call test first asserts from the host-side plan that its input leaves a tile inactive, has a hole that lies in
at least two tiles and a non-zero number of pixels in every class it compares."""
import math

import numpy as np
import pytest
import torch

from eo_diffusion_amd import _lib
from eo_diffusion_amd._lib import EodError
from eo_diffusion_amd.diffusion.util import make_resample_schedule
from eo_diffusion_amd.tiling import TilePlan, active_tiles, blend_tiles, gather_padded, gather_tiles, keep_known, tile_slots, tiled_estimate
from tests.gpu_util import DEV
from tests.synth import synth_input, synth_state_dict

pytestmark = pytest.mark.gpu

# (H, W, tile, overlap, holes [y0, y1, x0, x1]) -- classified on the CPU in tests/test_scene_skip_plan.py
CASES = {
    "one_hole": (200, 264, 64, 16, [(70, 100, 100, 150)]),             # 6 of 24 tiles: 7, 8, 9, 13, 14, 15
    "two_holes": (200, 264, 64, 16, [(70, 100, 100, 150), (190, 200, 0, 5)]),  # + 18
    "overlap_0": (128, 192, 64, 0, [(10, 30, 100, 150)]),             # 2 of 6: 1, 2
    "odd_width": (150, 217, 64, 8, [(60, 70, 60, 70)]),               # 4 of 12: 0, 1, 4, 5
    "small": (40, 57, 16, 4, [(14, 20, 10, 30)]),                     # 6 of 15: 0, 1, 2, 5, 6, 7
}
KERNEL_PLANS = [c[:4] for c in CASES.values()] + [(145, 152, 64, 16), (128, 777, 64, 24), (50, 61, 18, 5), (300, 257, 256, 16)]


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def cut(scene, plan):
    s = plan.tile
    return torch.cat([scene[:, :, y0:y0 + s, x0:x0 + s] for y0, x0 in plan.origins()]).contiguous()


def rect_holes(H, W, holes, value=0.0):
    m = np.ones((H, W), dtype=np.float32)
    for y0, y1, x0, x1 in holes:
        m[y0:y1, x0:x1] = value
    return m


def classes(plan, mask_np):
    """(subset, hole, est) with the input conditions of the module docstring asserted; mask_np [H, W] or [..., H, W]"""
    hole = (np.asarray(mask_np) != 1).reshape(-1, plan.H, plan.W).any(axis=0)
    act = plan.active_tiles(mask_np)
    assert 2 <= act.size < plan.n_tiles, "a test that skips nothing (or has its hole in one tile) proves nothing"
    sub = plan.subset(act)
    est = sub.estimated()
    assert hole.sum() > 0 and bool(est[hole].all()) and (est & ~hole).sum() > 0 and (~est).sum() > 0
    if plan.overlap > 0:
        touched = np.zeros_like(est)
        for i in act:
            y0, x0 = plan.origin(i)
            touched[y0:y0 + plan.tile, x0:x0 + plan.tile] = True
        assert (~est & touched).sum() > 0                            # known pixels covered by an active AND an inactive tile
    return sub, hole, est


def assert_skip_equals_full(skip, full, known, est, what=""):
    e = torch.from_numpy(est).to(skip.device)[None, None].expand_as(full)
    assert skip.shape == full.shape and bool(torch.isfinite(skip).all()) and bool(torch.isfinite(full).all())
    n_est = int((skip[e] != full[e]).sum())
    n_known = int((skip[~e] != known.to(skip.device)[~e]).sum())
    print(f"{what}: differing at estimated pixels {n_est} of {int(e.sum())}; differing from the known image elsewhere {n_known} of {int((~e).sum())}")
    assert torch.equal(skip[e], full[e])
    assert torch.equal(skip[~e], known.to(skip.device)[~e])
    assert not torch.equal(full[~e], known.to(skip.device)[~e])     # (the documented difference: the full call denoises the known image)


# ---------------------------------------------------------------------------------------------------- 2. classification kernel
def _masks(H, W, seed):
    """(name, mask [Cm, H, W] or [H, W]) -- binary, soft, NaN, per channel"""
    rng = np.random.default_rng(seed)
    y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
    one = np.ones((H, W), dtype=np.float32)
    out = [("ones", one.copy()), ("zeros", np.zeros((H, W), dtype=np.float32))]
    m = one.copy(); m[y:y + 9, x:x + 13] = 0.0; out.append(("binary", m))
    m = one.copy(); m[y, x] = 0.5; out.append(("soft", m))
    m = one.copy(); m[y, x] = np.nan; out.append(("nan", m))
    m = one.copy(); m[H - 1, W - 1] = np.float32(1.0) - np.float32(2.0 ** -24); out.append(("one ulp below 1, last pixel", m))
    m = one.copy(); m[0, 0] = 2.0; out.append(("above 1, first pixel", m))
    m = np.ones((3, H, W), dtype=np.float32); m[2, y, x] = 0.5; m[0, (y * 7) % H, (x * 3) % W] = np.nan; out.append(("channels", m))
    return out


@pytest.mark.parametrize("H,W,tile,overlap", KERNEL_PLANS)
def test_tile_active_is_the_host_rule(H, W, tile, overlap):
    plan = TilePlan(H, W, tile, overlap)
    for name, m in _masks(H, W, H + W):
        want = plan.active_tiles(m)
        got = active_tiles(torch.from_numpy(m).to(DEV), plan)
        assert got.dtype == np.int32 and np.array_equal(got, want), name
        if m.ndim == 2:                                              # [1, 1, H, W] as the samplers hand it over, and an unaligned view
            assert np.array_equal(active_tiles(torch.from_numpy(m).to(DEV)[None, None], plan), want), name
            base = _nan(H * W + 1)
            base[1:] = torch.from_numpy(m).to(DEV).reshape(-1)
            assert np.array_equal(active_tiles(base[1:].view(H, W), plan), want), name
    for name, (h, w, t, o, holes) in CASES.items():
        if (h, w, t, o) == (H, W, tile, overlap):
            m = rect_holes(H, W, holes)
            assert np.array_equal(active_tiles(torch.from_numpy(m).to(DEV), plan), plan.active_tiles(m)), name


def test_tile_active_writes_every_entry():
    plan = TilePlan(200, 264, 64, 16)
    oy, ox, _, _ = plan.device_tables(DEV)
    m = torch.ones(1, 200, 264, device=DEV)
    m[0, 80, 120] = 0.0
    out = torch.full((plan.n_tiles,), 77, dtype=torch.int32, device=DEV)
    assert _lib.lib().eod_scene_tile_active(m.data_ptr(), out.data_ptr(), 1, 200, 264, 64, oy.data_ptr(), ox.data_ptr(), plan.nty, plan.ntx, 0) == 0
    got = out.cpu().numpy()
    assert set(got.tolist()) == {0, 1} and np.flatnonzero(got).tolist() == plan.active_tiles(m.cpu().numpy()).tolist()


# ---------------------------------------------------------------------------------------------------------- 3. gather of a list
def _subsets(plan, seed):
    rng = np.random.default_rng(seed)
    n = plan.n_tiles
    picks = [[0], [n - 1], list(range(n))]
    if n > 2:
        picks.append(sorted(rng.choice(n, size=max(2, n // 3), replace=False).tolist()))
        picks.append(list(range(1, n, 2)))
    return [plan.subset(p) for p in picks]


@pytest.mark.parametrize("C", [1, 3, 7])
@pytest.mark.parametrize("H,W,tile,overlap", KERNEL_PLANS)
def test_gather_of_a_subset_is_the_listed_rows(H, W, tile, overlap, C):
    plan = TilePlan(H, W, tile, overlap)
    scene = synth_input("skg", (1, C, H, W), 3).to(DEV)
    full = gather_tiles(scene, plan)
    for sub in _subsets(plan, H + C):
        out = _nan(sub.n_tiles, C, tile, tile)                       # exactly n_list tiles: a write behind it leaves the allocation
        got = gather_tiles(scene, sub, out=out)
        assert got.shape == (sub.n_tiles, C, tile, tile)
        assert torch.equal(got, full[torch.from_numpy(sub.index).long().to(DEV)])
    assert torch.equal(gather_tiles(scene[0], sub), got)


def test_gather_of_a_subset_from_an_unaligned_view_into_a_padded_buffer():
    plan = TilePlan(150, 217, 64, 8)                                 # odd width: the last column's origin is odd
    assert any(int(o) % 2 for o in plan.origins_x)
    base = synth_input("sku", (3 * 150 * 217 + 1,), 5).to(DEV)
    scene = base[1:].view(1, 3, 150, 217)
    sub = plan.subset([0, 3, 5, 7, 11])
    chunk, slots = tile_slots(sub, 4)
    assert (chunk, slots) == (4, 8)
    out = _nan(slots, 3, 64, 64)
    got = gather_tiles(scene, sub, out=out)
    assert torch.equal(got, cut(scene, plan)[[0, 3, 5, 7, 11]])
    assert bool(torch.isnan(out[sub.n_tiles:]).all())                # the padding slots are the caller's
    pad = gather_padded(scene, sub, 4)
    assert pad.shape[0] == 8 and torch.equal(pad[:5], got) and all(torch.equal(pad[k], got[4]) for k in (5, 6, 7))


# ----------------------------------------------------------------------------------------------------------- 4. blend of a list
@pytest.mark.parametrize("scale", [1.0, 1e-30, 1e30])
@pytest.mark.parametrize("C", [1, 3, 7, 13])
@pytest.mark.parametrize("H,W,tile,overlap", KERNEL_PLANS)
def test_blend_of_a_subset_is_the_full_blend_where_estimated_and_zero_elsewhere(H, W, tile, overlap, C, scale):
    plan = TilePlan(H, W, tile, overlap)
    if C > 3 and H * W > 300 * 300:
        C = 2
    tiles = (synth_input("ske", (plan.n_tiles, C, tile, tile), 11) * scale).to(DEV)
    full = blend_tiles(tiles, plan, out=_nan(1, C, H, W))
    for sub in _subsets(plan, W + C):
        compact = tiles[torch.from_numpy(sub.index).long().to(DEV)].clone()   # exactly n_list tiles: a wrong slot reads outside it
        assert compact.shape[0] == sub.n_tiles
        out = blend_tiles(compact, sub, out=_nan(1, C, H, W))
        est = torch.from_numpy(sub.estimated()).to(DEV)[None, None].expand_as(out)
        assert torch.equal(out[est].view(torch.int32), full[est].view(torch.int32))
        assert bool((out[~est].view(torch.int32) == 0).all())        # exactly +0.0, every element written (none is NaN)
        if sub.n_tiles == plan.n_tiles:
            assert bool(est.all())


def test_blend_of_a_subset_with_unaligned_buffers():
    plan = TilePlan(200, 264, 64, 16)
    sub = plan.subset([7, 8, 9, 13, 14, 15])
    tiles = synth_input("skb", (plan.n_tiles, 3, 64, 64), 12).to(DEV)
    full = blend_tiles(tiles, plan)
    base = _nan(6 * 3 * 64 * 64 + 1)
    base[1:] = tiles[[7, 8, 9, 13, 14, 15]].reshape(-1)
    out = blend_tiles(base[1:].view(6, 3, 64, 64), sub)             # (made contiguous, not aligned: torch keeps the storage offset)
    est = torch.from_numpy(sub.estimated()).to(DEV)[None, None].expand_as(out)
    assert torch.equal(out[est], full[est]) and bool((out[~est] == 0).all())


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("H,W,tile,overlap", KERNEL_PLANS)
def test_keep_known_vs_torch_where(H, W, tile, overlap, C):
    plan = TilePlan(H, W, tile, overlap)
    x = synth_input("skx", (1, C, H, W), 13).to(DEV)
    known = synth_input("skk", (1, C, H, W), 14).to(DEV)
    for sub in _subsets(plan, 2 * H + C):
        est = torch.from_numpy(sub.estimated()).to(DEV)[None, None]
        got = keep_known(x, known, sub, out=_nan(1, C, H, W))
        assert torch.equal(got.view(torch.int32), torch.where(est, x, known).view(torch.int32))
    base = _nan(C * H * W + 1)
    base[1:] = x.reshape(-1)
    assert torch.equal(keep_known(base[1:].view(1, C, H, W), known[0], sub), torch.where(est, x, known))


def test_tiled_estimate_of_a_subset_numbers_slots():
    plan = TilePlan(200, 264, 64, 16)
    sub = plan.subset([7, 8, 9, 13, 14, 15])
    scene = synth_input("sks", (1, 3, 200, 264), 15).to(DEV)
    seen = []

    def fn(x, lo):
        seen.append((lo, x.clone()))
        return x * 2.0

    got = tiled_estimate(scene, sub, 4, fn)
    assert [lo for lo, _ in seen] == [0, 4]
    want = cut(scene, plan)[[7, 8, 9, 13, 14, 15, 15, 15]]
    assert torch.equal(torch.cat([x for _, x in seen]), want)
    full = tiled_estimate(scene, plan, 4, lambda x, lo: x * 2.0)
    est = torch.from_numpy(sub.estimated()).to(DEV)[None, None].expand_as(got)
    assert torch.equal(got[est], full[est]) and bool((got[~est] == 0).all())


# -------------------------------------------------------------------------------------------- models shared by the sampler tests
_UNETS = {}


def _unet(prec, attn, s=64, in_ch=3, num_classes=None):
    from eo_diffusion_amd.backbones.unet_openai import UNetModel, unet_param_shapes
    key = (prec, attn, s, in_ch, num_classes)
    if key not in _UNETS:
        cfg = dict(image_size=s, in_channels=in_ch, model_channels=32, out_channels=3, num_res_blocks=1,
                   attention_resolutions=[4] if attn else [], channel_mult=[1, 2, 2] if attn else [1, 2], num_heads=4 if attn else 1)
        if num_classes:
            cfg["num_classes"] = num_classes
        u = UNetModel(**cfg).set_precision(prec)
        u.load_state_dict(synth_state_dict(unet_param_shapes(**cfg), 7))
        _UNETS[key] = u.to(DEV).eval()
    return _UNETS[key]


def _diffusion(prec, attn=False, T=8, cond_type=None, s=64, in_ch=3, num_classes=None):
    from eo_diffusion_amd.diffusion.model import EODiffusion
    return EODiffusion(_unet(prec, attn, s, in_ch, num_classes), timesteps=T, image_size=s, in_channels=3, cond_type=cond_type,
                       device=DEV).to(DEV).eval()


class Calls:
    """forward hook on the UNet: the batch size of every call"""

    def __init__(self, module):
        self.batches = []
        self.handle = module.register_forward_hook(lambda mod, args, out: self.batches.append(int(args[0].shape[0])))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.handle.remove()


def _case(name, seed, value=0.0):
    H, W, tile, overlap, holes = CASES[name]
    plan = TilePlan(H, W, tile, overlap)
    mask = rect_holes(H, W, holes, value)
    gt = synth_input("skgt", (1, 3, H, W), seed, uniform=True) * 2 - 1
    return plan, mask, gt


def _ddpm_pair(m, plan, mask, gt, clip, seed, resample=None, tile_batch=16, **kw):
    """(skip, full) of sampling_scene with the same injected draws"""
    T = m.timesteps
    H, W = plan.H, plan.W
    n_eval, n_jump = T, 0
    if resample is not None:
        visits, jumps = make_resample_schedule(T, *resample)
        n_eval, n_jump = len(visits), len(jumps)
        kw["jump_noises"] = synth_input("skj", (n_jump, 1, 3, H, W), seed)
        kw["resample"] = resample
    cond = torch.cat([gt, torch.from_numpy(mask)[None, None]], 1)
    args = dict(cond=cond, overlap=plan.overlap, x_T=synth_input("skxT", (1, 3, H, W), seed),
                noises=synth_input("skn", (n_eval, 1, 3, H, W), seed), progress=False, **kw)
    full = m.sampling_scene((H, W), clip, DEV, tile_batch=16, **args)
    skip = m.sampling_scene((H, W), clip, DEV, tile_batch=tile_batch, skip_known=True, **args)
    return skip, full


# ------------------------------------------------------------------------------------------------------- 5. whole calls, DDPM
@pytest.mark.parametrize("attn", [False, True])
@pytest.mark.parametrize("prec", ["fp32x3", "fp16"])
@pytest.mark.parametrize("clip", [True, False])
def test_ddpm_skip_known_equals_the_full_call(clip, prec, attn):
    plan, mask, gt = _case("one_hole", 41)
    _, _, est = classes(plan, mask)
    m = _diffusion(prec, attn, 8, "sum")
    skip, full = _ddpm_pair(m, plan, mask, gt, clip, 41)
    assert_skip_equals_full(skip, full, gt, est, f"DDPM clip={clip} {prec} attn={attn}")


@pytest.mark.parametrize("name", ["two_holes", "overlap_0", "odd_width"])
def test_ddpm_skip_known_on_other_plans(name):
    plan, mask, gt = _case(name, 42)
    _, _, est = classes(plan, mask)
    m = _diffusion("fp32x3", False, 8, "sum")
    skip, full = _ddpm_pair(m, plan, mask, gt, True, 42)
    assert_skip_equals_full(skip, full, gt, est, name)


def test_ddpm_skip_known_with_a_soft_hole():
    """mask 0.5 in the hole: a hole pixel all the same (anything but exactly 1), mixed half and half on every visit"""
    plan, mask, gt = _case("one_hole", 43, value=0.5)
    _, _, est = classes(plan, mask)
    m = _diffusion("fp32x3", False, 8, "sum")
    skip, full = _ddpm_pair(m, plan, mask, gt, True, 43)
    assert_skip_equals_full(skip, full, gt, est, "soft hole")


@pytest.mark.parametrize("prec", ["fp32x3", "fp16"])
def test_ddpm_skip_known_with_resampling(prec):
    plan, mask, gt = _case("one_hole", 44)
    _, _, est = classes(plan, mask)
    m = _diffusion(prec, False, 8, "sum")
    assert len(make_resample_schedule(8, 2, 2)[1]) > 0
    skip, full = _ddpm_pair(m, plan, mask, gt, True, 44, resample=(2, 2))
    assert_skip_equals_full(skip, full, gt, est, f"resample=(2, 2) {prec}")
    plain, _ = _ddpm_pair(m, plan, mask, gt, True, 44)
    assert not torch.equal(plain, skip)


def test_ddpm_skip_known_for_every_tile_batch():
    plan, mask, gt = _case("one_hole", 45)
    _, _, est = classes(plan, mask)
    m = _diffusion("fp32x3", True, 8, "sum")
    got = {}
    for tb in (1, 4, 16):
        got[tb], full = _ddpm_pair(m, plan, mask, gt, True, 45, tile_batch=tb)
        assert_skip_equals_full(got[tb], full, gt, est, f"tile_batch {tb}")
    assert torch.equal(got[1], got[16]) and torch.equal(got[4], got[16])


@pytest.mark.parametrize("resample", [None, (2, 2)])
def test_ddpm_skip_known_with_philox_and_torch_draws(resample):
    """no injected draws: the draws are scene-level and keyed as in the full call, which is what makes the two comparable"""
    plan, mask, gt = _case("two_holes", 46)
    _, _, est = classes(plan, mask)
    m = _diffusion("fp32x3", False, 8, "sum")
    cond = torch.cat([gt, torch.from_numpy(mask)[None, None]], 1)
    run = lambda **kw: m.sampling_scene((plan.H, plan.W), True, DEV, cond=cond, overlap=plan.overlap, progress=False, resample=resample, **kw)
    full = run(rng="philox", seed=5)
    skip = run(rng="philox", seed=5, skip_known=True, tile_batch=4)
    assert_skip_equals_full(skip, full, gt, est, f"philox resample={resample}")
    assert not torch.equal(run(rng="philox", seed=6, skip_known=True), skip)
    torch.manual_seed(3)
    full = run(rng="torch")
    torch.manual_seed(3)
    skip = run(rng="torch", skip_known=True)
    assert_skip_equals_full(skip, full, gt, est, f"torch resample={resample}")


def test_ddpm_skip_known_passes_the_label_on():
    s, T = 16, 6
    plan, mask, gt = _case("small", 47)
    _, _, est = classes(plan, mask)
    from eo_diffusion_amd.diffusion.model import EODiffusion
    m = EODiffusion(_unet("fp32x3", True, s, 3, 5), timesteps=T, image_size=s, in_channels=3, cond_type="sum", device=DEV).to(DEV).eval()
    y = torch.tensor([3])
    skip, full = _ddpm_pair(m, plan, mask, gt, True, 47, y=y, tile_batch=4)
    assert_skip_equals_full(skip, full, gt, est, "label")
    other, _ = _ddpm_pair(m, plan, mask, gt, True, 47, y=torch.tensor([1]), tile_batch=4)
    assert not torch.equal(other, skip)


# ------------------------------------------------------------------------------------------------------- 5. whole calls, DDIM
def _ddim_pair(smp, S, plan, mask, x0, eta, seed, resample=None, tile_batch=16, **kw):
    H, W = plan.H, plan.W
    n_eval = S
    if resample is not None:
        visits, jumps = make_resample_schedule(S, *resample)
        n_eval = len(visits)
        kw["jump_noises"] = synth_input("skdj", (len(jumps), 1, 3, H, W), seed)
        kw["resample"] = resample
    args = dict(overlap=plan.overlap, mask=mask.to(DEV), x0=x0.to(DEV), eta=eta, x_T=synth_input("skdx", (1, 3, H, W), seed),
                step_noises=synth_input("skds", (n_eval, 1, 3, H, W), seed), mix_noises=synth_input("skdm", (n_eval, 1, 3, H, W), seed),
                progress=False, **kw)
    full, inter_f = smp.sample_scene(S, (H, W), tile_batch=16, **args)
    skip, inter_s = smp.sample_scene(S, (H, W), tile_batch=tile_batch, skip_known=True, **args)
    assert len(inter_f["x_inter"]) == len(inter_s["x_inter"])
    return skip, full, inter_s, inter_f


@pytest.mark.parametrize("prec", ["fp32x3", "fp16"])
@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_ddim_skip_known_equals_the_full_call(eta, prec):
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    plan, mask, x0 = _case("one_hole", 51)
    _, _, est = classes(plan, mask)
    smp = DDIMSampler(_diffusion(prec, False, 20))
    skip, full, inter_s, inter_f = _ddim_pair(smp, 5, plan, torch.from_numpy(mask)[None, None], x0, eta, 51, tile_batch=4)
    assert_skip_equals_full(skip, full, x0, est, f"DDIM eta={eta} {prec}")
    e = torch.from_numpy(est).to(DEV)[None, None].expand_as(full)      # the raw states: meaningful at estimated pixels only
    for a, b in zip(inter_s["pred_x0"], inter_f["pred_x0"]):
        assert torch.equal(a[e], b[e])
    assert torch.equal(inter_s["x_inter"][-1][e], skip[e])


def test_ddim_skip_known_with_a_mask_per_channel():
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    H, W, tile, overlap, _ = CASES["one_hole"]
    plan = TilePlan(H, W, tile, overlap)
    mask = np.ones((3, H, W), dtype=np.float32)
    mask[0, 70:100, 100:150] = 0.0
    mask[1, 75:95, 90:120] = 0.0                                     # a hole in one channel is a hole
    mask[2, 80:85, 140:155] = 0.5
    _, hole, est = classes(plan, mask)
    assert hole.sum() > (mask[0] != 1).sum()
    x0 = synth_input("skgt", (1, 3, H, W), 52, uniform=True) * 2 - 1
    smp = DDIMSampler(_diffusion("fp32x3", True, 20))
    skip, full, _, _ = _ddim_pair(smp, 4, plan, torch.from_numpy(mask)[None], x0, 1.0, 52)
    assert_skip_equals_full(skip, full, x0, est, "per-channel mask")


def test_ddim_skip_known_with_resampling():
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    plan, mask, x0 = _case("odd_width", 53)
    _, _, est = classes(plan, mask)
    smp = DDIMSampler(_diffusion("fp32x3", False, 20))
    skip, full, _, _ = _ddim_pair(smp, 5, plan, torch.from_numpy(mask)[None, None], x0, 0.5, 53, resample=(2, 2), tile_batch=3)
    assert_skip_equals_full(skip, full, x0, est, "DDIM resample=(2, 2)")


@pytest.mark.parametrize("scale", [1.0, 2.5])
def test_ddim_skip_known_with_concat_conditioning_and_guidance(scale):
    """the conditioning is cut for the active tiles only, and guidance runs per chunk on the doubled batch"""
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    plan, mask, x0 = _case("small", 54)
    _, _, est = classes(plan, mask)
    H, W = plan.H, plan.W
    smp = DDIMSampler(_diffusion("fp32x3", True, 20, None, s=16, in_ch=7))
    c = synth_input("skc", (1, 4, H, W), 54, uniform=True)
    kw = dict(conditioning=c, unconditional_guidance_scale=scale, unconditional_conditioning=torch.zeros_like(c))
    with Calls(smp.model.model) as calls:
        skip, full, _, _ = _ddim_pair(smp, 4, plan, torch.from_numpy(mask)[None, None], x0, 0.5, 54, tile_batch=4, **kw)
    assert_skip_equals_full(skip, full, x0, est, f"guidance {scale}")
    per = 8 if scale != 1.0 else 4                                   # the doubled batch
    assert calls.batches == [15 * (2 if scale != 1.0 else 1)] * 4 + [per] * (2 * 4)
    other, _, _, _ = _ddim_pair(smp, 4, plan, torch.from_numpy(mask)[None, None], x0, 0.5, 54, tile_batch=4,
                                conditioning=c.flip(3), unconditional_guidance_scale=scale, unconditional_conditioning=torch.zeros_like(c))
    assert not torch.equal(other, skip)


# ------------------------------------------------------------------------------------------------- 6. the work is skipped
@pytest.mark.parametrize("resample", [None, (2, 2)])
@pytest.mark.parametrize("tile_batch", [1, 4, 16])
def test_the_unet_sees_ceil_n_active_over_chunk_calls_per_step(tile_batch, resample):
    plan, mask, gt = _case("one_hole", 61)
    sub, _, _ = classes(plan, mask)
    m = _diffusion("fp32x3", False, 8, "sum")
    n_eval = 8 if resample is None else len(make_resample_schedule(8, *resample)[0])
    cond = torch.cat([gt, torch.from_numpy(mask)[None, None]], 1)
    with Calls(m.model) as calls:
        m.sampling_scene((plan.H, plan.W), True, DEV, cond=cond, overlap=plan.overlap, tile_batch=tile_batch, skip_known=True,
                         resample=resample, progress=False)
    chunk = min(tile_batch, sub.n_tiles)
    assert sub.n_tiles == 6 and calls.batches == [chunk] * (n_eval * math.ceil(sub.n_tiles / chunk))
    with Calls(m.model) as calls:
        m.sampling_scene((plan.H, plan.W), True, DEV, cond=cond, overlap=plan.overlap, tile_batch=tile_batch, resample=resample, progress=False)
    chunk = min(tile_batch, plan.n_tiles)
    assert calls.batches == [chunk] * (n_eval * math.ceil(plan.n_tiles / chunk))


class Echo(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.seen = []

    def forward(self, x, t, cond=None, y=None):
        self.seen.append((x.clone(), t.clone()))
        return torch.zeros_like(x)


@pytest.mark.parametrize("tile_batch", [16, 4])
def test_the_unet_is_given_the_active_windows_in_ascending_order(tile_batch):
    from eo_diffusion_amd.diffusion.model import EODiffusion
    plan, mask, gt = _case("small", 62)
    sub, _, _ = classes(plan, mask)
    assert sub.index.tolist() == [0, 1, 2, 5, 6, 7]
    T, H, W = 4, plan.H, plan.W
    m = EODiffusion(Echo(), timesteps=T, image_size=plan.tile, in_channels=3, cond_type="sum", device=DEV).to(DEV)
    x_T, noises = synth_input("ekx", (1, 3, H, W), 62), synth_input("ekn", (T, 1, 3, H, W), 62)
    mk = torch.from_numpy(mask)[None, None]
    out = m.sampling_scene((H, W), True, DEV, cond=torch.cat([gt, mk], 1), x_T=x_T, noises=noises, overlap=plan.overlap,
                           tile_batch=tile_batch, skip_known=True, progress=False)
    chunk, slots = tile_slots(sub, tile_batch)
    per_step = slots // chunk
    assert len(m.model.seen) == T * per_step and all(x.shape[0] == chunk for x, _ in m.model.seen)
    # the first step's input: the mix of x_T at t = T - 1, cut at the listed tiles (padding: copies of the last listed tile)
    t1 = torch.full((1,), T - 1, dtype=torch.int64, device=DEV)
    x_in = m._repaint_mix(x_T.to(DEV), gt.to(DEV), mk.to(DEV), t1, noises[0].to(DEV))
    order = sub.index.tolist() + [int(sub.index[-1])] * (slots - sub.n_tiles)
    assert torch.equal(torch.cat([x for x, _ in m.model.seen[:per_step]]), cut(x_in, plan)[order])
    assert all(bool((t == T - 1).all()) for _, t in m.model.seen[:per_step]) and bool((m.model.seen[-1][1] == 0).all())
    est = torch.from_numpy(sub.estimated()).to(DEV)[None, None].expand_as(out)
    assert torch.equal(out[~est], gt.to(DEV)[~est])


# ------------------------------------------------------------------------------------------------------------------ 7. edges
def test_a_mask_of_ones_returns_the_known_image_without_a_unet_call():
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    plan, _, gt = _case("one_hole", 71)
    m = _diffusion("fp32x3", False, 8, "sum")
    cond = torch.cat([gt, torch.ones(1, 1, plan.H, plan.W)], 1)
    with Calls(m.model) as calls:
        out = m.sampling_scene((plan.H, plan.W), True, DEV, cond=cond, overlap=plan.overlap, skip_known=True, progress=False)
        smp = DDIMSampler(m)
        img, inter = smp.sample_scene(4, (plan.H, plan.W), overlap=plan.overlap, mask=torch.ones(plan.H, plan.W), x0=gt, skip_known=True,
                                      progress=False)
    assert calls.batches == []
    assert torch.equal(out, gt.to(DEV)) and torch.equal(img, gt.to(DEV)) and torch.equal(inter["x_inter"][-1], img)


def test_a_mask_of_zeros_is_the_full_call_everywhere():
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    plan, _, gt = _case("overlap_0", 72)
    m = _diffusion("fp32x3", False, 8, "sum")
    cond = torch.cat([gt, torch.zeros(1, 1, plan.H, plan.W)], 1)
    run = lambda **kw: m.sampling_scene((plan.H, plan.W), True, DEV, cond=cond, seed=3, progress=False, **kw)
    assert torch.equal(run(skip_known=True), run())
    smp = DDIMSampler(_diffusion("fp32x3", False, 20))
    kw = dict(mask=torch.zeros(1, 1, plan.H, plan.W), x0=gt, x_T=synth_input("zx", (1, 3, plan.H, plan.W), 72), progress=False)
    assert torch.equal(smp.sample_scene(3, (plan.H, plan.W), skip_known=True, **kw)[0], smp.sample_scene(3, (plan.H, plan.W), **kw)[0])


def test_skip_known_without_a_known_region_is_refused_before_any_launch():
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    plan, mask, gt = _case("small", 73)
    H, W = plan.H, plan.W
    plain = _diffusion("fp32x3", True, 20, None, s=16, in_ch=7)      # channel-concatenated cond: no known region
    summed = _diffusion("fp32x3", True, 20, "sum", s=16)
    with Calls(plain.model) as calls, Calls(summed.model) as calls2:
        with pytest.raises(EodError):
            plain.sampling_scene((H, W), True, DEV, cond=torch.zeros(1, 4, H, W), overlap=4, skip_known=True, progress=False)
        with pytest.raises(EodError):
            summed.sampling_scene((H, W), True, DEV, overlap=4, skip_known=True, progress=False)
        with pytest.raises(EodError):
            DDIMSampler(summed).sample_scene(4, (H, W), overlap=4, skip_known=True, progress=False)
        with pytest.raises(EodError):
            DDIMSampler(plain).sample_scene(4, (H, W), overlap=4, conditioning=torch.zeros(1, 4, H, W), skip_known=True, progress=False)
    assert calls.batches == [] and calls2.batches == []
    with pytest.raises(TypeError):                                   # keyword-only
        summed.sampling_scene((H, W), True, DEV, None, None, True)


def test_refusals_of_the_subset_entry_points():
    plan = TilePlan(32, 48, 16, 4)
    sub = plan.subset([1, 4])
    with pytest.raises(EodError):
        gather_tiles(torch.zeros(1, 3, 32, 32, device=DEV), sub)
    with pytest.raises(EodError):
        blend_tiles(torch.zeros(1, 3, 16, 16, device=DEV), sub)      # one tile, two listed
    with pytest.raises(EodError):
        keep_known(torch.zeros(1, 3, 32, 48, device=DEV), torch.zeros(1, 3, 32, 48, device=DEV), plan)
    with pytest.raises(EodError):
        keep_known(torch.zeros(1, 3, 32, 48, device=DEV), torch.zeros(1, 1, 32, 48, device=DEV), sub)
    with pytest.raises(EodError):
        active_tiles(torch.ones(32, 47, device=DEV), plan)
    with pytest.raises(EodError):
        active_tiles(torch.ones(32, 48, device=DEV), sub)
    L = _lib.lib()
    oy, ox, wy, wx = plan.device_tables(DEV)
    index, slot_of = sub.device_tables(DEV)
    t = torch.zeros(2, 3, 16, 16, device=DEV)
    sc = torch.zeros(1, 3, 32, 48, device=DEV)
    a = torch.zeros(plan.n_tiles, dtype=torch.int32, device=DEV)
    p = lambda x: x.data_ptr()
    assert L.eod_scene_tile_active(p(sc), p(a), 0, 32, 48, 16, p(oy), p(ox), plan.nty, plan.ntx, 0) == -1
    assert L.eod_scene_tile_active(p(sc), 0, 1, 32, 48, 16, p(oy), p(ox), plan.nty, plan.ntx, 0) == -1
    assert L.eod_scene_gather_list(p(sc), p(t), 3, 32, 48, 16, p(oy), p(ox), plan.nty, plan.ntx, p(index), 0, 0) == -1
    assert L.eod_scene_gather_list(p(sc), p(t), 3, 32, 48, 16, p(oy), p(ox), plan.nty, plan.ntx, p(index), plan.n_tiles + 1, 0) == -1
    assert L.eod_scene_gather_list(p(sc), p(t), 3, 32, 48, 16, p(oy), p(ox), plan.nty, plan.ntx, 0, 2, 0) == -1
    assert L.eod_scene_blend_list(p(t), p(sc), p(wy), p(wx), p(oy), p(ox), p(slot_of), 0, 3, 32, 48, 16, plan.nty, plan.ntx, 0) == -1
    assert L.eod_scene_blend_list(p(t), p(sc), p(wy), p(wx), p(oy), p(ox), 0, 2, 3, 32, 48, 16, plan.nty, plan.ntx, 0) == -1
    assert L.eod_scene_keep_known(p(sc), p(sc), p(slot_of), 2, p(oy), p(ox), 3, 32, 8, 16, plan.nty, plan.ntx, p(sc), 0) == -1
    assert L.eod_scene_keep_known(p(sc), p(sc), p(slot_of), 0, p(oy), p(ox), 3, 32, 48, 16, plan.nty, plan.ntx, p(sc), 0) == -1


def test_tables_are_not_trusted_with_an_address():
    """a slot number outside the compact buffer counts as absent (0.0 written, nothing read); an index outside the plan gives a NaN tile"""
    plan = TilePlan(32, 48, 16, 4)
    sub = plan.subset([1, 4])
    L = _lib.lib()
    oy, ox, wy, wx = plan.device_tables(DEV)
    p = lambda x: x.data_ptr()
    t = torch.ones(2, 3, 16, 16, device=DEV)
    sc = _nan(1, 3, 32, 48)
    wild = torch.from_numpy(np.where(sub.slot_of >= 0, sub.slot_of + 2, -1).astype(np.int32)).to(DEV)   # slots 2, 3 of a 2-tile buffer
    assert L.eod_scene_blend_list(p(t), p(sc), p(wy), p(wx), p(oy), p(ox), p(wild), 2, 3, 32, 48, 16, plan.nty, plan.ntx, 0) == 0
    assert bool((sc == 0).all())
    bad = torch.tensor([1, plan.n_tiles], dtype=torch.int32, device=DEV)
    src = torch.ones(1, 3, 32, 48, device=DEV)
    assert L.eod_scene_gather_list(p(src), p(t), 3, 32, 48, 16, p(oy), p(ox), plan.nty, plan.ntx, p(bad), 2, 0) == 0
    assert bool((t[0] == 1).all()) and bool(torch.isnan(t[1]).all())


@pytest.mark.parametrize("H,W,tile,overlap", [(40, 57, 16, 4), (32, 48, 16, 0)])
def test_the_single_scene_c_entry_points_have_the_bits_of_the_python_layer(H, W, tile, overlap):
    """The Python layer calls only the eod_scene_stack_* entry points; the six single-scene ones remain for C callers
    (INTEGRATION.md).  Each of them, called directly, against the Python layer on the same inputs, bit for bit.  (40, 57): 3 x 5 tiles,
    an odd width and both last tiles shifted inwards, so the scalar path; (32, 48), overlap 0: 2 x 3 tiles on the 16-byte path.  The
    subset is tiles 1, 4, 7 as far as the plan has them (six tiles: 1, 4)."""
    from eo_diffusion_amd.engine import current_stream_ptr
    plan, C = TilePlan(H, W, tile, overlap), 3
    assert (plan.nty, plan.ntx) == ((3, 5) if W == 57 else (2, 3))
    sub = plan.subset([i for i in (1, 4, 7) if i < plan.n_tiles])
    nt, n = plan.n_tiles, sub.n_tiles
    L, st, p = _lib.lib(), current_stream_ptr(torch.device(DEV)), lambda x: x.data_ptr()
    oy, ox, wy, wx = plan.device_tables(DEV)
    index, slot_of = sub.device_tables(DEV)
    scene = synth_input("cw_scene", (1, C, H, W), 3).to(DEV)
    known = synth_input("cw_known", (1, C, H, W), 4).to(DEV)
    tiles = synth_input("cw_tiles", (nt, C, tile, tile), 5).to(DEV)
    mask = torch.ones(1, H, W, device=DEV)
    mask[0, 20:23, 18:21] = 0.0                                       # one hole, in some tiles and not in others
    want = active_tiles(mask, plan)
    assert 0 < want.size < nt

    got = _nan(nt, C, tile, tile)
    assert L.eod_scene_gather(p(scene), p(got), C, H, W, tile, p(oy), p(ox), plan.nty, plan.ntx, st) == 0
    assert torch.equal(got, gather_tiles(scene, plan))
    got = _nan(n, C, tile, tile)
    assert L.eod_scene_gather_list(p(scene), p(got), C, H, W, tile, p(oy), p(ox), plan.nty, plan.ntx, p(index), n, st) == 0
    assert torch.equal(got, gather_tiles(scene, sub))
    got = _nan(1, C, H, W)
    assert L.eod_scene_blend(p(tiles), p(got), p(wy), p(wx), p(oy), p(ox), C, H, W, tile, plan.nty, plan.ntx, st) == 0
    assert torch.equal(got, blend_tiles(tiles, plan))
    got = _nan(1, C, H, W)
    assert L.eod_scene_blend_list(p(tiles), p(got), p(wy), p(wx), p(oy), p(ox), p(slot_of), n, C, H, W, tile, plan.nty, plan.ntx, st) == 0
    assert torch.equal(got, blend_tiles(tiles[:n], sub))
    act = torch.full((nt,), -7, dtype=torch.int32, device=DEV)
    assert L.eod_scene_tile_active(p(mask), p(act), 1, H, W, tile, p(oy), p(ox), plan.nty, plan.ntx, st) == 0
    assert np.array_equal(np.flatnonzero(act.cpu().numpy()), want) and set(act.tolist()) == {0, 1}
    got = _nan(1, C, H, W)
    assert L.eod_scene_keep_known(p(scene), p(known), p(slot_of), n, p(oy), p(ox), C, H, W, tile, plan.nty, plan.ntx, p(got), st) == 0
    assert torch.equal(got, keep_known(scene, known, sub))
