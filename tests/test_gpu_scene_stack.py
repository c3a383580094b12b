"""GPU: a STACK of B scenes in one call -- the scene kernels with a leading scene dimension (csrc/scene.hip: eod_scene_stack_gather /
_blend / _tile_active / _keep_known), eod_scene_stats, tiling.TileStack, EODiffusion.sampling_scene(n_scenes=B, sample_offset=k),
DDIMSampler.sample_scene(n_scenes=B) and dist.sharded_sampling_scene.

The claim is BIT equality (torch.equal) throughout: member b of a stacked call is the single-scene call on scene b's inputs (Philox:
with sample_offset + b; injected draws: with scene b's draws), whatever else is in the stack, whatever tile_batch is and however the
stack is split over calls.  Every whole-call test first asserts its premises from the host-side plan: how many tiles of each scene
are active, and that every pixel class it compares is non-empty."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from eo_diffusion_amd import _lib
from eo_diffusion_amd._lib import EodError
from eo_diffusion_amd.diffusion.util import make_resample_schedule
from eo_diffusion_amd.tiling import (TilePlan, TileStack, active_tiles, blend_tiles, gather_padded, gather_tiles, keep_known, scene_stats,
                                     tile_slots, tiled_estimate)
from tests.gpu_util import DEV
from tests.synth import synth_input
from tests.test_gpu_scene import check_blend, cut
from tests.test_gpu_scene_skip import Calls, _diffusion, rect_holes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24

# odd widths (scalar paths), last tiles shifted inwards on both axes, a 256-pixel tile, an odd tile size
KERNEL_PLANS = [(40, 57, 16, 4), (150, 217, 64, 8), (200, 264, 64, 16), (128, 777, 64, 24), (50, 61, 18, 5), (300, 257, 256, 16)]


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def ragged(plan, B, seed):
    """a listed stack: scene 0 some tiles, scene 1 NONE, scene 2 ALL, every further scene its own random pick"""
    assert B >= 3
    rng = np.random.default_rng(seed)
    nt = plan.n_tiles
    out = sorted(rng.choice(nt, size=max(1, nt // 3), replace=False).tolist())
    out += [2 * nt + i for i in range(nt)]
    for b in range(3, B):
        out += [b * nt + i for i in sorted(rng.choice(nt, size=int(rng.integers(1, nt + 1)), replace=False).tolist())]
    st = TileStack(plan, B, out)
    per = st.per_scene()
    assert per[1].size == 0 and per[2].size == nt and (0 < per[0].size < nt or nt == 1)
    assert len({tuple(p.tolist()) for p in per}) >= 3                 # the scenes have different active sets
    return st


# ------------------------------------------------------------------------------------------------------------------ 1. gather
@pytest.mark.parametrize("C", [1, 3, 13])
@pytest.mark.parametrize("H,W,tile,overlap", KERNEL_PLANS)
def test_stacked_gather_is_torch_slicing_per_scene(H, W, tile, overlap, C):
    plan = TilePlan(H, W, tile, overlap)
    B = 4
    if W % 2 == 1:
        assert any(int(o) % 2 for o in plan.origins_x) or W % 4 != 0  # (scalar loads somewhere)
    scenes = synth_input("stg", (B, C, H, W), 3).to(DEV)
    want = torch.cat([cut(scenes[b:b + 1], plan) for b in range(B)])
    stack = TileStack(plan, B)
    out = _nan(stack.n_tiles, C, tile, tile)
    got = gather_tiles(scenes, stack, out=out)
    assert got.shape == (B * plan.n_tiles, C, tile, tile) and _bits(got, want)
    for b in range(B):                                               # ... which is the single-scene kernel's result, scene by scene
        assert _bits(got[b * plan.n_tiles:(b + 1) * plan.n_tiles], gather_tiles(scenes[b:b + 1], plan))
    lst = ragged(plan, B, H + C)
    out = _nan(lst.n_tiles, C, tile, tile)                           # exactly n_list tiles: a write behind it leaves the allocation
    got = gather_tiles(scenes, lst, out=out)
    assert got.shape[0] == lst.n_tiles and _bits(got, want[torch.from_numpy(lst.index).long().to(DEV)])


def test_stacked_gather_from_an_unaligned_view_into_a_padded_buffer():
    plan = TilePlan(150, 217, 64, 8)
    assert any(int(o) % 2 for o in plan.origins_x)
    B = 3
    base = synth_input("stu", (B * 3 * 150 * 217 + 1,), 5).to(DEV)
    scenes = base[1:].view(B, 3, 150, 217)
    want = torch.cat([cut(scenes[b:b + 1], plan) for b in range(B)])
    lst = ragged(plan, B, 9)
    chunk, slots = tile_slots(lst, 5)
    assert slots > lst.n_tiles
    out = _nan(slots, 3, 64, 64)
    got = gather_tiles(scenes, lst, out=out)
    idx = torch.from_numpy(lst.index).long().to(DEV)
    assert _bits(got, want[idx]) and bool(torch.isnan(out[lst.n_tiles:]).all())   # the padding slots are the caller's
    pad = gather_padded(scenes, lst, 5)
    assert pad.shape[0] == slots and _bits(pad[:lst.n_tiles], got) and all(_bits(pad[k], got[-1]) for k in range(lst.n_tiles, slots))
    aligned = torch.empty(B * 3 * 152 * 216 + 4, device=DEV)          # W % 4 == 0 but the view starts 4 bytes in
    al = aligned[1:1 + B * 3 * 152 * 216].view(B, 3, 152, 216)
    al.copy_(synth_input("stu2", (B, 3, 152, 216), 6))
    p2 = TilePlan(152, 216, 64, 8)
    assert _bits(gather_tiles(al, TileStack(p2, B)), torch.cat([cut(al[b:b + 1], p2) for b in range(B)]))


# ------------------------------------------------------------------------------------------------------------------- 2. blend
# every plan with C 1 and 3 at the three scales; C = 13 at scale 1 on the plans of at most 200 x 300 pixels, C = 2 on the larger ones
BLEND_CASES = [(*p, C, scale) for p in KERNEL_PLANS for C in (1, 3) for scale in (1.0, 1e-30, 1e30)]
BLEND_CASES += [(*p, 13 if p[0] * p[1] <= 200 * 300 else 2, 1.0) for p in KERNEL_PLANS]


@pytest.mark.parametrize("H,W,tile,overlap,C,scale", BLEND_CASES)
def test_stacked_blend_is_the_single_scene_blend_per_scene(H, W, tile, overlap, C, scale):
    plan = TilePlan(H, W, tile, overlap)
    B, nt = 4, plan.n_tiles
    tiles = (synth_input("stb", (B * nt, C, tile, tile), 11) * scale).to(DEV)
    got = blend_tiles(tiles, TileStack(plan, B), out=_nan(B, C, H, W))
    assert got.shape == (B, C, H, W)
    for b in range(B):
        mine = tiles[b * nt:(b + 1) * nt]
        assert _bits(got[b:b + 1], blend_tiles(mine, plan, out=_nan(1, C, H, W)))
    if C <= 3 and H * W <= 200 * 300:                                # the emulation and the float64 bound of tests/test_gpu_scene.py
        for b in (0, B - 1):
            check_blend(got[b:b + 1], tiles[b * nt:(b + 1) * nt], plan, f"scene {b} of {B}, scale {scale:g}")
    # the list form on a ragged list: per scene the single-scene list blend; all zeros for a scene with no listed tile
    lst = ragged(plan, B, W + C)
    compact = tiles[torch.from_numpy(lst.index).long().to(DEV)].clone()
    out = blend_tiles(compact, lst, out=_nan(B, C, H, W))
    est = torch.from_numpy(lst.estimated()).to(DEV)[:, None].expand_as(out)
    assert _bits(out[est], got[est]) and bool((out[~est].view(torch.int32) == 0).all())      # exactly +0.0, nothing left NaN
    lo = 0
    for b, p in enumerate(lst.per_scene()):
        if p.size == 0:
            assert bool((out[b].view(torch.int32) == 0).all())
            continue
        want = blend_tiles(compact[lo:lo + p.size], plan.subset(p), out=_nan(1, C, H, W))
        assert _bits(out[b:b + 1], want)
        if p.size == nt:
            assert _bits(out[b], got[b])
        lo += p.size


def test_stacked_blend_with_unaligned_buffers():
    plan = TilePlan(200, 264, 64, 16)
    B, nt = 3, plan.n_tiles
    tiles = synth_input("stbu", (B * nt, 3, 64, 64), 12).to(DEV)
    want = blend_tiles(tiles, TileStack(plan, B))
    base = _nan(tiles.numel() + 1)
    base[1:] = tiles.reshape(-1)
    assert _bits(blend_tiles(base[1:].view(B * nt, 3, 64, 64), TileStack(plan, B)), want)
    ob = _nan(B * 3 * 200 * 264 + 1)
    blend_tiles(tiles, TileStack(plan, B), out=ob[1:])
    assert _bits(ob[1:].view(B, 3, 200, 264), want)


# ---------------------------------------------------------------------------------------------------------- 3. classification
@pytest.mark.parametrize("H,W,tile,overlap", KERNEL_PLANS)
def test_tile_active_on_a_stacked_mask_is_the_host_rule_per_scene(H, W, tile, overlap):
    plan = TilePlan(H, W, tile, overlap)
    rng = np.random.default_rng(H * W)
    B, nt = 5, plan.n_tiles
    for Cm in (1, 3):
        m = np.ones((B, Cm, H, W), dtype=np.float32)
        y, x = int(rng.integers(0, H - 8)), int(rng.integers(0, W - 8))
        m[0, 0, y:y + 7, x:x + 5] = 0.0
        m[1, Cm - 1, H - 1, W - 1] = np.nan
        m[3] = 0.0
        m[4, 0, 0, 0] = 0.5
        want = np.concatenate([plan.active_tiles(m[b]).astype(np.int64) + b * nt for b in range(B)])
        assert plan.active_tiles(m[2]).size == 0 and plan.active_tiles(m[3]).size == nt
        got = active_tiles(torch.from_numpy(m).to(DEV), TileStack(plan, B))
        assert got.dtype == np.int32 and np.array_equal(got, want)
        assert np.array_equal(TileStack(plan, B).active_tiles(m), want)
        base = _nan(m.size + 1)
        base[1:] = torch.from_numpy(m).to(DEV).reshape(-1)
        assert np.array_equal(active_tiles(base[1:].view(B, Cm, H, W), TileStack(plan, B)), want)
    out = torch.full((B * nt,), 77, dtype=torch.int32, device=DEV)  # every entry is written
    oy, ox, _, _ = plan.device_tables(DEV)
    mm = torch.from_numpy(m).to(DEV)
    assert _lib.lib().eod_scene_stack_tile_active(mm.data_ptr(), out.data_ptr(), B, Cm, H, W, tile, oy.data_ptr(), ox.data_ptr(), plan.nty,
                                                  plan.ntx, 0) == 0
    assert set(out.cpu().tolist()) <= {0, 1} and np.array_equal(np.flatnonzero(out.cpu().numpy()), want)


# -------------------------------------------------------------------------------------------------------------- 4. keep_known
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("H,W,tile,overlap", KERNEL_PLANS)
def test_stacked_keep_known_vs_torch_where(H, W, tile, overlap, C):
    plan = TilePlan(H, W, tile, overlap)
    B = 4
    x = synth_input("stx", (B, C, H, W), 13).to(DEV)
    known = synth_input("stk", (B, C, H, W), 14).to(DEV)
    lst = ragged(plan, B, 2 * H + C)
    est = torch.from_numpy(lst.estimated()).to(DEV)[:, None]
    assert bool(est.any()) and bool((~est).any())
    got = keep_known(x, known, lst, out=_nan(B, C, H, W))
    assert _bits(got, torch.where(est, x, known))
    assert _bits(got[1], known[1]) and _bits(got[2], x[2])           # the scene with no listed tile, and the scene with all
    base = _nan(x.numel() + 1)
    base[1:] = x.reshape(-1)
    assert _bits(keep_known(base[1:].view(B, C, H, W), known, lst), torch.where(est, x, known))


def test_tiled_estimate_of_a_stack_numbers_slots_across_scenes():
    plan = TilePlan(40, 57, 16, 4)
    B, nt = 3, plan.n_tiles
    lst = TileStack(plan, B, [0, 1, 2, 5, 6, 7, 2 * nt + 3, 2 * nt + 14])
    scenes = synth_input("sts", (B, 3, 40, 57), 15).to(DEV)
    seen = []

    def fn(x, lo):
        seen.append((lo, x.clone()))
        return x * 2.0

    got = tiled_estimate(scenes, lst, 3, fn)
    assert [lo for lo, _ in seen] == [0, 3, 6]
    allt = torch.cat([cut(scenes[b:b + 1], plan) for b in range(B)])
    assert _bits(torch.cat([x for _, x in seen]), allt[[0, 1, 2, 5, 6, 7, 2 * nt + 3, 2 * nt + 14, 2 * nt + 14]])   # chunk 2 mixes scenes 0 and 2
    full = tiled_estimate(scenes, TileStack(plan, B), 16, lambda x, lo: x * 2.0)
    est = torch.from_numpy(lst.estimated()).to(DEV)[:, None].expand_as(got)
    assert bool(est.any()) and _bits(got[est], full[est]) and bool((got[~est] == 0).all()) and bool((got[1] == 0).all())


# ------------------------------------------------------------------------------------------------------------------- 5. stats
def stats_emulated(x):
    """eod_scene_stats in plain torch fp32 on the CPU, operation by operation (every torch op below rounds once, to nearest):
    s = x_0; s = s + x_b; mean = s / B; q = d_0 * d_0; q = q + d_b * d_b with d_b = x_b - mean; std = sqrt(q / (B - 1)); B = 1: 0.
    The root is taken in float64 and rounded to fp32, which IS the correctly rounded fp32 root (csrc/scene.hip sqrt_rn has the
    argument).  The vectorised torch.sqrt on an fp32 CPU tensor is not correctly rounded (it differs from numpy's fp32 root and from
    the float64 route, which agree with each other), so it cannot stand for the stated operation."""
    x = x.detach().float().cpu()
    B = x.shape[0]
    s = x[0].clone()
    for b in range(1, B):
        s = s + x[b]
    mean = s / torch.full_like(s, float(B))
    if B == 1:
        return mean, torch.zeros_like(mean)
    q = None
    for b in range(B):
        d = x[b] - mean
        p = d * d
        q = p if q is None else q + p
    return mean, torch.sqrt((q / torch.full_like(q, float(B - 1))).double()).float()


@pytest.mark.parametrize("scale", [1.0, 1e-30, 1e30])
@pytest.mark.parametrize("B", [1, 2, 5, 16, 19])
def test_scene_stats_is_bit_equal_to_the_emulation(B, scale):
    for shape in ((B, 3, 40, 57), (B, 1, 33, 31), (B, 2, 64, 64)):   # odd n (scalar form), n % 4 == 0 (vector form)
        x = synth_input("stat", shape, 21 + B) * scale
        x[:, 0, 3] = x[0, 0, 3].clone()                               # a row where every draw agrees
        x[:, 0, 5] += 100.0 * scale                                   # spread small against the mean
        want_mean, want_std = stats_emulated(x)
        mean, std = scene_stats(x.to(DEV))
        assert mean.shape == std.shape == (1,) + shape[1:]
        nm = int((mean[0].cpu().view(torch.int32) != want_mean.view(torch.int32)).sum())
        ns = int((std[0].cpu().view(torch.int32) != want_std.view(torch.int32)).sum())
        print(f"B = {B}, scale {scale:g}, {shape}: mean differs in {nm} elements, std in {ns} of {want_mean.numel()}")
        assert nm == 0 and ns == 0
        if B > 1 and scale == 1.0:
            assert bool((std[0, 0, 4] > 0).all())
        if B == 1:
            assert _bits(mean[0].cpu(), x[0]) and bool((std.view(torch.int32) == 0).all())


def test_scene_stats_on_an_unaligned_view_writes_every_element():
    B, shape = 5, (3, 24, 28)
    n = 3 * 24 * 28
    assert n % 4 == 0
    x = synth_input("statu", (B,) + shape, 31)
    want_mean, want_std = stats_emulated(x)
    base = _nan(B * n + 1)
    base[1:] = x.to(DEV).reshape(-1)
    mean, std = scene_stats(base[1:].view((B,) + shape))             # x starts 4 bytes into its allocation: the scalar form
    assert _bits(mean[0].cpu(), want_mean) and _bits(std[0].cpu(), want_std)
    out = _nan(2 * n + 1)                                            # unaligned outputs, NaN-prefilled
    L = _lib.lib()
    xd = x.to(DEV)
    assert L.eod_scene_stats(xd.data_ptr(), out[1:].data_ptr(), out[1 + n:].data_ptr(), B, n, 0) == 0
    assert _bits(out[1:1 + n].cpu().view(shape), want_mean) and _bits(out[1 + n:].cpu().view(shape), want_std)
    assert bool(torch.isnan(out[:1]).all())
    buf = _nan(2, *shape)
    mean, std = scene_stats(xd, out=buf)
    assert mean.data_ptr() == buf.data_ptr() and bool(torch.isfinite(buf).all()) and _bits(buf[0].cpu(), want_mean) and _bits(buf[1].cpu(), want_std)


@pytest.mark.parametrize("B", [2, 5, 16])
def test_scene_stats_within_the_float64_bound(B):
    """Against float64 on the same fp32 inputs, u = 2^-24, A = sum_b |x_b| / B, sd = the float64 sample standard deviation.
    mean: B - 1 additions and one division, each within a factor (1 + u):  |mean - mean64| <= B u A (1 + 1e-4) + 2^-149.
    std: write dm for that bound on the mean.  Each d_b = fl(x_b - mean) is off by at most dm + u (|x_b - mean64| + dm); each term of
    q passes one multiplication, at most B - 1 additions and the division, B + 1 roundings, i.e. a factor within (1 + (B + 1) u / 2)
    on the term's square root; the square root rounds once more.  With the triangle inequality of the 2-norm over b
        |std - sd| <= ((B + 5) / 2) u sd (1 + 1e-3) + sqrt(B / (B - 1)) dm (1 + 1e-3) + 2^-70
    (2^-70 covers squares that underflow: at most 2^-149 per term of q, less than 2^-74 on std).  The inputs include rows whose
    spread is 1e-4 of their mean, where the second term dominates."""
    shape = (B, 3, 40, 57)
    x = synth_input("stat64", shape, 41)
    x[:, 1] = 100.0 + 0.01 * x[:, 1]
    mean, std = scene_stats(x.to(DEV))
    x64 = x.double()
    mean64, sd = x64.mean(0), x64.std(0, unbiased=True)
    A = x64.abs().sum(0) / B
    dm = B * U * A * (1 + 1e-4) + 2.0 ** -149
    em = (mean[0].cpu().double() - mean64).abs()
    es = (std[0].cpu().double() - sd).abs()
    bs = (B + 5) / 2 * U * sd * (1 + 1e-3) + math.sqrt(B / (B - 1)) * dm * (1 + 1e-3) + 2.0 ** -70
    print(f"B = {B}: mean max err / bound {float((em / dm).max()):.3f}; std max err / bound {float((es / bs).max()):.3f}")
    assert bool((em <= dm).all()) and bool((es <= bs).all())


# -------------------------------------------------------------------------------------------------- 6. bad arguments, -1, no launch
def test_bad_arguments_to_the_stack_entry_points():
    plan = TilePlan(32, 48, 16, 4)
    B, nt = 2, plan.n_tiles
    lst = TileStack(plan, B, [1, 4, nt + 2])
    L = _lib.lib()
    oy, ox, wy, wx = plan.device_tables(DEV)
    index, slot_of = lst.device_tables(DEV)
    p = lambda x: x.data_ptr()
    t = _nan(B * nt, 3, 16, 16)
    sc = _nan(B, 3, 32, 48)
    a = torch.full((B * nt,), 77, dtype=torch.int32, device=DEV)
    assert L.eod_scene_stack_gather(p(sc), p(t), 0, 3, 32, 48, 16, p(oy), p(ox), plan.nty, plan.ntx, 0, 0, 0) == -1           # B = 0
    assert L.eod_scene_stack_gather(p(sc), p(t), B, 3, 32, 8, 16, p(oy), p(ox), plan.nty, plan.ntx, 0, 0, 0) == -1            # W < s
    assert L.eod_scene_stack_gather(0, p(t), B, 3, 32, 48, 16, p(oy), p(ox), plan.nty, plan.ntx, 0, 0, 0) == -1
    assert L.eod_scene_stack_gather(p(sc), p(t), B, 3, 32, 48, 16, p(oy), p(ox), plan.nty, plan.ntx, p(index), 0, 0) == -1     # empty list
    assert L.eod_scene_stack_gather(p(sc), p(t), B, 3, 32, 48, 16, p(oy), p(ox), plan.nty, plan.ntx, p(index), B * nt + 1, 0) == -1
    assert L.eod_scene_stack_gather(p(sc), p(t), 1 << 30, 3, 32, 48, 16, p(oy), p(ox), plan.nty, plan.ntx, 0, 0, 0) == -1      # B * nt > int32
    assert L.eod_scene_stack_blend(p(t), p(sc), p(wy), p(wx), p(oy), p(ox), 0, 0, -1, 3, 32, 48, 16, plan.nty, plan.ntx, 0) == -1
    assert L.eod_scene_stack_blend(p(t), 0, p(wy), p(wx), p(oy), p(ox), 0, 0, B, 3, 32, 48, 16, plan.nty, plan.ntx, 0) == -1
    assert L.eod_scene_stack_blend(p(t), p(sc), p(wy), p(wx), p(oy), p(ox), p(slot_of), 0, B, 3, 32, 48, 16, plan.nty, plan.ntx, 0) == -1
    assert L.eod_scene_stack_blend(p(t), p(sc), p(wy), p(wx), p(oy), p(ox), p(slot_of), B * nt + 1, B, 3, 32, 48, 16, plan.nty, plan.ntx, 0) == -1
    assert L.eod_scene_stack_tile_active(p(sc), p(a), B, 0, 32, 48, 16, p(oy), p(ox), plan.nty, plan.ntx, 0) == -1
    assert L.eod_scene_stack_tile_active(p(sc), 0, B, 1, 32, 48, 16, p(oy), p(ox), plan.nty, plan.ntx, 0) == -1
    assert L.eod_scene_stack_tile_active(p(sc), p(a), 0, 1, 32, 48, 16, p(oy), p(ox), plan.nty, plan.ntx, 0) == -1
    assert L.eod_scene_stack_keep_known(p(sc), p(sc), 0, 3, p(oy), p(ox), B, 3, 32, 48, 16, plan.nty, plan.ntx, p(sc), 0) == -1
    assert L.eod_scene_stack_keep_known(p(sc), p(sc), p(slot_of), 0, p(oy), p(ox), B, 3, 32, 48, 16, plan.nty, plan.ntx, p(sc), 0) == -1
    assert L.eod_scene_stack_keep_known(p(sc), p(sc), p(slot_of), 3, p(oy), p(ox), 0, 3, 32, 48, 16, plan.nty, plan.ntx, p(sc), 0) == -1
    assert L.eod_scene_stats(p(sc), p(sc), p(sc), 0, 16, 0) == -1
    assert L.eod_scene_stats(p(sc), p(sc), p(sc), 2, 0, 0) == -1
    assert L.eod_scene_stats(0, p(sc), p(sc), 2, 16, 0) == -1
    assert L.eod_scene_stats(p(sc), p(sc), 0, 2, 16, 0) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(t).all()) and bool(torch.isnan(sc).all()) and bool((a == 77).all())      # nothing was launched
    # the Python layer refuses, too
    with pytest.raises(EodError):
        gather_tiles(torch.zeros(1, 3, 32, 48, device=DEV), TileStack(plan, 2))
    with pytest.raises(EodError):
        gather_tiles(torch.zeros(3, 32, 48, device=DEV), TileStack(plan, 1))
    with pytest.raises(EodError):
        blend_tiles(torch.zeros(nt, 3, 16, 16, device=DEV), TileStack(plan, 2))
    with pytest.raises(EodError):
        keep_known(torch.zeros(2, 3, 32, 48, device=DEV), torch.zeros(2, 3, 32, 48, device=DEV), TileStack(plan, 2))
    with pytest.raises(EodError):
        keep_known(torch.zeros(2, 3, 32, 48, device=DEV), torch.zeros(1, 3, 32, 48, device=DEV), lst)
    with pytest.raises(EodError):
        active_tiles(torch.ones(3, 1, 32, 48, device=DEV), TileStack(plan, 2))
    with pytest.raises(EodError):
        scene_stats(torch.zeros(3, 32, 48, device=DEV))


def test_the_stack_tables_are_not_trusted_with_an_address():
    plan = TilePlan(32, 48, 16, 4)
    B, nt = 2, plan.n_tiles
    lst = TileStack(plan, B, [1, nt + 4])
    L = _lib.lib()
    oy, ox, wy, wx = plan.device_tables(DEV)
    p = lambda x: x.data_ptr()
    t = torch.ones(2, 3, 16, 16, device=DEV)
    sc = _nan(B, 3, 32, 48)
    wild = torch.from_numpy(np.where(lst.slot_of >= 0, lst.slot_of + 2, -1).astype(np.int32)).to(DEV)   # slots 2, 3 of a 2-tile buffer
    assert L.eod_scene_stack_blend(p(t), p(sc), p(wy), p(wx), p(oy), p(ox), p(wild), 2, B, 3, 32, 48, 16, plan.nty, plan.ntx, 0) == 0
    assert bool((sc == 0).all())
    bad = torch.tensor([1, B * nt], dtype=torch.int32, device=DEV)
    src = torch.ones(B, 3, 32, 48, device=DEV)
    assert L.eod_scene_stack_gather(p(src), p(t), B, 3, 32, 48, 16, p(oy), p(ox), plan.nty, plan.ntx, p(bad), 2, 0) == 0
    assert bool((t[0] == 1).all()) and bool(torch.isnan(t[1]).all())


# -------------------------------------------------------------------------------------------------------- the samplers' inputs
S16 = (40, 57, 16, 4)                                                # 3 x 5 tiles of 16, odd width, both last tiles shifted
HOLES = [[(14, 20, 10, 30)], [(26, 32, 40, 50)], [], [(0, 3, 52, 57), (36, 40, 0, 4)], [(14, 20, 10, 30)]]   # scene 2: nothing to do


def stack_case(B, seed, channels=1):
    """(plan, masks [B, 1 or 3, H, W] numpy, gt [B, 3, H, W], a_b) -- premises asserted through the host rule"""
    H, W, tile, overlap = S16
    plan = TilePlan(H, W, tile, overlap)
    masks = np.stack([np.repeat(rect_holes(H, W, HOLES[b])[None], channels, 0) for b in range(B)])
    gt = synth_input("stgt", (B, 3, H, W), seed, uniform=True) * 2 - 1
    a = [int(plan.active_tiles(masks[b]).size) for b in range(B)]
    assert a[:3] == [6, 4, 0][:B] and all(n < plan.n_tiles for n in a) and len(set(a[:3])) == min(B, 3)
    return plan, masks, gt, a


def assert_classes(plan, masks, skip_known):
    """per scene (est [B, H, W] torch bool on DEV); with skip_known every compared class must be non-empty somewhere in the stack"""
    B = masks.shape[0]
    act = TileStack(plan, B).active_tiles(masks)
    est = TileStack(plan, B, act).estimated() if act.size else np.zeros((B, plan.H, plan.W), dtype=bool)
    hole = (masks != 1).any(axis=1)
    assert bool(est[hole].all()) and hole.sum() > 0 and (est & ~hole).sum() > 0 and (~est).sum() > 0
    return torch.from_numpy(est).to(DEV)


def ddpm_stack_vs_singles(m, plan, cond, B, *, clip=True, seed=5, k=0, y=None, what="", **kw):
    """philox: the stacked call, and the B single-scene calls it replaces; returns the stacked result"""
    run = lambda **a: m.sampling_scene((plan.H, plan.W), clip, DEV, overlap=plan.overlap, seed=seed, progress=False, **kw, **a)
    stack = run(cond=cond, y=y, n_scenes=B, sample_offset=k)
    assert stack.shape == (B, 3, plan.H, plan.W) and bool(torch.isfinite(stack).all())
    for b in range(B):
        one = run(cond=None if cond is None else cond[b:b + 1], y=None if y is None else y[b:b + 1], sample_offset=k + b)
        n = int((stack[b:b + 1] != one).sum())
        print(f"{what}: scene {b} of {B} (sample {k + b}): {n} of {one.numel()} elements differ from the single-scene call")
        assert torch.equal(stack[b:b + 1], one)
    return stack


# ------------------------------------------------------------------------------------------------------- 7. Philox equivalence
@pytest.mark.parametrize("skip_known", [False, True])
@pytest.mark.parametrize("attn", [False, True])
@pytest.mark.parametrize("prec", ["fp32x3", "fp16"])
@pytest.mark.parametrize("clip", [True, False])
def test_ddpm_stack_equals_the_single_scene_calls(clip, prec, attn, skip_known):
    B = 4
    plan, masks, gt, a = stack_case(B, 81)
    assert_classes(plan, masks, skip_known)
    m = _diffusion(prec, attn, 6, "sum", s=16)
    cond = torch.cat([gt, torch.from_numpy(masks)], 1)
    stack = ddpm_stack_vs_singles(m, plan, cond, B, clip=clip, k=3, skip_known=skip_known, tile_batch=4,
                                  what=f"clip={clip} {prec} attn={attn} skip_known={skip_known}")
    assert not torch.equal(stack[0], stack[4 - 1])                   # (scenes 0 and 3 are different scenes)
    if skip_known:
        assert torch.equal(stack[2], gt[2].to(DEV))                  # the scene with nothing to do is its known image


@pytest.mark.parametrize("skip_known", [False, True])
def test_ddpm_stack_with_resampling(skip_known):
    B = 3
    plan, masks, gt, a = stack_case(B, 82)
    m = _diffusion("fp32x3", False, 6, "sum", s=16)
    assert len(make_resample_schedule(6, 2, 2)[1]) > 0
    cond = torch.cat([gt, torch.from_numpy(masks)], 1)
    stack = ddpm_stack_vs_singles(m, plan, cond, B, k=1, skip_known=skip_known, resample=(2, 2), what=f"resample skip_known={skip_known}")
    plain = m.sampling_scene((plan.H, plan.W), True, DEV, cond=cond, overlap=plan.overlap, seed=5, progress=False, n_scenes=B, sample_offset=1,
                             skip_known=skip_known)
    assert not torch.equal(plain, stack)


def test_ddpm_stack_with_concatenated_cond_and_a_label_per_scene():
    B = 3
    H, W, tile, overlap = S16
    plan = TilePlan(H, W, tile, overlap)
    m = _diffusion("fp32x3", True, 6, None, s=16, in_ch=7, num_classes=5)
    cond = synth_input("stcc", (B, 4, H, W), 83, uniform=True)
    y = torch.tensor([3, 1, 4])
    stack = ddpm_stack_vs_singles(m, plan, cond, B, k=2, y=y, tile_batch=16, what="concat cond + labels")
    same = m.sampling_scene((H, W), True, DEV, cond=cond, y=torch.tensor([3]), overlap=overlap, seed=5, progress=False, n_scenes=B, sample_offset=2)
    assert torch.equal(same[0], stack[0]) and not torch.equal(same[1], stack[1])      # one label is every scene's label
    rep = m.sampling_scene((H, W), True, DEV, cond=cond, y=torch.tensor([3, 3, 3]), overlap=overlap, seed=5, progress=False, n_scenes=B, sample_offset=2)
    assert torch.equal(rep, same)


def test_ddpm_stack_without_a_known_region_is_b_draws():
    """no cond at all: B unconditional scenes, members = Philox samples k .. k + B - 1"""
    H, W, tile, overlap = S16
    plan = TilePlan(H, W, tile, overlap)
    m = _diffusion("fp32x3", False, 6, None, s=16)
    stack = ddpm_stack_vs_singles(m, plan, None, 3, k=0, what="unconditional")
    assert not torch.equal(stack[0], stack[1])


# --------------------------------------------------------------------------------------------------------- 8. injected draws
def _draws(name, n, B, H, W, seed):
    return synth_input(name, (n, B, 3, H, W), seed)


@pytest.mark.parametrize("skip_known", [False, True])
@pytest.mark.parametrize("resample", [None, (2, 2)])
def test_ddpm_stack_with_injected_draws(resample, skip_known):
    B, T = 3, 6
    plan, masks, gt, a = stack_case(B, 84)
    H, W = plan.H, plan.W
    m = _diffusion("fp32x3", True, T, "sum", s=16)
    n_eval, n_jump = T, 0
    if resample is not None:
        visits, jumps = make_resample_schedule(T, *resample)
        n_eval, n_jump = len(visits), len(jumps)
    x_T, noises = synth_input("ixT", (B, 3, H, W), 84), _draws("in", n_eval, B, H, W, 84)
    jn = _draws("ij", n_jump, B, H, W, 84) if n_jump else None
    cond = torch.cat([gt, torch.from_numpy(masks)], 1)
    run = lambda **kw: m.sampling_scene((H, W), True, DEV, overlap=plan.overlap, progress=False, resample=resample, skip_known=skip_known,
                                        tile_batch=4, **kw)
    stack = run(cond=cond, x_T=x_T, noises=noises, jump_noises=jn, n_scenes=B)
    for b in range(B):
        one = run(cond=cond[b:b + 1], x_T=x_T[b:b + 1], noises=noises[:, b:b + 1], jump_noises=None if jn is None else jn[:, b:b + 1])
        assert torch.equal(stack[b:b + 1], one), b
    fn = run(cond=cond, x_T=x_T, noises=lambda k: noises[k], jump_noises=jn, n_scenes=B)       # a callable is accepted as today
    assert torch.equal(fn, stack)


def _ddim_stack_vs_singles(smp, S, plan, B, masks_t, x0, eta, seed, resample=None, tile_batch=4, what="", **kw):
    H, W = plan.H, plan.W
    n_eval, n_jump = S, 0
    if resample is not None:
        visits, jumps = make_resample_schedule(S, *resample)
        n_eval, n_jump = len(visits), len(jumps)
    x_T = synth_input("dxT", (B, 3, H, W), seed)
    sn, mn = _draws("dsn", n_eval, B, H, W, seed), _draws("dmn", n_eval, B, H, W, seed + 1)
    jn = _draws("djn", n_jump, B, H, W, seed) if n_jump else None
    per_scene = {k: v for k, v in kw.items() if torch.is_tensor(v) and v.dim() == 4}
    rest = {k: v for k, v in kw.items() if k not in per_scene}
    run = lambda **a: smp.sample_scene(S, (H, W), overlap=plan.overlap, tile_batch=tile_batch, eta=eta, progress=False, resample=resample,
                                       **rest, **a)
    stack, inter = run(mask=masks_t, x0=x0, x_T=x_T, step_noises=sn, mix_noises=mn, jump_noises=jn, n_scenes=B, **per_scene)
    assert stack.shape == (B, 3, H, W) and bool(torch.isfinite(stack).all()) and all(z.shape[0] == B for z in inter["x_inter"])
    for b in range(B):
        one, inter1 = run(mask=masks_t[b:b + 1], x0=x0[b:b + 1], x_T=x_T[b:b + 1], step_noises=sn[:, b:b + 1], mix_noises=mn[:, b:b + 1],
                          jump_noises=None if jn is None else jn[:, b:b + 1], **{k: v[b:b + 1] for k, v in per_scene.items()})
        n = int((stack[b:b + 1] != one).sum())
        print(f"{what}: scene {b} of {B}: {n} of {one.numel()} elements differ from the single-scene call")
        assert torch.equal(stack[b:b + 1], one)
        if len(inter1["pred_x0"]) == len(inter["pred_x0"]):         # (a scene with no active tile returns early, with x0 alone)
            assert all(torch.equal(p[b:b + 1], q) for p, q in zip(inter["pred_x0"], inter1["pred_x0"]))
    return stack


@pytest.mark.parametrize("skip_known", [False, True])
@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_ddim_stack_equals_the_single_scene_calls(eta, skip_known):
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    B = 4
    plan, masks, x0, a = stack_case(B, 85)
    assert_classes(plan, masks, skip_known)
    smp = DDIMSampler(_diffusion("fp32x3", True, 20, s=16))
    stack = _ddim_stack_vs_singles(smp, 4, plan, B, torch.from_numpy(masks), x0, eta, 85, skip_known=skip_known, what=f"DDIM eta={eta} skip={skip_known}")
    if skip_known:
        assert torch.equal(stack[2], x0[2].to(DEV))


def test_ddim_stack_with_a_mask_per_channel_and_resampling():
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    B = 3
    plan, masks, x0, a = stack_case(B, 86, channels=3)
    masks[0, 1, 30:34, 2:9] = 0.0                                    # a hole in one channel is a hole
    masks[1, 2, 5:9, 5:9] = 0.5
    assert plan.active_tiles(masks[0]).size > a[0] and plan.active_tiles(masks[1]).size > a[1]
    assert_classes(plan, masks, True)
    smp = DDIMSampler(_diffusion("fp32x3", False, 20, s=16))
    for sk in (False, True):
        _ddim_stack_vs_singles(smp, 5, plan, B, torch.from_numpy(masks), x0, 0.5, 86, resample=(2, 2), tile_batch=3, skip_known=sk,
                               what=f"per-channel mask, resample, skip={sk}")


@pytest.mark.parametrize("scale", [1.0, 2.5])
def test_ddim_stack_with_conditioning_and_guidance(scale):
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    B = 3
    plan, masks, x0, a = stack_case(B, 87)
    smp = DDIMSampler(_diffusion("fp32x3", True, 20, None, s=16, in_ch=7))
    c = synth_input("dsc", (B, 4, plan.H, plan.W), 87, uniform=True)
    for sk in (False, True):
        _ddim_stack_vs_singles(smp, 4, plan, B, torch.from_numpy(masks), x0, 0.5, 87, skip_known=sk, conditioning=c,
                               unconditional_guidance_scale=scale, unconditional_conditioning=torch.zeros_like(c), what=f"guidance {scale} skip={sk}")


# -------------------------------------------------------------------------------------------- 9. broadcast, tile_batch, splits
def test_a_broadcast_known_scene_is_the_known_scene_repeated():
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    B = 3
    plan, masks, gt, a = stack_case(1, 88)
    H, W = plan.H, plan.W
    m = _diffusion("fp32x3", False, 6, "sum", s=16)
    cond1 = torch.cat([gt, torch.from_numpy(masks)], 1)
    for sk in (False, True):
        run = lambda c: m.sampling_scene((H, W), True, DEV, cond=c, overlap=plan.overlap, seed=9, progress=False, n_scenes=B, skip_known=sk)
        one, rep = run(cond1), run(cond1.repeat(B, 1, 1, 1))
        assert torch.equal(one, rep) and not torch.equal(one[0], one[1])         # B different draws of one known scene
    smp = DDIMSampler(_diffusion("fp32x3", False, 20, s=16))
    x_T, sn, mn = synth_input("bx", (B, 3, H, W), 88), _draws("bs", 4, B, H, W, 88), _draws("bm", 4, B, H, W, 89)
    for sk in (False, True):
        run = lambda mask, x0: smp.sample_scene(4, (H, W), overlap=plan.overlap, eta=0.5, mask=mask, x0=x0, x_T=x_T, step_noises=sn, mix_noises=mn,
                                                progress=False, n_scenes=B, skip_known=sk)[0]
        one = run(torch.from_numpy(masks[0, 0]), gt)                 # [H, W] mask, [1, 3, H, W] x0
        rep = run(torch.from_numpy(masks).repeat(B, 1, 1, 1), gt.repeat(B, 1, 1, 1))
        assert torch.equal(one, rep) and not torch.equal(one[0], one[1])
    # one draw for every member, too: x_T [1, ...] -- with the same known scene and the same step draws the members coincide
    same = smp.sample_scene(4, (H, W), overlap=plan.overlap, eta=0.5, mask=torch.from_numpy(masks), x0=gt, x_T=x_T[:1], step_noises=sn[:, :1],
                            mix_noises=mn[:, :1], progress=False, n_scenes=B)[0]
    assert torch.equal(same[0], same[1]) and torch.equal(same[0], same[2])


@pytest.mark.parametrize("skip_known", [False, True])
def test_the_stack_does_not_depend_on_tile_batch_or_on_how_it_is_split(skip_known):
    B = 5
    plan, masks, gt, a = stack_case(B, 90)
    m = _diffusion("fp32x3", True, 6, "sum", s=16)
    cond = torch.cat([gt, torch.from_numpy(masks)], 1)
    run = lambda c, n, off, tb: m.sampling_scene((plan.H, plan.W), True, DEV, cond=c, overlap=plan.overlap, seed=11, progress=False, n_scenes=n,
                                                 sample_offset=off, tile_batch=tb, skip_known=skip_known)
    got = {tb: run(cond, B, 2, tb) for tb in (1, 4, 16)}
    assert torch.equal(got[1], got[16]) and torch.equal(got[4], got[16])
    for k in (1, 2, 4):                                              # [0, B) in one call == [0, k) and [k, B) in two: any world size
        parts = torch.cat([run(cond[:k], k, 2, 16), run(cond[k:], B - k, 2 + k, 16)])
        assert torch.equal(parts, got[16]), k
    # three ranks with a ragged split (2, 2, 1), as dist.shard_bounds deals them
    from eo_diffusion_amd.dist import shard_bounds
    parts = []
    for r in range(3):
        lo, hi = shard_bounds(B, 3, r)
        parts.append(run(cond[lo:hi], hi - lo, 2 + lo, 16))
    assert [p.shape[0] for p in parts] == [2, 2, 1] and torch.equal(torch.cat(parts), got[16])


# ------------------------------------------------------------------------------------------------------ 10. the batch fills
@pytest.mark.parametrize("resample", [None, (2, 2)])
def test_the_unet_sees_the_chunks_of_the_whole_stack(resample):
    B, T = 4, 6
    plan, masks, gt, a = stack_case(B, 91)
    total = sum(a)
    assert a == [6, 4, 0, 2] and total == 12
    m = _diffusion("fp32x3", False, T, "sum", s=16)
    n_eval = T if resample is None else len(make_resample_schedule(T, *resample)[0])
    cond = torch.cat([gt, torch.from_numpy(masks)], 1)
    run = lambda **kw: m.sampling_scene((plan.H, plan.W), True, DEV, cond=cond, overlap=plan.overlap, progress=False, resample=resample,
                                        n_scenes=B, **kw)
    for tb in (16, 4, 5):
        with Calls(m.model) as calls:
            run(tile_batch=tb, skip_known=True)
        chunk = min(tb, total)
        assert calls.batches == [chunk] * (n_eval * math.ceil(total / chunk))
        per_scene = sum(math.ceil(n / min(tb, n)) for n in a if n)
        if tb == 16:
            assert math.ceil(total / chunk) == 1 < per_scene == 3    # one launch of 12, where scene by scene it is 6 + 4 + 2
    with Calls(m.model) as calls:
        run(tile_batch=16)
    assert calls.batches == [16] * (n_eval * math.ceil(B * plan.n_tiles / 16))   # 60 tiles: 4 launches of 16 (4 padding slots)


class Echo(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.seen = []

    def forward(self, x, t, cond=None, y=None):
        self.seen.append((x.clone(), t.clone(), None if y is None else y.clone()))
        return torch.zeros_like(x)


@pytest.mark.parametrize("tile_batch", [16, 5])
def test_the_unet_is_given_the_windows_in_global_order_with_their_scenes_labels(tile_batch):
    from eo_diffusion_amd.diffusion.model import EODiffusion
    B, T = 4, 3
    plan, masks, gt, a = stack_case(B, 92)
    H, W, nt = plan.H, plan.W, plan.n_tiles
    act = TileStack(plan, B).active_tiles(masks)
    lst = TileStack(plan, B, act)
    assert [int(g) // nt for g in act] == [0] * 6 + [1] * 4 + [3] * 2
    m = EODiffusion(Echo(), timesteps=T, image_size=plan.tile, in_channels=3, cond_type="sum", device=DEV).to(DEV)
    x_T, noises = synth_input("ex", (B, 3, H, W), 92), _draws("en", T, B, H, W, 92)
    mk = torch.from_numpy(masks)
    y = torch.tensor([7, 8, 9, 5])
    out = m.sampling_scene((H, W), True, DEV, cond=torch.cat([gt, mk], 1), y=y, x_T=x_T, noises=noises, overlap=plan.overlap,
                           tile_batch=tile_batch, skip_known=True, n_scenes=B, progress=False)
    chunk, slots = tile_slots(lst, tile_batch)
    per_step = slots // chunk
    assert len(m.model.seen) == T * per_step and all(x.shape[0] == chunk for x, _, _ in m.model.seen)
    t1 = torch.full((B,), T - 1, dtype=torch.int64, device=DEV)
    x_in = m._repaint_mix(x_T.to(DEV), gt.to(DEV), mk.to(DEV), t1, noises[0].to(DEV))
    allt = torch.cat([cut(x_in[b:b + 1], plan) for b in range(B)])
    order = act.tolist() + [int(act[-1])] * (slots - lst.n_tiles)
    assert torch.equal(torch.cat([x for x, _, _ in m.model.seen[:per_step]]), allt[order])
    labels = torch.cat([yy for _, _, yy in m.model.seen[:per_step]]).cpu()
    assert labels.tolist() == [int(y[g // nt]) for g in order]       # 7 x 6, 8 x 4, 5 x 2 (+ padding: the last tile's)
    assert all(bool((t == T - 1).all()) for _, t, _ in m.model.seen[:per_step]) and bool((m.model.seen[-1][1] == 0).all())
    est = torch.from_numpy(lst.estimated()).to(DEV)[:, None].expand_as(out)
    assert torch.equal(out[~est], gt.to(DEV)[~est]) and torch.equal(out[2], gt[2].to(DEV))


# ------------------------------------------------------------------------------------------------------ 11. skip_known on a stack
def test_skip_known_on_a_stack():
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    B = 4
    plan, masks, gt, a = stack_case(B, 93)
    est = assert_classes(plan, masks, True)
    H, W = plan.H, plan.W
    m = _diffusion("fp32x3", True, 6, "sum", s=16)
    cond = torch.cat([gt, torch.from_numpy(masks)], 1)
    run = lambda **kw: m.sampling_scene((H, W), True, DEV, cond=cond, overlap=plan.overlap, seed=13, progress=False, n_scenes=B, **kw)
    full, skip = run(), run(skip_known=True)
    known = gt.to(DEV)
    for b in range(B):
        e = est[b][None].expand(3, H, W)
        if a[b] == 0:
            assert not bool(e.any()) and torch.equal(skip[b], known[b])           # all ones: the known image itself
            continue
        assert bool(e.any()) and bool((~e).any())
        assert torch.equal(skip[b][e], full[b][e]) and torch.equal(skip[b][~e], known[b][~e])
        assert not torch.equal(full[b][~e], known[b][~e])            # (the full call denoises the known image there)
    # every mask all ones: the known images, and the UNet is never called
    ones = torch.cat([gt, torch.ones(B, 1, H, W)], 1)
    with Calls(m.model) as calls:
        out = m.sampling_scene((H, W), True, DEV, cond=ones, overlap=plan.overlap, progress=False, n_scenes=B, skip_known=True)
        img, inter = DDIMSampler(m).sample_scene(4, (H, W), overlap=plan.overlap, mask=torch.ones(H, W), x0=gt, skip_known=True, n_scenes=B,
                                                 progress=False)
    assert calls.batches == [] and torch.equal(out, known) and torch.equal(img, known) and torch.equal(inter["x_inter"][-1], img)
    # every mask all zeros: every tile active, the full path
    zeros = torch.cat([gt, torch.zeros(B, 1, H, W)], 1)
    z = lambda **kw: m.sampling_scene((H, W), True, DEV, cond=zeros, overlap=plan.overlap, seed=3, progress=False, n_scenes=B, **kw)
    assert torch.equal(z(skip_known=True), z())


# -------------------------------------------------------------------------------------------------- 12. n_scenes = 1, refusals
def test_n_scenes_1_is_the_call_without_the_keyword():
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    plan, masks, gt, a = stack_case(1, 94)
    H, W = plan.H, plan.W
    m = _diffusion("fp32x3", True, 6, "sum", s=16)
    cond = torch.cat([gt, torch.from_numpy(masks)], 1)
    for sk in (False, True):
        run = lambda **kw: m.sampling_scene((H, W), True, DEV, cond=cond, overlap=plan.overlap, seed=4, progress=False, skip_known=sk,
                                            resample=(2, 2), **kw)
        assert torch.equal(run(n_scenes=1), run()) and torch.equal(run(n_scenes=1, sample_offset=0), run())
        assert torch.equal(run(n_scenes=np.int64(1)), run())
        assert not torch.equal(run(sample_offset=1), run())
    smp = DDIMSampler(_diffusion("fp32x3", False, 20, s=16))
    kw = dict(overlap=plan.overlap, eta=0.5, mask=torch.from_numpy(masks), x0=gt, x_T=synth_input("n1", (1, 3, H, W), 94),
              step_noises=_draws("n1s", 4, 1, H, W, 94), mix_noises=_draws("n1m", 4, 1, H, W, 95), progress=False)
    for sk in (False, True):
        (one, i1), (two, i2) = smp.sample_scene(4, (H, W), skip_known=sk, n_scenes=1, **kw), smp.sample_scene(4, (H, W), skip_known=sk, **kw)
        assert torch.equal(one, two) and all(torch.equal(p, q) for p, q in zip(i1["pred_x0"], i2["pred_x0"]))


def test_new_refusals_come_before_any_launch():
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    from eo_diffusion_amd.diffusion.model import EODiffusion

    class Never(torch.nn.Module):
        def forward(self, x, t, cond=None, y=None):
            raise AssertionError("the network was reached")

    m = EODiffusion(Never(), timesteps=4, image_size=16, in_channels=3, cond_type="sum", device=DEV).to(DEV)
    smp = DDIMSampler(m)
    size = (32, 48)
    ok = torch.ones(3, 4, 32, 48)
    for kw in (dict(n_scenes=0), dict(n_scenes=-2), dict(n_scenes=1.5), dict(n_scenes=None),
               dict(n_scenes=3, cond=torch.ones(2, 4, 32, 48)), dict(n_scenes=3, cond=ok, x_T=torch.zeros(2, 3, 32, 48)),
               dict(n_scenes=3, cond=ok, x_T=torch.zeros(3, 3, 32, 47)), dict(n_scenes=3, cond=ok, y=torch.tensor([1, 2])),
               dict(n_scenes=3, cond=ok, y=torch.tensor([1, 2, 3, 4])), dict(n_scenes=3, cond=ok, tile_batch=0),
               dict(n_scenes=3, cond=ok, resample=(2, 2), noises=torch.zeros(4, 3, 3, 32, 48)),   # the walk has more than 4 evaluations
               dict(n_scenes=3, skip_known=True),                                     # nothing known
               dict(n_scenes=2, cond=ok)):
        with pytest.raises(EodError):
            m.sampling_scene(size, True, DEV, progress=False, **kw)
    # at the default the old refusals stand: two scenes, two labels
    with pytest.raises(EodError):
        m.sampling_scene(size, True, DEV, cond=torch.ones(2, 4, 32, 48), progress=False)
    with pytest.raises(EodError):
        m.sampling_scene(size, True, DEV, cond=torch.ones(1, 4, 32, 48) * 0, y=torch.tensor([1, 2]), progress=False)
    z = torch.zeros(3, 3, 32, 48)
    for kw in (dict(n_scenes=0), dict(n_scenes=3, mask=torch.ones(2, 1, 32, 48), x0=z), dict(n_scenes=3, mask=torch.ones(32, 48), x0=z[:2]),
               dict(n_scenes=3, x_T=z[:2]), dict(n_scenes=3, conditioning=torch.zeros(2, 4, 32, 48)),
               dict(n_scenes=3, mask=torch.ones(32, 48), x0=z, skip_known=True, unconditional_conditioning=torch.zeros(2, 4, 32, 48))):
        with pytest.raises(EodError):
            smp.sample_scene(2, size, progress=False, **kw)
    with pytest.raises(EodError):
        smp.sample_scene(2, size, mask=torch.ones(2, 1, 32, 48), x0=z[:1], progress=False)


# ------------------------------------------------------------------------------------------------------------ 13. multi-GPU
def test_sharded_sampling_scene_through_a_one_rank_rccl_group():
    """dist.sharded_sampling_scene(force_gather=True) under a one-rank nccl group == the plain stacked call, in a fresh child
    process (tests/scene_stack_dist_child.py), as tests/test_gpu_dist.py does for sharded_sampling"""
    from tests.test_gpu_dist import _child_env, _json_lines
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "scene_stack_dist_child.py")], env=_child_env(), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = _json_lines(r.stdout)
    assert len(out) == 1, r.stdout
    assert out[0] == {"backend": "nccl", "world": 1, "sharded_equals_stacked_bits": True, "skip_known_equals_stacked_bits": True,
                      "members_differ": True, "finite": True, "on_gpu": True, "shape": [3, 3, 40, 57]}
