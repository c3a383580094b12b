#!/usr/bin/env python3
"""What stacking B scenes into one call buys when skip_known leaves each of them a few active tiles.

One process, the arms alternating, HIP events around each timed window.  The UNet keeps ONE launch program, for one batch size
(UNetModel.program_for rebuilds it when the batch size changes), so no timed window mixes chunk sizes: every window is preceded by an
untimed call of its own shape, and arm (b) times each scene's step in windows of its own and sums them -- which is what the B separate
sampling_scene calls it stands for pay, each running its whole chain at one chunk size.
  (a) one step of the stacked call (EODiffusion._scene_step on the listed TileStack: one mix, one gather, the UNet on chunks of
      min(tile_batch, active tiles of the whole stack), one blend, one update);
  (b) the B single-scene steps it replaces (each on its own TileSubset, chunk = min(tile_batch, that scene's active tiles));
  (c) the UNet launches of (a) alone, on pre-cut tiles.
The yardstick for (a) is (b) of the same run.  The padded share of the tile slots is printed for both arms.  The masks are seeded
rectangles of 10-40 % of each side (harness.make_label), one per scene.  The noise is drawn before the timed windows.  Also timed on
their own: eod_scene_stats and the stacked gather / blend over the whole stack (bytes from the shapes -> GB/s; these buffers fit the
Infinity Cache), and eod_scene_stats on a 16 x 3 x 2048 x 2048 stack (805 MB, which does not): its streaming rate.

    python tools/scene_stack_bench.py [--height 600] [--width 777] [--tile 256] [--overlap 32] [--scenes 4 8] [--tile-batch 16] [--reps 7]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import build_model  # noqa: E402
from eo_diffusion_amd import harness  # noqa: E402
from eo_diffusion_amd.tiling import TilePlan, TileStack, blend_tiles, gather_padded, gather_tiles, scene_stats, tile_slots  # noqa: E402
from tools.scene_bench import timed  # noqa: E402


def spread(v):
    med = statistics.median(v)
    return {"median": round(med, 3), "min": round(min(v), 3), "max": round(max(v), 3), "spread": round((max(v) - min(v)) / med, 4)}


def one_stack(m, plan, B, args, dev):
    C, s, i = 3, plan.tile, 500
    H, W = plan.H, plan.W
    masks = np.stack([1.0 - harness.make_label((H, W), 10, 10, 40, 40, rng=np.random.RandomState(args.seed + b)).astype(np.float32)
                      for b in range(B)])[:, None]                   # 1 = keep
    stack = TileStack(plan, B)
    act = stack.active_tiles(masks)
    lst = TileStack(plan, B, act)
    subs = [plan.subset(p) if p.size else None for p in lst.per_scene()]
    mask = torch.from_numpy(masks).to(dev)
    gt = m._philox((B, C, H, W), dev, 2, 0, 0, 0).clamp_(-1, 1)
    x = m._philox((B, C, H, W), dev, 1, 0, m.timesteps, 0)
    z = m._philox((B, C, H, W), dev, 1, 0, i, 1)
    chunk, slots = tile_slots(lst, args.tile_batch)
    x_tiles = gather_padded(x, lst, args.tile_batch).clone()
    t_chunk = torch.full((chunk,), i, dtype=torch.int64, device=dev)
    singles = [(x[b:b + 1].contiguous(), z[b:b + 1].contiguous(), gt[b:b + 1].contiguous(), mask[b:b + 1].contiguous(), subs[b])
               for b in range(B) if subs[b] is not None]

    def arm_stack():
        return m._scene_step(x, i, z, lst, args.tile_batch, True, gt, mask)

    def single(k):
        xb, zb, gb, mb, sub = singles[k]
        return lambda: m._scene_step(xb, i, zb, sub, args.tile_batch, True, gb, mb)

    def warm(fn):
        """an untimed window of fn's shape: fn(), then timed(fn, ...) starts on a program built for fn's chunk size"""
        fn()
        return timed(fn, args.steps)

    def unet_only():
        for lo in range(0, slots, chunk):
            m.model(x_tiles[lo:lo + chunk], t_chunk)

    with torch.no_grad():
        for fn in [arm_stack, unet_only] + [single(k) for k in range(len(singles))]:  # every shape of the timed windows, all arms
            fn(), fn()
        torch.cuda.synchronize()
        ta, tb, tc, per = [], [], [], [[] for _ in singles]
        for _ in range(args.reps):
            ta.append(warm(arm_stack))
            for k in range(len(singles)):
                per[k].append(warm(single(k)))
            tb.append(sum(p[-1] for p in per))
            tc.append(warm(unet_only))
        # the streaming kernels on the whole stack
        tiles_out = torch.empty((stack.n_tiles, C, s, s), dtype=torch.float32, device=dev)
        scene_out = torch.empty((B, C, H, W), dtype=torch.float32, device=dev)
        stats_out = torch.empty((2, C, H, W), dtype=torch.float32, device=dev)
        gather_tiles(x, stack, out=tiles_out)
        kern = {"stack_gather": lambda: gather_tiles(x, stack, out=tiles_out), "stack_blend": lambda: blend_tiles(tiles_out, stack, out=scene_out),
                "scene_stats": lambda: scene_stats(x, out=stats_out)}
        kt = {}
        for name, fn in kern.items():
            timed(fn, 5)
            kt[name] = [timed(fn, 50) for _ in range(args.reps)]
    per_scene = lst.per_scene()
    single_slots = [tile_slots(sub, args.tile_batch) for *_, sub in singles]
    b_slots, b_launch = sum(sl for _, sl in single_slots), sum(sl // ch for ch, sl in single_slots)
    med = statistics.median
    scene_bytes, tile_bytes = B * C * H * W * 4, stack.n_tiles * C * s * s * 4
    res = {"scenes": B, "active_tiles_per_scene": [int(p.size) for p in per_scene], "active_tiles": int(lst.n_tiles),
           "a_stacked": {"launches_per_step": slots // chunk, "chunk": chunk, "slots": slots, "padded_share_of_slots": round((slots - lst.n_tiles) / slots, 4)},
           "b_singles": {"launches_per_step": b_launch, "chunks": [ch for ch, _ in single_slots], "slots": b_slots,
                         "padded_share_of_slots": round((b_slots - lst.n_tiles) / b_slots, 4),
                         "step_ms_per_scene": [round(med(p), 3) for p in per]},
           "a_stacked_step_ms": spread(ta), "b_single_steps_ms": spread(tb), "c_unet_launches_of_a_ms": spread(tc),
           "a_over_b": round(med(ta) / med(tb), 4), "a_over_c": round(med(ta) / med(tc), 4),
           "a_faster_than_b_by_more_than_bs_spread": bool(med(tb) - med(ta) > max(tb) - min(tb)),
           "kernels": {}}
    for name, nbytes in (("stack_gather", 2 * tile_bytes), ("stack_blend", tile_bytes + scene_bytes), ("scene_stats", scene_bytes + 2 * scene_bytes // B)):
        ms = med(kt[name])
        res["kernels"][name] = {"ms": round(ms, 4), "min_ms": round(min(kt[name]), 4), "bytes": nbytes, "GBps": round(nbytes / ms / 1e6, 1)}
    return res


def stats_streaming(m, dev, reps, B=16, side=2048):
    """eod_scene_stats on a stack that does not fit the 256 MiB Infinity Cache (B x 3 x side x side fp32): its streaming rate"""
    x = m._philox((B, 3, side, side), dev, 3, 0, 0, 0)
    out = torch.empty((2, 3, side, side), dtype=torch.float32, device=dev)
    fn = lambda: scene_stats(x, out=out)
    timed(fn, 3)
    t = [timed(fn, 10) for _ in range(reps)]
    nbytes = (B + 2) * 3 * side * side * 4
    ms = statistics.median(t)
    return {"shape": [B, 3, side, side], "ms": round(ms, 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4), "bytes": nbytes,
            "GBps": round(nbytes / ms / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--width", type=int, default=777)
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--overlap", type=int, default=32)
    ap.add_argument("--scenes", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--tile-batch", type=int, default=16)
    ap.add_argument("--arch", default="A0")
    ap.add_argument("--precision", default="fp32x3")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=7, help="alternations of the arms")
    ap.add_argument("--steps", type=int, default=3, help="steps per timed window")
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scene_stack_bench.py measures on the GPU; there is nothing to time without one")
    dev = torch.device("cuda", 0)
    m = build_model(args.arch, args.tile, args.precision, dev)
    plan = TilePlan(args.height, args.width, args.tile, args.overlap)
    res = {"workload": f"{args.arch} @ {args.tile}x{args.tile} tiles, {args.precision}, scenes {plan.H}x{plan.W}x3, overlap {args.overlap}: "
                       f"{plan.nty} x {plan.ntx} = {plan.n_tiles} tiles per scene, tile_batch {args.tile_batch}, skip_known",
           "reps": args.reps, "steps_per_window": args.steps, "stacks": [one_stack(m, plan, B, args, dev) for B in args.scenes]}
    with torch.no_grad():
        res["scene_stats_streaming"] = stats_streaming(m, dev, args.reps)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
