#!/usr/bin/env python3
"""What whole-scene sampling costs on top of the UNet launches it needs.

One process, the two arms alternating, HIP events around each timed window:
  (a) one `sampling_scene` step (EODiffusion._scene_step: gather -> UNet on chunks of tile_batch tiles -> blend -> scene-level
      eod_ddpm_step) on an H x W scene;
  (b) the same number of UNet launches on PRE-CUT tiles with the per-batch update (`_reverse_diffusion_with_clip` per chunk):
      what a Python loop around `sampling()` does for the same work, minus cutting and stitching.
(a) - (b) is the cost of gather + blend + the chunk copies.  Both arms run the padded last chunk (96 tile slots for 81 tiles at the
defaults: 15.6 % of the UNet work is padding, by construction -- printed separately; `tile_batch` is the user's knob).  The noise
is drawn before the timed windows in both arms.  Also timed on their own: eod_scene_gather, eod_scene_blend (bytes from the
shapes -> GB/s) and the whole tiling overhead with the network replaced by a stub.

    python tools/scene_bench.py [--size 2048] [--tile 256] [--overlap 32] [--tile-batch 16] [--arch A0] [--precision fp32x3] [--reps 7]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bench import build_model  # noqa: E402
from eo_diffusion_amd.tiling import TilePlan, blend_tiles, gather_padded, gather_tiles, tile_slots, tiled_estimate  # noqa: E402


def timed(fn, reps):
    """ms per call of fn over `reps` back-to-back calls (HIP events; fn only enqueues)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048, help="scene is size x size")
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--overlap", type=int, default=32)
    ap.add_argument("--tile-batch", type=int, default=16)
    ap.add_argument("--arch", default="A0")
    ap.add_argument("--precision", default="fp32x3")
    ap.add_argument("--reps", type=int, default=7, help="alternations of the two arms")
    ap.add_argument("--steps", type=int, default=3, help="steps per timed window")
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scene_bench.py measures on the GPU; there is nothing to time without one")
    dev = torch.device("cuda", 0)
    m = build_model(args.arch, args.tile, args.precision, dev)
    plan = TilePlan(args.size, args.size, args.tile, args.overlap)
    chunk, slots = tile_slots(plan, args.tile_batch)
    C, s, i = 3, args.tile, 500
    x_scene = m._philox((1, C, plan.H, plan.W), dev, 1, 0, m.timesteps, 0)
    z_scene = m._philox((1, C, plan.H, plan.W), dev, 1, 0, i, 1)
    x_tiles = gather_padded(x_scene, plan, args.tile_batch).clone()
    z_tiles = gather_padded(z_scene, plan, args.tile_batch).clone()
    t_chunk = torch.full((chunk,), i, dtype=torch.int64, device=dev)

    def arm_scene():
        return m._scene_step(x_scene, i, z_scene, plan, args.tile_batch, True)

    def arm_tiles():
        for lo in range(0, slots, chunk):
            m._reverse_diffusion_with_clip(x_tiles[lo:lo + chunk], t_chunk, z_tiles[lo:lo + chunk])

    def unet_only():
        for lo in range(0, slots, chunk):
            m.model(x_tiles[lo:lo + chunk], t_chunk)

    with torch.no_grad():
        for _ in range(2):  # every shape of the timed windows, both arms
            arm_scene(), arm_tiles(), unet_only()
        torch.cuda.synchronize()
        ta, tb, tu = [], [], []
        for _ in range(args.reps):
            ta.append(timed(arm_scene, args.steps))
            tb.append(timed(arm_tiles, args.steps))
            tu.append(timed(unet_only, args.steps))
        tiles_out = torch.empty((slots, C, s, s), dtype=torch.float32, device=dev)
        scene_out = torch.empty((1, C, plan.H, plan.W), dtype=torch.float32, device=dev)
        e_chunk = x_tiles[:chunk].clone()
        kern = {"gather": lambda: gather_tiles(x_scene, plan, out=tiles_out), "blend": lambda: blend_tiles(x_tiles, plan, out=scene_out),
                "tiling_with_stub_network": lambda: tiled_estimate(x_scene, plan, args.tile_batch, lambda x, lo: e_chunk)}
        kt = {}
        for name, fn in kern.items():
            timed(fn, 5)
            kt[name] = [timed(fn, 50) for _ in range(args.reps)]
    tile_bytes = plan.n_tiles * C * s * s * 4
    scene_bytes = C * plan.H * plan.W * 4
    med = statistics.median
    res = {
        "workload": f"{args.arch} @ {s}x{s} tiles, {args.precision}, scene {plan.H}x{plan.W}x{C}, overlap {args.overlap}: {plan.nty} x {plan.ntx} = "
                    f"{plan.n_tiles} tiles in {slots // chunk} launches of {chunk} ({slots} slots)",
        "padding_share_of_unet_work": round((slots - plan.n_tiles) / slots, 4),
        "reps": args.reps, "steps_per_window": args.steps,
        "a_scene_step_ms": {"median": round(med(ta), 3), "min": round(min(ta), 3), "max": round(max(ta), 3)},
        "b_precut_tiles_step_ms": {"median": round(med(tb), 3), "min": round(min(tb), 3), "max": round(max(tb), 3)},
        "unet_launches_only_ms": {"median": round(med(tu), 3), "min": round(min(tu), 3), "max": round(max(tu), 3)},
        "a_over_b": round(med(ta) / med(tb), 4),
        "a_minus_b_ms": round(med(ta) - med(tb), 3),
        "per_useful_tile_ms": round(med(ta) / plan.n_tiles, 4),
        "kernels": {},
    }
    for name, nbytes in (("gather", 2 * tile_bytes), ("blend", tile_bytes + scene_bytes), ("tiling_with_stub_network", None)):
        ms = med(kt[name])
        res["kernels"][name] = {"ms": round(ms, 4), "min_ms": round(min(kt[name]), 4), "share_of_scene_step": round(ms / med(ta), 5)}
        if nbytes:
            res["kernels"][name].update(bytes=nbytes, GBps=round(nbytes / ms / 1e6, 1))
    res["gather_plus_blend_share_of_scene_step"] = round((med(kt["gather"]) + med(kt["blend"])) / med(ta), 5)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
