#!/usr/bin/env python3
"""What skip_known saves on a scene whose RePaint mask touches a few tiles.

One process, the arms alternating, HIP events around each timed window (the method of tools/scene_bench.py):
  (a)  the full scene step: EODiffusion._scene_step on the TilePlan (mix -> gather -> UNet on every tile -> blend -> update);
  (au) the UNet launches of (a) alone;
  (b)  the skipping step: the same call on the TileSubset of the active tiles;
  (c)  the UNet launches of (b) alone, at (b)'s chunk size.
(b) / (a) is what a user saves per step; it should approach (c) / (au).  (b) - (c) is the skipping step's overhead over its launches
(mix, gather of the list, blend of the list, update, chunk copies), to be read next to (a) - (au), the full step's own overhead, and
against the run-to-run spread of the arms, which is printed with them.  The noise is drawn before the timed windows.
Optional: --call  one complete call (T = 250, resample=(10, 10)) on a smaller scene with and without skip_known, host clock, after a
warm-up call on a short chain that builds the same launch programs;  --big N  one skipping step on an N x N scene (10980: a
Sentinel-2 granule) with its scene-level passes timed one by one.

    python tools/scene_skip_bench.py [--size 2048] [--tile 256] [--overlap 32] [--tile-batch 16] [--arch A0] [--precision fp32x3]
                                     [--reps 7] [--call] [--big 10980] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import build_model  # noqa: E402
from eo_diffusion_amd.tiling import TilePlan, active_tiles, blend_tiles, gather_padded, gather_tiles, keep_known, tile_slots  # noqa: E402


def timed(fn, reps):
    """ms per call of fn over `reps` back-to-back calls (HIP events; fn only enqueues)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def blob_mask(H, W, blobs, dev):
    """[1, 1, H, W]: 1 = known, 0 inside the discs (cy, cx, r) given as fractions of the scene"""
    yy = torch.arange(H, device=dev, dtype=torch.float32)[:, None]
    xx = torch.arange(W, device=dev, dtype=torch.float32)[None, :]
    m = torch.ones((H, W), dtype=torch.float32, device=dev)
    for cy, cx, r in blobs:
        m[(yy - cy * H) ** 2 + (xx - cx * W) ** 2 <= (r * min(H, W)) ** 2] = 0.0
    return m[None, None].contiguous()


def stats(v):
    med = statistics.median(v)
    return {"median": round(med, 3), "min": round(min(v), 3), "max": round(max(v), 3), "spread_pct": round(100 * (max(v) - min(v)) / med, 2)}


def step_arms(m, plan, sub, tile_batch, gt, mask, x, z, i, reps, steps):
    dev = x.device
    tiles_of = {"full": plan, "skip": sub}
    unet_in = {}
    for name, p in tiles_of.items():
        chunk, slots = tile_slots(p, tile_batch)
        unet_in[name] = (gather_padded(x, p, tile_batch).clone(), torch.full((chunk,), i, dtype=torch.int64, device=dev), chunk, slots)

    def scene(name):
        return lambda: m._scene_step(x, i, z, tiles_of[name], tile_batch, True, gt, mask)

    def unet(name):
        tiles, t, chunk, slots = unet_in[name]

        def run():
            for lo in range(0, slots, chunk):
                m.model(tiles[lo:lo + chunk], t)
        return run

    arms = {"a_full_step": scene("full"), "au_full_unet_only": unet("full"), "b_skip_step": scene("skip"), "c_skip_unet_only": unet("skip")}
    for _ in range(2):  # every shape of the timed windows (the launch program of the smaller batch is built here)
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            t[k].append(timed(fn, steps))
    return t, {k: (v[2], v[3]) for k, v in unet_in.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048, help="scene is size x size")
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--overlap", type=int, default=32)
    ap.add_argument("--tile-batch", type=int, default=16)
    ap.add_argument("--arch", default="A0")
    ap.add_argument("--precision", default="fp32x3")
    ap.add_argument("--reps", type=int, default=7, help="alternations of the arms")
    ap.add_argument("--steps", type=int, default=3, help="steps per timed window")
    ap.add_argument("--call", action="store_true", help="also one complete resampled call with and without skip_known")
    ap.add_argument("--call-size", type=int, default=1024)
    ap.add_argument("--big", type=int, default=0, help="also one skipping step on a scene of this size (10980: Sentinel-2)")
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scene_skip_bench.py measures on the GPU; there is nothing to time without one")
    dev = torch.device("cuda", 0)
    m = build_model(args.arch, args.tile, args.precision, dev)
    C, s, i = 3, args.tile, 500
    blobs = [(0.16, 0.17, 0.05), (0.55, 0.60, 0.07), (0.86, 0.30, 0.03)]  # three clouds
    med = statistics.median
    res = {}
    with torch.no_grad():
        plan = TilePlan(args.size, args.size, s, args.overlap)
        mask = blob_mask(plan.H, plan.W, blobs, dev)
        act = active_tiles(mask, plan)
        assert np.array_equal(act, plan.active_tiles(mask.cpu().numpy()))
        sub = plan.subset(act)
        gt = m._philox((1, C, plan.H, plan.W), dev, 2, 0, 0, 0).clamp_(-1, 1)
        x = m._philox((1, C, plan.H, plan.W), dev, 1, 0, m.timesteps, 0)
        z = m._philox((1, C, plan.H, plan.W), dev, 1, 0, i, 1)
        t, shapes = step_arms(m, plan, sub, args.tile_batch, gt, mask, x, z, i, args.reps, args.steps)
        # the kernels of the skipping path on their own
        compact = gather_tiles(x, sub).clone()
        scene_out = torch.empty_like(x)
        kern = {"tile_active": lambda: active_tiles(mask, plan),  # (includes its device-to-host copy: once per call)
                "gather_list": lambda: gather_tiles(x, sub, out=compact), "blend_list": lambda: blend_tiles(compact, sub, out=scene_out),
                "keep_known": lambda: keep_known(x, gt, sub, out=scene_out)}
        kt = {}
        for name, fn in kern.items():
            timed(fn, 5)
            kt[name] = [timed(fn, 50) for _ in range(args.reps)]
        a, au, b, c = (med(t[k]) for k in ("a_full_step", "au_full_unet_only", "b_skip_step", "c_skip_unet_only"))
        res = {
            "workload": f"{args.arch} @ {s}x{s} tiles, {args.precision}, scene {plan.H}x{plan.W}x{C}, overlap {args.overlap}: {plan.n_tiles} tiles in "
                        f"{shapes['full'][1] // shapes['full'][0]} launches of {shapes['full'][0]}; mask of {len(blobs)} discs, "
                        f"{float((mask != 1).float().mean()) * 100:.2f} % hole: {sub.n_tiles} active tiles in "
                        f"{shapes['skip'][1] // shapes['skip'][0]} launches of {shapes['skip'][0]}",
            "active_tiles": act.tolist(), "estimated_share_of_scene": round(float(sub.estimated().mean()), 4),
            "reps": args.reps, "steps_per_window": args.steps,
            **{k + "_ms": stats(v) for k, v in t.items()},
            "b_over_a": round(b / a, 4), "c_over_au": round(c / au, 4),
            "a_minus_au_ms": round(a - au, 3), "b_minus_c_ms": round(b - c, 3),
            "kernels_ms": {k: {"median": round(med(v), 4), "min": round(min(v), 4)} for k, v in kt.items()},
        }
        del x, z, gt, mask, compact, scene_out
        if args.call:
            res["call"] = whole_call(m, args, blobs, dev)
        if args.big:
            res["big"] = big_step(m, args, dev)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def whole_call(m, args, blobs, dev):
    """T = 250, resample=(10, 10): seconds of a complete call, full and skipping, host clock around a synchronised call"""
    from eo_diffusion_amd.diffusion.model import EODiffusion
    from eo_diffusion_amd.diffusion.util import make_resample_schedule
    s, n = args.tile, args.call_size
    plan = TilePlan(n, n, s, args.overlap)
    mask = blob_mask(n, n, blobs[:2], dev)
    gt = m._philox((1, 3, n, n), dev, 3, 0, 0, 0).clamp_(-1, 1)
    cond = torch.cat([gt, mask], 1)
    n_active = int(active_tiles(mask, plan).size)
    out = {"scene": f"{n}x{n}, {plan.n_tiles} tiles, {n_active} active", "T": 250, "resample": [10, 10],
           "evaluations": len(make_resample_schedule(250, 10, 10)[0])}
    warm = EODiffusion(m.model, timesteps=4, image_size=s, in_channels=3, cond_type="sum", device=str(dev)).to(dev).eval()
    full = EODiffusion(m.model, timesteps=250, image_size=s, in_channels=3, cond_type="sum", device=str(dev)).to(dev).eval()
    got = {}
    for name, skip in (("full", False), ("skip_known", True)):
        kw = dict(cond=cond, overlap=args.overlap, tile_batch=args.tile_batch, seed=7, progress=False, skip_known=skip)
        warm.sampling_scene((n, n), True, dev, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got[name] = full.sampling_scene((n, n), True, dev, resample=(10, 10), **kw)
        torch.cuda.synchronize()
        out[name + "_s"] = round(time.perf_counter() - t0, 3)
    est = torch.from_numpy(plan.subset(active_tiles(mask, plan)).estimated()).to(dev)[None, None].expand_as(gt)
    out["skip_over_full"] = round(out["skip_known_s"] / out["full_s"], 4)
    out["bit_equal_at_estimated_pixels"] = bool(torch.equal(got["full"][est], got["skip_known"][est]))
    out["known_image_elsewhere"] = bool(torch.equal(got["skip_known"][~est], gt[~est]))
    return out


def big_step(m, args, dev):
    """one skipping step on a --big x --big scene, and its scene-level passes one by one (each: median of 5 windows of 3 calls)"""
    s, n, i = args.tile, args.big, 500
    plan = TilePlan(n, n, s, args.overlap)
    mask = blob_mask(n, n, [(0.31, 0.42, 0.02), (0.70, 0.66, 0.012)], dev)
    sub = plan.subset(active_tiles(mask, plan))
    shape = (1, 3, n, n)
    gt = m._philox(shape, dev, 4, 0, 0, 0).clamp_(-1, 1)
    x = m._philox(shape, dev, 1, 0, m.timesteps, 0)
    z = m._philox(shape, dev, 1, 0, i, 1)
    chunk, slots = tile_slots(sub, args.tile_batch)
    tiles = gather_padded(x, sub, args.tile_batch).clone()
    t1 = torch.full((1,), i, dtype=torch.int64, device=dev)
    tc = torch.full((chunk,), i, dtype=torch.int64, device=dev)
    compact = tiles[:sub.n_tiles]
    scene_out = torch.empty_like(x)

    def unet():
        for lo in range(0, slots, chunk):
            m.model(tiles[lo:lo + chunk], tc)

    passes = {
        "skip_step": lambda: m._scene_step(x, i, z, sub, args.tile_batch, True, gt, mask),
        "unet_only": unet,
        "philox_noise": lambda: m._philox(shape, dev, 1, 0, i, 1),
        "repaint_mix": lambda: m._repaint_mix(x, gt, mask, t1, z),
        "gather_list": lambda: gather_tiles(x, sub, out=tiles),
        "blend_list": lambda: blend_tiles(compact, sub, out=scene_out),
        "ddpm_update": lambda: m._ddpm_update(x, scene_out, z, t1, True),
        "keep_known": lambda: keep_known(x, gt, sub, out=scene_out),
    }
    out = {"scene": f"{n}x{n}x3 ({3 * n * n * 4 / 1e9:.2f} GB per tensor), {plan.nty} x {plan.ntx} = {plan.n_tiles} tiles, {sub.n_tiles} active in "
                    f"{slots // chunk} launches of {chunk}"}
    for name, fn in passes.items():
        fn()
        torch.cuda.synchronize()
        v = [timed(fn, 3) for _ in range(5)]
        out[name + "_ms"] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    out["scene_passes_share_of_step"] = round(1.0 - out["unet_only_ms"]["median"] / out["skip_step_ms"]["median"], 4)
    return out


if __name__ == "__main__":
    main()
