#!/usr/bin/env python3
"""What the ensemble statistics cost.

One process, profiler off:
  (1) kernels, HIP events around back-to-back calls, the three alternating on the SAME stack: eod_scene_stats (the yardstick: one pass, mean
      and std), eod_scene_quantiles (Q = 3) and eod_ensemble_stats (L = 2, no map) at B in {8, 16, 64} on B x 3 x 256^2 and, for B <= 16,
      on B x 3 x 2048^2 (805 MB at B = 16: larger than the Infinity Cache).  Byte model from the shapes: all three read the stack once;
      scene_stats writes 2 planes, scene_quantiles Q, ensemble_stats reads the truth: (B + 2), (B + Q), (B + 1) planes.  The ratio to
      eod_scene_stats on the same stack, in the same process, is the figure; the byte model says (B + Q) / (B + 2) for the quantiles;
  (2) tiling.scene_quantiles next to torch.quantile(stack, q, dim=0) on the 256^2 stacks (and the 2048^2 stack at B = 8): host clock around
      calls that end in a synchronise;
  (3) the call: a 25-evaluation sampling_scene(n_scenes=8) with and without scene_quantiles + metrics.ensemble after it, alternating.

    python tools/ensemble_bench.py [--arch A0] [--tile 64] [--side 128] [--reps 3] [--no-call] [--no-large] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bench import build_model  # noqa: E402
from eo_diffusion_amd import _lib, metrics  # noqa: E402
from eo_diffusion_amd.engine import current_stream_ptr, quantile_rank  # noqa: E402
from eo_diffusion_amd.tiling import scene_quantiles  # noqa: E402

Q = (0.05, 0.5, 0.95)
LEVELS = (0.5, 0.9)


def timed(fn, reps):
    """ms per call of fn over `reps` back-to-back calls (HIP events; fn only enqueues)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def kernels(L, dev, gen, B, side, st):
    C, H, W = 3, side, side
    n = C * H * W
    truth = torch.rand((1, C, H, W), device=dev, generator=gen)
    x = (truth + 0.1 * torch.randn((B, C, H, W), device=dev, generator=gen)).clamp(0, 1)
    p = lambda t: t.data_ptr()
    stats = torch.empty((2, C, H, W), device=dev)
    qout = torch.empty((len(Q), C, H, W), device=dev)
    ranks = [quantile_rank(q, B) for q in Q]
    ks = (ctypes.c_int32 * len(Q))(*[k for k, _ in ranks])
    fr = (ctypes.c_float * len(Q))(*[f for _, f in ranks])
    lv = [quantile_rank(v, B) for pl in LEVELS for v in ((1 - pl) / 2, (1 + pl) / 2)]
    lk = (ctypes.c_int32 * len(lv))(*[k for k, _ in lv])
    lf = (ctypes.c_float * len(lv))(*[f for _, f in lv])
    sums = torch.empty(C * 5, dtype=torch.float64, device=dev)
    counts = torch.empty(C * (2 + B + 1 + len(LEVELS)), dtype=torch.int64, device=dev)
    ws = torch.empty(int(L.eod_ensemble_stats_workspace_size(B, C, H, W)), dtype=torch.uint8, device=dev)
    forms = {
        "scene_stats": lambda: L.eod_scene_stats(p(x), p(stats[0]), p(stats[1]), B, n, st),
        "scene_quantiles": lambda: L.eod_scene_quantiles(p(x), p(qout), B, n, ks, fr, len(Q), st),
        "ensemble_stats": lambda: L.eod_ensemble_stats(p(x), p(truth), 0, B, C, H, W, lk, lf, len(LEVELS), p(sums), p(counts), 0, p(ws), ws.numel(), st),
    }
    planes = {"scene_stats": B + 2, "scene_quantiles": B + len(Q), "ensemble_stats": B + 1}
    reps = 50 if B * n < 2 ** 25 else 5
    ts = {form: [] for form in forms}
    for fn in forms.values():
        assert fn() == 0
        timed(fn, 3)
    for _ in range(5):                                                # the three alternate
        for form, fn in forms.items():
            ts[form].append(timed(fn, reps))
    med = statistics.median
    row = {"shape": [B, C, H, W], "stack_bytes": B * n * 4}
    for form, v in ts.items():
        row[form] = {"us": round(med(v) * 1e3, 2), "min_us": round(min(v) * 1e3, 2), "max_us": round(max(v) * 1e3, 2),
                     "GB_per_s": round(planes[form] * n * 4 / (med(v) * 1e-3) / 1e9, 1)}
    base = med(ts["scene_stats"])
    row["yardstick_spread"] = round((max(ts["scene_stats"]) - min(ts["scene_stats"])) / base, 4)
    row["quantiles_over_scene_stats"] = round(med(ts["scene_quantiles"]) / base, 3)
    row["quantiles_byte_model"] = round((B + len(Q)) / (B + 2), 3)
    row["ensemble_stats_over_scene_stats"] = round(med(ts["ensemble_stats"]) / base, 3)
    row["ensemble_stats_byte_model"] = round((B + 1) / (B + 2), 3)
    return row, x


def against_torch(x, reps):
    qt = torch.tensor(Q, device=x.device)
    ours, theirs = lambda: scene_quantiles(x, Q), lambda: torch.quantile(x, qt, dim=0)
    wall(ours), wall(theirs)
    a, b = [], []
    for _ in range(reps):
        dt, o = wall(ours)
        a.append(dt)
        dt, t = wall(theirs)
        b.append(dt)
    med = statistics.median
    return {"scene_quantiles_ms": round(med(a) * 1e3, 3), "torch_quantile_ms": round(med(b) * 1e3, 3), "ratio_torch_over_ours": round(med(b) / med(a), 2),
            "max_abs_difference": float((o - t).abs().max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="A0")
    ap.add_argument("--tile", type=int, default=64)
    ap.add_argument("--side", type=int, default=128, help="side of the sampled scenes of part (3)")
    ap.add_argument("--precision", default="fp32x3")
    ap.add_argument("--reps", type=int, default=3, help="alternations of the two calls")
    ap.add_argument("--no-call", action="store_true", help="kernels and torch.quantile only")
    ap.add_argument("--no-large", action="store_true", help="skip the 2048^2 stacks")
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ensemble_bench.py measures on the GPU; there is nothing to time without one")
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    st = current_stream_ptr(dev)
    gen = torch.Generator(device=dev).manual_seed(7)
    med = statistics.median
    res = {"kernels": {}, "against_torch_quantile": {}}
    with torch.no_grad():
        for side in (256,) if args.no_large else (256, 2048):
            for B in (8, 16, 64):
                if side == 2048 and B > 16:
                    continue
                name = f"B{B}_x3x{side}"
                res["kernels"][name], x = kernels(L, dev, gen, B, side, st)
                if side == 256 or B == 8:
                    res["against_torch_quantile"][name] = against_torch(x, args.reps)
                del x
                torch.cuda.empty_cache()
        if not args.no_call:
            T, n_scenes = 25, 8
            m = build_model(args.arch, args.tile, args.precision, dev, timesteps=T)
            hw = (args.side, args.side)
            truth = torch.rand((1, 3) + hw, device=dev, generator=gen) * 2 - 1
            plain = lambda: m.sampling_scene(hw, True, dev, overlap=args.tile // 4, seed=3, progress=False, n_scenes=n_scenes)

            def scored():
                out = plain()
                return scene_quantiles(out, Q), metrics.ensemble(out, truth, levels=LEVELS)

            wall(plain), wall(scored)                                 # warm-up: plan build, the shapes of both calls
            t0, t1 = [], []
            for _ in range(args.reps):
                t0.append(wall(plain)[0])
                dt, (qs, e) = wall(scored)
                t1.append(dt)
            res["call"] = {
                "workload": f"{args.arch} @ {args.tile}x{args.tile} tiles, {args.precision}: sampling_scene of {n_scenes} draws of a {hw[0]}x{hw[1]}x3 scene, "
                            f"T = {T} ({T} evaluations), alone against followed by scene_quantiles(Q = 3) + metrics.ensemble(levels = (0.5, 0.9))",
                "sample_s": {"median": round(med(t0), 4), "min": round(min(t0), 4), "max": round(max(t0), 4)},
                "sample_and_statistics_s": {"median": round(med(t1), 4), "min": round(min(t1), 4), "max": round(max(t1), 4)},
                "sample_spread": round((max(t0) - min(t0)) / med(t0), 4),
                "ratio": round(med(t1) / med(t0), 4),
                "extra_ms": round((med(t1) - med(t0)) * 1e3, 3),
                "finite": bool(torch.isfinite(qs).all()) and bool((e.crps == e.crps).all()),
            }
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
