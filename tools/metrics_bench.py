#!/usr/bin/env python3
"""What scoring a result costs.

One process, profiler off:
  (1) kernels, HIP events around back-to-back calls, the two operators alternating: eod_band_stats and eod_ssim (11 taps, no map) at
      16 x 3 x 256^2 and 1 x 13 x 2048^2.  Byte model from the shapes: both images read once, 2 * B * C * H * W * 4 bytes (the tables
      and the workspace are three orders smaller); GB/s is that over the time -- eod_ssim is arithmetic in float64, the figure says how
      far from a streaming pass it is, not a share of any peak;
  (2) the evaluation: metrics.quality() (both operators, one copy of the tables, the host arithmetic) next to harness.ssim (device-to-host
      copy, numpy) at 16 x 3 x 256^2 -- the host path at that size only -- host clock around calls that end in a synchronise;
  (3) the call: a 25-evaluation DPMSolverSampler.sample with and without a quality() call after it, alternating.

    python tools/metrics_bench.py [--arch A0] [--size 64] [--batch 16] [--steps 25] [--reps 3] [--no-call] [--out FILE]
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
from eo_diffusion_amd import _lib, harness, metrics  # noqa: E402
from eo_diffusion_amd.engine import current_stream_ptr  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="A0")
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--precision", default="fp32x3")
    ap.add_argument("--timesteps", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=25, help="S of the DPM-Solver++ call")
    ap.add_argument("--reps", type=int, default=3, help="alternations of the two calls")
    ap.add_argument("--no-call", action="store_true", help="kernels and the evaluation only")
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench.py measures on the GPU; there is nothing to time without one")
    dev = torch.device("cuda", 0)
    med = statistics.median
    L = _lib.lib()
    st = current_stream_ptr(dev)
    p = lambda t: t.data_ptr()
    taps = metrics.gauss_window(11, 1.5)
    tp = taps.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    gen = torch.Generator(device=dev).manual_seed(7)
    res = {"kernels": {}}
    with torch.no_grad():
        for name, shape in (("batch_256", (16, 3, 256, 256)), ("scene_2048", (1, 13, 2048, 2048))):
            B, C, H, W = shape
            t = torch.rand(shape, device=dev, generator=gen)
            x = (t + 0.05 * torch.randn(shape, device=dev, generator=gen)).clamp(0, 1)
            band = torch.empty(B * C * 8, dtype=torch.float64, device=dev)
            sample = torch.empty(B * 3, dtype=torch.float64, device=dev)
            sums = torch.empty(B * C * 2, dtype=torch.float64, device=dev)
            ws1 = torch.empty(int(L.eod_band_stats_workspace_size(B, C, H, W)), dtype=torch.uint8, device=dev)
            ws2 = torch.empty(int(L.eod_ssim_workspace_size(B, C, H, W, 5)), dtype=torch.uint8, device=dev)
            forms = {
                "band_stats": lambda: L.eod_band_stats(p(x), p(t), 0, B, B, 1, C, H, W, 1.0, 0.0, p(band), p(sample), p(ws1), ws1.numel(), st),
                "ssim": lambda: L.eod_ssim(p(x), p(t), 0, B, B, 1, C, H, W, tp, 5, 1.0, 0.0, 1e-4, 9e-4, 0, p(sums), p(ws2), ws2.numel(), st),
            }
            ts = {form: [] for form in forms}
            reps = 50 if B * C * H * W < 2 ** 24 else 10
            for fn in forms.values():
                assert fn() == 0
                timed(fn, 5)
            for _ in range(5):                                        # the two alternate
                for form, fn in forms.items():
                    ts[form].append(timed(fn, reps))
            nbytes = 2 * B * C * H * W * 4
            row = {"shape": list(shape), "bytes": nbytes, "workspace_bytes": {"band_stats": ws1.numel(), "ssim": ws2.numel()}}
            for form, v in ts.items():
                row[form] = {"us": round(med(v) * 1e3, 2), "min_us": round(min(v) * 1e3, 2), "max_us": round(max(v) * 1e3, 2),
                             "GB_per_s": round(nbytes / (med(v) * 1e-3) / 1e9, 1)}
            row["ssim_ns_per_output_pixel"] = round(med(ts["ssim"]) * 1e6 / (B * C * (H - 10) * (W - 10)), 4)
            res["kernels"][name] = row
            if name == "batch_256":
                wall(lambda: metrics.quality(x, t)), wall(lambda: harness.ssim(x, t))
                tq, th = [], []
                for _ in range(args.reps):
                    dt, q = wall(lambda: metrics.quality(x, t))
                    tq.append(dt)
                    dt, hs = wall(lambda: harness.ssim(x, t))
                    th.append(dt)
                res["evaluation_batch_256"] = {
                    "quality_s": {"median": round(med(tq), 5), "min": round(min(tq), 5), "max": round(max(tq), 5)},
                    "harness_ssim_s": {"median": round(med(th), 4), "min": round(min(th), 4), "max": round(max(th), 4)},
                    "ratio_harness_over_quality": round(med(th) / med(tq), 1),
                    "ssim_difference": abs(float(q.ssim_all.mean()) - hs),
                }
        if not args.no_call:
            from eo_diffusion_amd.diffusion.dpm_solver import DPMSolverSampler
            m = build_model(args.arch, args.size, args.precision, dev, timesteps=args.timesteps)
            shape = (3, args.size, args.size)
            x_T = m._philox((args.batch,) + shape, dev, 1, 0, args.timesteps, 0)
            truth = torch.rand((1,) + shape, device=dev, generator=gen) * 2 - 1
            dpm = DPMSolverSampler(m)
            plain = lambda: dpm.sample(args.steps, args.batch, shape, x_T=x_T, clip_denoised=True, progress=False)[0]

            def scored():
                out = plain()
                return metrics.quality(out, truth, affine=(0.5, 0.5), ratio=2)

            wall(plain), wall(scored)                                 # warm-up: plan build, the shapes of both calls
            t0, t1 = [], []
            for _ in range(args.reps):
                t0.append(wall(plain)[0])
                dt, q = wall(scored)
                t1.append(dt)
            res["call"] = {
                "workload": f"{args.arch} @ {args.size}x{args.size}, batch {args.batch}, {args.precision}, T = {args.timesteps}: DPM-Solver++ 2M, "
                            f"S = {args.steps} ({dpm.num_evaluations} evaluations), alone against followed by quality(affine=(0.5, 0.5), ratio=2)",
                "sample_s": {"median": round(med(t0), 4), "min": round(min(t0), 4), "max": round(max(t0), 4)},
                "sample_and_quality_s": {"median": round(med(t1), 4), "min": round(min(t1), 4), "max": round(max(t1), 4)},
                "sample_spread": round((max(t0) - min(t0)) / med(t0), 4),
                "ratio": round(med(t1) / med(t0), 4),
                "extra_ms": round((med(t1) - med(t0)) * 1e3, 3),
                "finite": bool(torch.isfinite(torch.from_numpy(q.rmse)).all()),
            }
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
