#!/usr/bin/env python3
"""What dynamic thresholding costs.

One process, profiler off, the arms alternating:
  (1) kernels, HIP events around back-to-back calls: eod_dyn_threshold (one clear, four reading passes, the apply pass) next to
      eod_pred_x0 (two reads, one write) on the same tensor, at 16 x 3 x 64^2, 16 x 3 x 256^2 and 1 x 4 x 2048^2, on three inputs:
      2.5 * N(0, 1), a constant tensor and a tensor already clamped to +-1.  Byte model: R = 4 reading passes + one read-write pass = 6
      tensors moved against 3, ratio 2; on the 64^2 batch it is the launch count (6 against 1).  A constant or clamped input several
      times slower than the Gaussian one would mean the histogram serialises on one counter;
  (2) the call: a 25-evaluation DPMSolverSampler.sample with and without threshold=DynamicThreshold(), host clock around a call that ends
      in a synchronise, after a warm-up call, the two alternating.

    python tools/threshold_bench.py [--arch A0] [--size 64] [--batch 16] [--steps 25] [--reps 3] [--no-call] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bench import build_model  # noqa: E402
from eo_diffusion_amd import _lib  # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="A0")
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--precision", default="fp32x3")
    ap.add_argument("--timesteps", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=25, help="S of the DPM-Solver++ call")
    ap.add_argument("--quantile", type=float, default=0.995)
    ap.add_argument("--reps", type=int, default=3, help="alternations of the two calls")
    ap.add_argument("--no-call", action="store_true", help="kernels only")
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("threshold_bench.py measures on the GPU; there is nothing to time without one")
    from eo_diffusion_amd.diffusion.dpm_solver import DPMSolverSampler
    from eo_diffusion_amd.diffusion.threshold import DynamicThreshold
    dev = torch.device("cuda", 0)
    m = build_model(args.arch, args.size, args.precision, dev, timesteps=args.timesteps)
    med = statistics.median
    L = _lib.lib()
    thr = DynamicThreshold(args.quantile)
    res = {"kernels": {}, "quantile": args.quantile}
    st = current_stream_ptr(dev)
    p = lambda t: t.data_ptr()
    with torch.no_grad():
        for name, shape in (("batch_64", (16, 3, 64, 64)), ("batch_256", (16, 3, 256, 256)), ("scene_2048", (1, 4, 2048, 2048))):
            B, n = shape[0], shape[1] * shape[2] * shape[3]
            k, frac = thr.rank(n)
            g = m._philox(shape, dev, 1, 0, 7, 0) * 2.5
            e = m._philox(shape, dev, 1, 0, 7, 1)
            inputs = {"gaussian_2.5": g, "constant": torch.full_like(g, 1.75), "clamped": g.clamp(-1, 1)}
            out, s = torch.empty_like(g), torch.empty(B, device=dev)
            ws = torch.empty(int(L.eod_dyn_threshold_workspace_size(B, n)), dtype=torch.uint8, device=dev)
            forms = {"pred_x0": lambda: L.eod_pred_x0(p(g), p(e), 0.37, 0.63 ** 0.5, 1, p(out), g.numel(), st)}
            for iname, x in inputs.items():
                forms["dyn_threshold_" + iname] = lambda x=x: L.eod_dyn_threshold(p(x), k, frac, float("inf"), p(out), p(s), B, n, p(ws), ws.numel(), st)
            ts = {form: [] for form in forms}
            reps = 200 if n * B < 2 ** 22 else 50
            for fn in forms.values():
                assert fn() == 0
                timed(fn, 10)
            for _ in range(5):                                        # the arms alternate
                for form, fn in forms.items():
                    ts[form].append(timed(fn, reps))
            nbytes = g.numel() * 4
            row = {"shape": list(shape), "bytes": {"pred_x0": 3 * nbytes, "dyn_threshold": 6 * nbytes}, "launches": {"pred_x0": 1, "dyn_threshold": 6}}
            for form, t in ts.items():
                moved = row["bytes"]["pred_x0" if form == "pred_x0" else "dyn_threshold"]
                row[form] = {"us": round(med(t) * 1e3, 2), "min_us": round(min(t) * 1e3, 2), "max_us": round(max(t) * 1e3, 2),
                             "GB_per_s": round(moved / (med(t) * 1e-3) / 1e9, 1)}
            for iname in inputs:
                row[f"ratio_{iname}_over_pred_x0"] = round(med(ts["dyn_threshold_" + iname]) / med(ts["pred_x0"]), 3)
                row[f"ratio_{iname}_over_gaussian"] = round(med(ts["dyn_threshold_" + iname]) / med(ts["dyn_threshold_gaussian_2.5"]), 3)
            res["kernels"][name] = row
        if not args.no_call:
            shape = (3, args.size, args.size)
            x_T = m._philox((args.batch,) + shape, dev, 1, 0, args.timesteps, 0)
            dpm = DPMSolverSampler(m)
            plain = lambda: dpm.sample(args.steps, args.batch, shape, x_T=x_T, clip_denoised=True, progress=False)[0]
            thresholded = lambda: dpm.sample(args.steps, args.batch, shape, x_T=x_T, progress=False, threshold=thr)[0]

            def wall(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                return time.perf_counter() - t0, out

            wall(plain), wall(thresholded)                            # warm-up: plan build, the shapes of both calls
            tp, tt = [], []
            for _ in range(args.reps):
                tp.append(wall(plain)[0])
                dt, out = wall(thresholded)
                tt.append(dt)
            res["call"] = {
                "workload": f"{args.arch} @ {args.size}x{args.size}, batch {args.batch}, {args.precision}, T = {args.timesteps}: DPM-Solver++ 2M, "
                            f"logsnr, S = {args.steps} ({dpm.num_evaluations} evaluations), clip_denoised=True against threshold={thr!r}",
                "clamped_call_s": {"median": round(med(tp), 4), "min": round(min(tp), 4), "max": round(max(tp), 4)},
                "thresholded_call_s": {"median": round(med(tt), 4), "min": round(min(tt), 4), "max": round(max(tt), 4)},
                "clamped_spread": round((max(tp) - min(tp)) / med(tp), 4),
                "ratio": round(med(tt) / med(tp), 4),
                "extra_us_per_evaluation": round((med(tt) - med(tp)) / dpm.num_evaluations * 1e6, 1),
                "last_scale_max": float(thr.last_bound.last_scale.max()),
                "range": [float(out.min()), float(out.max())],
                "finite": bool(torch.isfinite(out).all()),
            }
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
