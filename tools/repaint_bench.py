#!/usr/bin/env python3
"""What RePaint resampling costs on top of the UNet evaluations it asks for.

One process:
  (1) kernels, HIP events around back-to-back launches: eod_renoise with given noise, eod_renoise with the noise generated in
      registers, and the pair the latter replaces (eod_randn_philox writing z + eod_renoise reading it), at the batch shape of the
      call below and at a scene-sized tensor (1 x 3 x 2048 x 2048);
  (2) the call: `sampling(batch, rng="philox", resample=(L, U))` timed by a host clock around a call that ends in a synchronise,
      after a warm-up call, next to  len(visits) x  the per-step time of a plain `sampling()` of the same model, the two alternating.
      The ratio is the cost of the jumps (launches + host work of the walk) relative to the evaluations alone; the spread of the
      plain call's per-step time says what the ratio can resolve.

    python tools/repaint_bench.py [--arch A0] [--size 64] [--batch 16] [--timesteps 250] [--resample 10 10] [--reps 3] [--no-call]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/repaint_bench.py --reps 1 --shapes     (the call alone)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/repaint_bench.py --no-call --shapes scene
(runs of their own: the statistics are per kernel NAME, so one tensor shape per traced run)
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
from eo_diffusion_amd.diffusion.util import make_resample_schedule  # noqa: E402


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
    ap.add_argument("--timesteps", type=int, default=250)
    ap.add_argument("--resample", type=int, nargs=2, default=[10, 10], metavar=("L", "U"))
    ap.add_argument("--reps", type=int, default=3, help="alternations of the plain and the resampled call")
    ap.add_argument("--no-call", action="store_true", help="kernels only")
    ap.add_argument("--shapes", nargs="*", default=["batch", "scene"], choices=["batch", "scene"], help="tensors of the kernel timings (none: the call only)")
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("repaint_bench.py measures on the GPU; there is nothing to time without one")
    dev = torch.device("cuda", 0)
    m = build_model(args.arch, args.size, args.precision, dev, timesteps=args.timesteps)
    med = statistics.median
    res = {"kernels": {}}
    with torch.no_grad():
        for name, shape in (("batch", (args.batch, 3, args.size, args.size)), ("scene", (1, 3, 2048, 2048))):
            if name not in args.shapes:
                continue
            x = m._philox(shape, dev, 1, 0, 7, 0)
            z = m._philox(shape, dev, 1, 0, 7, 1)
            forms = {"renoise_given_noise": lambda: m._renoise(x, 0.9, 0.3, z),
                     "renoise_philox": lambda: m._renoise(x, 0.9, 0.3, key=(1, 0, 7, 2)),
                     "randn_philox_then_renoise": lambda: m._renoise(x, 0.9, 0.3, m._philox(shape, dev, 1, 0, 7, 2))}
            nbytes = x.numel() * 4
            row = {"shape": list(shape)}
            for form, fn in forms.items():
                timed(fn, 10)
                ts = [timed(fn, 200) for _ in range(5)]
                row[form] = {"us": round(med(ts) * 1e3, 2), "min_us": round(min(ts) * 1e3, 2), "max_us": round(max(ts) * 1e3, 2)}
            row["bytes"] = {"renoise_given_noise": 3 * nbytes, "renoise_philox": 2 * nbytes, "randn_philox_then_renoise": 4 * nbytes}
            res["kernels"][name] = row
        if not args.no_call:
            L, U = args.resample
            visits, jumps = make_resample_schedule(args.timesteps, L, U)
            plain = lambda: m.sampling(args.batch, device="cuda:0", rng="philox", seed=7, progress=False)
            resampled = lambda: m.sampling(args.batch, device="cuda:0", rng="philox", seed=7, progress=False, resample=(L, U))

            def wall(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                return time.perf_counter() - t0, out

            wall(plain)                                               # warm-up: plan build, every shape of both calls
            tp, tr = [], []
            for _ in range(args.reps):
                tp.append(wall(plain)[0] / args.timesteps * 1e3)
                dt, out = wall(resampled)
                tr.append(dt)
            per_step, call = med(tp), med(tr)
            res["call"] = {
                "workload": f"{args.arch} @ {args.size}x{args.size}, batch {args.batch}, {args.precision}, T = {args.timesteps}, resample = ({L}, {U}): "
                            f"{len(visits)} evaluations, {len(jumps)} jumps",
                "plain_ms_per_step": {"median": round(per_step, 4), "min": round(min(tp), 4), "max": round(max(tp), 4)},
                "plain_spread": round((max(tp) - min(tp)) / per_step, 4),
                "resampled_call_s": {"median": round(call, 4), "min": round(min(tr), 4), "max": round(max(tr), 4)},
                "evaluations_x_plain_step_s": round(len(visits) * per_step / 1e3, 4),
                "ratio": round(call / (len(visits) * per_step / 1e3), 4),
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
