#!/usr/bin/env python3
"""What a DPM-Solver++ (2M) call costs next to the DDIM call it replaces.

One process, profiler off, the arms alternating:
  (1) kernels, HIP events around back-to-back launches: eod_dpmpp_step at first order (4 tensors moved) and at second order (5) next
      to eod_ddim_step without eta noise (4), at the batch shape of the call below and at a scene-sized tensor (1 x 3 x 2048 x 2048).
      Expectation: the byte ratio, 1 at first order and 5 / 4 at second;
  (2) the call: `DPMSolverSampler.sample(S)` timed by a host clock around a call that ends in a synchronise, after a warm-up call,
      next to  num_evaluations x  the per-step time of a plain `DDIMSampler.sample(250)` of the same model and shape, the two
      alternating.  The ratio is the cost of the solver's host work and its one kernel per step relative to the evaluations alone;
      the spread of the DDIM call's per-step time says what the ratio can resolve.

    python tools/dpm_bench.py [--arch A0] [--size 64] [--batch 16] [--steps 25] [--ddim-steps 250] [--reps 3] [--no-call] [--out FILE]
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
    ap.add_argument("--ddim-steps", type=int, default=250, help="S of the DDIM call it is priced against")
    ap.add_argument("--reps", type=int, default=3, help="alternations of the two calls")
    ap.add_argument("--no-call", action="store_true", help="kernels only")
    ap.add_argument("--shapes", nargs="*", default=["batch", "scene"], choices=["batch", "scene"])
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dpm_bench.py measures on the GPU; there is nothing to time without one")
    from eo_diffusion_amd.diffusion.ddim import DDIMSampler
    from eo_diffusion_amd.diffusion.dpm_solver import DPMSolverSampler
    from eo_diffusion_amd.diffusion.util import dpm_coefficients
    dev = torch.device("cuda", 0)
    m = build_model(args.arch, args.size, args.precision, dev, timesteps=args.timesteps)
    med = statistics.median
    L = _lib.lib()
    res = {"kernels": {}}
    with torch.no_grad():
        for name, shape in (("batch", (args.batch, 3, args.size, args.size)), ("scene", (1, 3, 2048, 2048))):
            if name not in args.shapes:
                continue
            x, e, d = (m._philox(shape, dev, 1, 0, 7, k) for k in range(3))
            o1, o2 = torch.empty_like(x), torch.empty_like(x)
            a_s, a_t = 0.37, 0.61
            s1m = (1.0 - a_s) ** 0.5
            c = [float(v) for v in dpm_coefficients(a_s, a_t, 0.4, 2)]
            st = current_stream_ptr(dev)
            p = lambda t: t.data_ptr()
            forms = {
                "ddim_step": lambda: L.eod_ddim_step(p(x), p(e), 0, a_s, a_t, 0.0, s1m, 1.0, p(o1), p(o2), x.numel(), st),
                "dpmpp_step_first_order": lambda: L.eod_dpmpp_step(p(x), p(e), 0, a_s, s1m, *c, 0, p(o1), p(o2), x.numel(), st),
                "dpmpp_step_second_order": lambda: L.eod_dpmpp_step(p(x), p(e), p(d), a_s, s1m, *c, 0, p(o1), p(o2), x.numel(), st),
            }
            ts = {form: [] for form in forms}
            for fn in forms.values():
                assert fn() == 0
                timed(fn, 10)
            for _ in range(5):                                        # the arms alternate
                for form, fn in forms.items():
                    ts[form].append(timed(fn, 200))
            nbytes = x.numel() * 4
            row = {"shape": list(shape), "bytes": {"ddim_step": 4 * nbytes, "dpmpp_step_first_order": 4 * nbytes, "dpmpp_step_second_order": 5 * nbytes}}
            for form, t in ts.items():
                row[form] = {"us": round(med(t) * 1e3, 2), "min_us": round(min(t) * 1e3, 2), "max_us": round(max(t) * 1e3, 2),
                             "GB_per_s": round(row["bytes"][form] / (med(t) * 1e-3) / 1e9, 1)}
            row["ratio_first_order_over_ddim"] = round(med(ts["dpmpp_step_first_order"]) / med(ts["ddim_step"]), 3)
            row["ratio_second_order_over_ddim"] = round(med(ts["dpmpp_step_second_order"]) / med(ts["ddim_step"]), 3)
            res["kernels"][name] = row
        if not args.no_call:
            shape = (3, args.size, args.size)
            x_T = m._philox((args.batch,) + shape, dev, 1, 0, args.timesteps, 0)
            ddim, dpm = DDIMSampler(m), DPMSolverSampler(m)
            plain = lambda: ddim.sample(args.ddim_steps, args.batch, shape, eta=0.0, x_T=x_T, verbose=False, progress=False)[0]
            solver = lambda: dpm.sample(args.steps, args.batch, shape, x_T=x_T, progress=False)[0]

            def wall(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                return time.perf_counter() - t0, out

            wall(solver)                                              # warm-up: plan build, the shapes of both calls
            tp, tr = [], []
            for _ in range(args.reps):
                dt, _ = wall(plain)
                n_ddim = len(ddim.ddim_timesteps)
                tp.append(dt / n_ddim * 1e3)
                dt, out = wall(solver)
                tr.append(dt)
            n = dpm.num_evaluations
            per_step, call = med(tp), med(tr)
            res["call"] = {
                "workload": f"{args.arch} @ {args.size}x{args.size}, batch {args.batch}, {args.precision}, T = {args.timesteps}: DPM-Solver++ 2M, logsnr, "
                            f"S = {args.steps} ({n} evaluations) against DDIM eta 0, S = {args.ddim_steps} ({n_ddim} evaluations)",
                "ddim_ms_per_step": {"median": round(per_step, 4), "min": round(min(tp), 4), "max": round(max(tp), 4)},
                "ddim_spread": round((max(tp) - min(tp)) / per_step, 4),
                "ddim_call_s": round(per_step * n_ddim / 1e3, 4),
                "dpm_call_s": {"median": round(call, 4), "min": round(min(tr), 4), "max": round(max(tr), 4)},
                "evaluations_x_ddim_step_s": round(n * per_step / 1e3, 4),
                "ratio": round(call / (n * per_step / 1e3), 4),
                "speedup_over_the_ddim_call": round(per_step * n_ddim / 1e3 / call, 2),
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
