#!/usr/bin/env python3
"""What observation consistency costs.

One process, profiler off, the arms alternating:
  (1) kernels, HIP events around back-to-back launches: eod_ddim_step_obs / eod_dpmpp_step_obs next to eod_ddim_step / eod_dpmpp_step
      (the step kernels as they were before this feature: their code is untouched) on a scene-sized tensor (1 x 3 x 2048 x 2048) and on a
      batch of the 13-band configuration (2 x 13 x 512 x 512), for the factor sets all-1, (1, 2, 4) and a Sentinel-2-like one, with and
      without a mask.  The yardstick is the byte ratio: the obs form moves 5 tensors (6 with a mask) where the plain step moves 4, at
      second order 6 (7) against 5.  Reported: measured time / (plain time x byte ratio);
  (2) the call: a 25-evaluation `DPMSolverSampler.sample` with an observation next to the same call without one, alternating, timed by a
      host clock around a call that ends in a synchronise, after a warm-up call of each.

    python tools/consistency_bench.py [--arch A0] [--size 64] [--batch 16] [--steps 25] [--reps 5] [--no-call] [--out FILE]
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
from eo_diffusion_amd import _lib  # noqa: E402
from eo_diffusion_amd.engine import current_stream_ptr  # noqa: E402

S2 = (6, 1, 1, 1, 2, 2, 2, 1, 2, 6, 6, 2, 2)


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
    ap.add_argument("--reps", type=int, default=5, help="alternations")
    ap.add_argument("--launches", type=int, default=100, help="back-to-back launches per timing")
    ap.add_argument("--no-call", action="store_true", help="kernels only")
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("consistency_bench.py measures on the GPU; there is nothing to time without one")
    from eo_diffusion_amd.diffusion.consistency import Observation, block_mean
    from eo_diffusion_amd.diffusion.dpm_solver import DPMSolverSampler
    from eo_diffusion_amd.diffusion.util import dpm_coefficients
    dev = torch.device("cuda", 0)
    med = statistics.median
    L = _lib.lib()
    res = {"kernels": []}
    a_s, a_t = 0.37, 0.61
    s1m = (1.0 - a_s) ** 0.5
    c = [float(v) for v in dpm_coefficients(a_s, a_t, 0.4, 2)]
    st = current_stream_ptr(dev)
    p = lambda t: 0 if t is None else t.data_ptr()
    with torch.no_grad():
        for shape, sets in (((1, 3, 2048, 2048), {"all_1": (1, 1, 1), "1_2_4": (1, 2, 4)}), ((2, 13, 512, 512), {"all_1": (1,) * 13, "sentinel2": S2})):
            B, C, H, W = shape
            g = torch.Generator(device=dev).manual_seed(1)
            x, e, d, v = (torch.randn(shape, device=dev, generator=g) for _ in range(4))
            mk = (torch.rand(shape, device=dev, generator=g) > 0.5).float()
            o1, o2 = torch.empty_like(x), torch.empty_like(x)
            n = x.numel()
            nbytes = 4 * n
            plain = {
                "ddim": lambda: L.eod_ddim_step(p(x), p(e), 0, a_s, a_t, 0.0, s1m, 1.0, p(o1), p(o2), n, st),
                "dpmpp_1": lambda: L.eod_dpmpp_step(p(x), p(e), 0, a_s, s1m, *c, 0, p(o1), p(o2), n, st),
                "dpmpp_2": lambda: L.eod_dpmpp_step(p(x), p(e), p(d), a_s, s1m, *c, 0, p(o1), p(o2), n, st),
            }
            streams = {"ddim": 4, "dpmpp_1": 4, "dpmpp_2": 5}
            for fname, factors in sets.items():
                f = (ctypes.c_int32 * C)(*factors)
                for masked in (False, True):
                    m_ = mk if masked else None
                    tail = lambda: (p(v), p(m_), 1.0, f, B, C, H, W, 0, 0, 0, p(o1), p(o2), st)
                    obs = {
                        "ddim": lambda: L.eod_ddim_step_obs(p(x), p(e), 0, a_s, a_t, 0.0, s1m, 1.0, *tail()),
                        "dpmpp_1": lambda: L.eod_dpmpp_step_obs(p(x), p(e), 0, a_s, s1m, *c, 0, *tail()),
                        "dpmpp_2": lambda: L.eod_dpmpp_step_obs(p(x), p(e), p(d), a_s, s1m, *c, 0, *tail()),
                    }
                    ts = {(k, arm): [] for k in plain for arm in ("plain", "obs")}
                    for k in plain:
                        for fn in (plain[k], obs[k]):
                            assert fn() == 0, L.eod_last_error()
                            timed(fn, 10)
                    for _ in range(args.reps):                        # the arms alternate
                        for k in plain:
                            ts[(k, "plain")].append(timed(plain[k], args.launches))
                            ts[(k, "obs")].append(timed(obs[k], args.launches))
                    row = {"shape": list(shape), "factors": fname, "mask": masked, "launches_per_call": len(set(factors))}
                    for k in plain:
                        tp, to = med(ts[(k, "plain")]), med(ts[(k, "obs")])
                        ratio = (streams[k] + 1 + int(masked)) / streams[k]
                        row[k] = {"plain_us": round(tp * 1e3, 2), "obs_us": round(to * 1e3, 2),
                                  "obs_min_max_us": [round(min(ts[(k, "obs")]) * 1e3, 2), round(max(ts[(k, "obs")]) * 1e3, 2)],
                                  "plain_GB_per_s": round(streams[k] * nbytes / (tp * 1e-3) / 1e9, 1),
                                  "obs_GB_per_s": round((streams[k] + 1 + int(masked)) * nbytes / (to * 1e-3) / 1e9, 1),
                                  "byte_ratio": round(ratio, 3), "time_over_plain_x_byte_ratio": round(to / (tp * ratio), 3)}
                    res["kernels"].append(row)
                    print(json.dumps(row), flush=True)
        if not args.no_call:
            m = build_model(args.arch, args.size, args.precision, dev, timesteps=args.timesteps)
            shape = (3, args.size, args.size)
            factors = (1, 2, 4)
            x_T = m._philox((args.batch,) + shape, dev, 1, 0, args.timesteps, 0)
            values = block_mean(torch.tanh(m._philox((args.batch,) + shape, dev, 2, 0, 0, 0)), factors)
            ob = Observation(values, factors)
            dpm = DPMSolverSampler(m)
            arms = {"plain": lambda: dpm.sample(args.steps, args.batch, shape, x_T=x_T, clip_denoised=True, progress=False)[0],
                    "observed": lambda: dpm.sample(args.steps, args.batch, shape, x_T=x_T, clip_denoised=True, progress=False, observation=ob)[0]}

            def wall(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                return time.perf_counter() - t0, out

            for fn in arms.values():
                wall(fn)
            tw = {k: [] for k in arms}
            for _ in range(args.reps):
                for k, fn in arms.items():
                    dt, out = wall(fn)
                    tw[k].append(dt)
            resid = float((block_mean(out, factors) - values).abs().max())
            res["call"] = {
                "workload": f"{args.arch} @ {args.size}x{args.size}, batch {args.batch}, {args.precision}, T = {args.timesteps}: DPM-Solver++ 2M, "
                            f"S = {args.steps} ({dpm.num_evaluations} evaluations), clip, factors {factors}, no mask, weight 1",
                "plain_s": {"median": round(med(tw["plain"]), 4), "min": round(min(tw["plain"]), 4), "max": round(max(tw["plain"]), 4)},
                "observed_s": {"median": round(med(tw["observed"]), 4), "min": round(min(tw["observed"]), 4), "max": round(max(tw["observed"]), 4)},
                "plain_spread": round((max(tw["plain"]) - min(tw["plain"])) / med(tw["plain"]), 4),
                "ratio": round(med(tw["observed"]) / med(tw["plain"]), 4),
                "max_abs_block_mean_minus_values_of_the_result": resid,
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
