#!/usr/bin/env python3
"""What cross-band observations and chains of observations cost.

One process, profiler off, the arms alternating:
  (1) kernels, HIP events around back-to-back launches: eod_ddim_step_spec / eod_dpmpp_step_spec next to eod_ddim_step / eod_dpmpp_step on
      a scene-sized tensor (1 x 4 x 2048 x 2048, K = 1: a panchromatic band) and on a batch of the 13-band configuration
      (2 x 13 x 512 x 512 at f = 1, 2 x 13 x 510 x 510 at f = 3; K = 1, 4, 8).  The yardstick is the byte ratio: the plain step moves 4
      tensors of B x C planes (5 at second order), the cross-band form K / C of one more (the values) -- its second read of x and e_t is
      meant to come out of the cache.  Reported: measured time / (plain time x byte ratio);
  (2) the call: a 25-evaluation `DPMSolverSampler.sample` with the 2-link chain [pan at f = 1, bands at f = 4] next to the same call
      without an observation, alternating, timed by a host clock around a call that ends in a synchronise, after a warm-up call of each.

    python tools/spectral_bench.py [--arch A0] [--size 64] [--batch 16] [--steps 25] [--reps 5] [--no-call] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import build_model  # noqa: E402
from eo_diffusion_amd import _lib  # noqa: E402
from eo_diffusion_amd.engine import current_stream_ptr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(fn, reps):
    """ms per call of fn over `reps` back-to-back calls (HIP events; fn only enqueues)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def response(K, C, seed=0):
    R = np.random.default_rng(seed).random((K, C)) + 0.05
    return (R / R.sum(axis=1, keepdims=True)).astype(np.float32)


def c_floats(a):
    return (ctypes.c_float * a.size)(*a.ravel().tolist())


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
    ap.add_argument("--out", default=None, help="the JSON object is written here, too (default: profiles/spectral_bench_<arch>_<size>_T<timesteps>.json)")
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", f"spectral_bench_{args.arch}_{args.size}_T{args.timesteps}.json")
    if not torch.cuda.is_available():
        raise SystemExit("spectral_bench.py measures on the GPU; there is nothing to time without one")
    from eo_diffusion_amd.diffusion.consistency import Observation, SpectralObservation, block_mean, spectral_response
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
        for shape, f, Ks in (((1, 4, 2048, 2048), 1, (1,)), ((2, 13, 512, 512), 1, (1, 4, 8)), ((2, 13, 510, 510), 3, (1, 4, 8))):
            B, C, H, W = shape
            g = torch.Generator(device=dev).manual_seed(1)
            x, e, d = (torch.randn(shape, device=dev, generator=g) for _ in range(3))
            o1, o2 = torch.empty_like(x), torch.empty_like(x)
            n = x.numel()
            plain = {
                "ddim": lambda: L.eod_ddim_step(p(x), p(e), 0, a_s, a_t, 0.0, s1m, 1.0, p(o1), p(o2), n, st),
                "dpmpp_1": lambda: L.eod_dpmpp_step(p(x), p(e), 0, a_s, s1m, *c, 0, p(o1), p(o2), n, st),
                "dpmpp_2": lambda: L.eod_dpmpp_step(p(x), p(e), p(d), a_s, s1m, *c, 0, p(o1), p(o2), n, st),
            }
            streams = {"ddim": 4, "dpmpp_1": 4, "dpmpp_2": 5}
            for K in Ks:
                R = response(K, C)
                G = np.linalg.pinv(R.astype(np.float64)).astype(np.float32)
                cR, cG = c_floats(R), c_floats(G)
                v = torch.randn((B, K, H, W), device=dev, generator=g)
                tail = lambda: (p(v), 0, 1.0, cR, cG, K, f, B, C, H, W, 0, 0, p(o1), p(o2), st)
                spec = {
                    "ddim": lambda: L.eod_ddim_step_spec(p(x), p(e), 0, a_s, a_t, 0.0, s1m, 1.0, *tail()),
                    "dpmpp_1": lambda: L.eod_dpmpp_step_spec(p(x), p(e), 0, a_s, s1m, *c, 0, *tail()),
                    "dpmpp_2": lambda: L.eod_dpmpp_step_spec(p(x), p(e), p(d), a_s, s1m, *c, 0, *tail()),
                }
                ts = {(k, arm): [] for k in plain for arm in ("plain", "spec")}
                for k in plain:
                    for fn in (plain[k], spec[k]):
                        assert fn() == 0, L.eod_last_error()
                        timed(fn, 10)
                for _ in range(args.reps):                            # the arms alternate
                    for k in plain:
                        ts[(k, "plain")].append(timed(plain[k], args.launches))
                        ts[(k, "spec")].append(timed(spec[k], args.launches))
                row = {"shape": list(shape), "K": K, "f": f}
                for k in plain:
                    tp, to = med(ts[(k, "plain")]), med(ts[(k, "spec")])
                    ratio = (streams[k] + K / C) / streams[k]
                    row[k] = {"plain_us": round(tp * 1e3, 2), "spec_us": round(to * 1e3, 2),
                              "spec_min_max_us": [round(min(ts[(k, "spec")]) * 1e3, 2), round(max(ts[(k, "spec")]) * 1e3, 2)],
                              "plain_GB_per_s": round(streams[k] * 4 * n / (tp * 1e-3) / 1e9, 1),
                              "byte_ratio": round(ratio, 3), "time_over_plain_x_byte_ratio": round(to / (tp * ratio), 3)}
                res["kernels"].append(row)
                print(json.dumps(row), flush=True)
        if not args.no_call:
            m = build_model(args.arch, args.size, args.precision, dev, timesteps=args.timesteps)
            shape = (3, args.size, args.size)
            pan_w, factors = [[0.3, 0.5, 0.2]], (4, 4, 4)
            x_T = m._philox((args.batch,) + shape, dev, 1, 0, args.timesteps, 0)
            truth = torch.tanh(m._philox((args.batch,) + shape, dev, 2, 0, 0, 0))
            pan, bands = spectral_response(truth, pan_w), block_mean(truth, factors)
            chain = [SpectralObservation(pan, pan_w), Observation(bands, factors)]
            dpm = DPMSolverSampler(m)
            arms = {"plain": lambda: dpm.sample(args.steps, args.batch, shape, x_T=x_T, clip_denoised=True, progress=False),
                    "chain": lambda: dpm.sample(args.steps, args.batch, shape, x_T=x_T, clip_denoised=True, progress=False, observation=chain)}

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
                    dt, (out, inter) = wall(fn)
                    tw[k].append(dt)
            last = inter["pred_x0"][-1]
            res["call"] = {
                "workload": f"{args.arch} @ {args.size}x{args.size}, batch {args.batch}, {args.precision}, T = {args.timesteps}: DPM-Solver++ 2M, "
                            f"S = {args.steps} ({dpm.num_evaluations} evaluations), clip, chain [pan {pan_w[0]} at f = 1, bands at f = 4], weights 1",
                "plain_s": {"median": round(med(tw["plain"]), 4), "min": round(min(tw["plain"]), 4), "max": round(max(tw["plain"]), 4)},
                "chain_s": {"median": round(med(tw["chain"]), 4), "min": round(min(tw["chain"]), 4), "max": round(max(tw["chain"]), 4)},
                "plain_spread": round((max(tw["plain"]) - min(tw["plain"])) / med(tw["plain"]), 4),
                "ratio": round(med(tw["chain"]) / med(tw["plain"]), 4),
                "last_prediction_max_abs_pan_residual": float((spectral_response(last, pan_w) - pan).abs().max()),
                "last_prediction_max_abs_band_residual": float((block_mean(last, factors) - bands).abs().max()),
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
