#!/usr/bin/env python3
"""What a band mix in front of the PSF costs.

One process, profiler off, HIP events, the arms alternating, the median of `--reps`:
  (1) eod_psf_residual_mix + eod_psf_update_mix (R [K, C], G = R^T) next to eod_psf_residual + eod_psf_update on K listed channels, at
      1 x 4 x 2048 x 2048 and 2 x 13 x 512 x 512, f in {1, 4} (Gaussian taps of MTF 0.3: r = 2 and 6), K in {1, 4}.  From the bytes the mixed
      residual reads C / K times the fine planes of the unmixed one and the mixed update K times its coarse planes, and writes all C channels
      where the unmixed one blurs K and copies the rest;
  (2) the call: a 25-evaluation `DPMSolverSampler.sample` with the chain [a pan band at f = 1 through gaussian_psf(1) with a response, the
      three bands at f = 4 through their PSF], both solver="cg", iters = 16, next to the same call without an observation, with the last
      prediction's residuals max |A x - y| of both links.

    python tools/spectral_psf_bench.py [--arch A0] [--size 64] [--batch 16] [--steps 25] [--reps 5] [--no-call] [--out FILE]
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
PAN3 = [[0.3, 0.5, 0.2]]


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
    ap.add_argument("--launches", type=int, default=20, help="back-to-back calls per timing")
    ap.add_argument("--no-call", action="store_true", help="kernels only")
    ap.add_argument("--out", default=None, help="the JSON object is written here, too (default: profiles/spectral_psf_bench_<arch>_<size>_T<timesteps>.json)")
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", f"spectral_psf_bench_{args.arch}_{args.size}_T{args.timesteps}.json")
    if not torch.cuda.is_available():
        raise SystemExit("spectral_psf_bench.py measures on the GPU; there is nothing to time without one")
    from eo_diffusion_amd.diffusion.consistency import PsfObservation, gaussian_psf, psf_observe, psf_tau
    from eo_diffusion_amd.diffusion.dpm_solver import DPMSolverSampler
    dev = torch.device("cuda", 0)
    med = statistics.median
    L = _lib.lib()
    res = {"kernels": []}
    st = current_stream_ptr(dev)
    p = lambda t: 0 if t is None else t.data_ptr()
    floats = lambda a: (ctypes.c_float * a.size)(*a.ravel().tolist())
    with torch.no_grad():
        for B, C, edge in ((1, 4, 2048), (2, 13, 512)):
            for f in (1, 4):
                for K in (1, 4):
                    H = W = edge
                    Hc, Wc = H // f, W // f
                    g = torch.Generator(device=dev).manual_seed(1)
                    x = torch.randn((B, C, H, W), device=dev, generator=g)
                    vals = torch.randn((B, K, Hc, Wc), device=dev, generator=g)
                    q, out = torch.empty_like(vals), torch.empty_like(x)
                    h = gaussian_psf(f, 0.3)
                    r = h.size // 2
                    taps = floats(h)
                    chans = (ctypes.c_int32 * K)(*range(K))
                    R = np.random.default_rng(K).uniform(0.1, 1.0, (K, C)).astype(np.float32)
                    cR, cG = floats(R), floats(np.ascontiguousarray(R.T))
                    step = psf_tau(h, f, H, W) / (f * f)
                    arms = {
                        "residual": lambda: L.eod_psf_residual(p(x), p(vals), 0, 1.0, taps, r, f, chans, K, B, C, H, W, 0, 0, 0, p(q), st),
                        "residual_mix": lambda: L.eod_psf_residual_mix(p(x), p(vals), 0, 1.0, taps, r, f, cR, K, B, C, H, W, 0, 0, p(q), st),
                        "update": lambda: L.eod_psf_update(p(x), p(q), step, taps, r, f, chans, K, B, C, H, W, p(out), st),
                        "update_mix": lambda: L.eod_psf_update_mix(p(x), p(q), step, taps, r, f, cG, K, B, C, H, W, p(out), st),
                    }
                    for fn in arms.values():
                        assert fn() == 0, L.eod_last_error()
                        timed(fn, 3)
                    ts = {k: [] for k in arms}
                    for _ in range(args.reps):                        # the arms alternate
                        for k, fn in arms.items():
                            ts[k].append(timed(fn, args.launches))
                    m = {k: med(v) for k, v in ts.items()}
                    row = {"shape": [B, C, H, W], "f": f, "r": r, "K": K, **{k + "_us": round(v * 1e3, 2) for k, v in m.items()},
                           "min_max_us": {k: [round(min(v) * 1e3, 2), round(max(v) * 1e3, 2)] for k, v in ts.items()},
                           "residual_mix_over_residual": round(m["residual_mix"] / m["residual"], 4),
                           "update_mix_over_update": round(m["update_mix"] / m["update"], 4),
                           "pair_mix_over_pair": round((m["residual_mix"] + m["update_mix"]) / (m["residual"] + m["update"]), 4)}
                    res["kernels"].append(row)
                    print(json.dumps(row), flush=True)
        if not args.no_call:
            mdl = build_model(args.arch, args.size, args.precision, dev, timesteps=args.timesteps)
            shape = (3, args.size, args.size)
            x_T = mdl._philox((args.batch,) + shape, dev, 1, 0, args.timesteps, 0)
            truth = torch.tanh(mdl._philox((args.batch,) + shape, dev, 2, 0, 0, 0))
            h1, h4 = gaussian_psf(1), gaussian_psf(4)
            y_pan, y_bands = psf_observe(truth, h1, 1, response=PAN3), psf_observe(truth, h4, 4)
            chain = lambda: [PsfObservation(y_pan, h1, 1, iters=16, solver="cg", response=PAN3), PsfObservation(y_bands, h4, 4, iters=16, solver="cg")]
            dpm = DPMSolverSampler(mdl)
            call = lambda **kw: dpm.sample(args.steps, args.batch, shape, x_T=x_T, clip_denoised=True, progress=False, **kw)
            arms = {"plain": call, "pan_psf_chain_cg16": lambda: call(observation=chain())}

            def wall(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                return time.perf_counter() - t0, out

            for fn in arms.values():
                wall(fn)
            tw, last = {k: [] for k in arms}, {}
            for _ in range(args.reps):
                for k, fn in arms.items():
                    dt, (out, inter) = wall(fn)
                    tw[k].append(dt)
                    last[k] = inter["pred_x0"][-1]
            stat = lambda v: {"median": round(med(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
            resid = lambda z: {"pan_f1": float((psf_observe(z, h1, 1, response=PAN3) - y_pan).abs().max()),
                               "bands_f4": float((psf_observe(z, h4, 4) - y_bands).abs().max())}
            res["call"] = {
                "workload": f"{args.arch} @ {args.size}x{args.size}, batch {args.batch}, {args.precision}, T = {args.timesteps}: DPM-Solver++ 2M, "
                            f"S = {args.steps} ({dpm.num_evaluations} evaluations), clip, chain [pan {PAN3[0]} through gaussian_psf(1) at f = 1; "
                            f"three bands through gaussian_psf(4) at f = 4], cg iters = 16, weights 1",
                **{k + "_s": stat(v) for k, v in tw.items()},
                "plain_spread": round((max(tw["plain"]) - min(tw["plain"])) / med(tw["plain"]), 4),
                "ratio_pan_psf_chain_cg16": round(med(tw["pan_psf_chain_cg16"]) / med(tw["plain"]), 4),
                "last_prediction_max_abs_residuals": {k: resid(z) for k, z in last.items()},
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
