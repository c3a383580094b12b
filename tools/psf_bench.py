#!/usr/bin/env python3
"""What PSF-aware observations cost.

One process, profiler off, the arms alternating:
  (1) kernels, HIP events around back-to-back launches: one Landweber step (eod_psf_residual + eod_psf_update) next to eod_obs_project,
      all channels observed, on a scene-sized tensor (1 x 4 x 2048 x 2048) and on a batch of the 13-band configuration (2 x 13 x 512 x 512),
      for (f, r) = (2, 3), (4, 6), (6, 9), (8, 12), Gaussian taps of MTF 0.3 at Nyquist (f = 6: 2046 and 510 pixels, which 6 divides).  The
      yardstick is the byte ratio: eod_obs_project moves 3 full-resolution tensors (p, values, out), the PSF step p twice and out once
      plus three coarse tensors (values, q written, q read): (3 + 3 / f^2) / 3.  Reported: time / (eod_obs_project time x byte ratio);
  (2) the call: a 25-evaluation `DPMSolverSampler.sample` with a 2-link PSF chain (bands 0, 1 at f = 2; band 2 at f = 4), iters = 1 and
      iters = 4, next to the same call without an observation, alternating, timed by a host clock around a call that ends in a
      synchronise, after a warm-up call of each.

    python tools/psf_bench.py [--arch A0] [--size 64] [--batch 16] [--steps 25] [--reps 5] [--no-call] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="A0")
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--precision", default="fp32x3")
    ap.add_argument("--timesteps", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=25, help="S of the DPM-Solver++ call")
    ap.add_argument("--reps", type=int, default=5, help="alternations")
    ap.add_argument("--launches", type=int, default=50, help="back-to-back launches per timing")
    ap.add_argument("--no-call", action="store_true", help="kernels only")
    ap.add_argument("--out", default=None, help="the JSON object is written here, too (default: profiles/psf_bench_<arch>_<size>_T<timesteps>.json)")
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", f"psf_bench_{args.arch}_{args.size}_T{args.timesteps}.json")
    if not torch.cuda.is_available():
        raise SystemExit("psf_bench.py measures on the GPU; there is nothing to time without one")
    from eo_diffusion_amd.diffusion.consistency import PsfObservation, gaussian_psf, psf_observe, psf_tau
    from eo_diffusion_amd.diffusion.dpm_solver import DPMSolverSampler
    dev = torch.device("cuda", 0)
    med = statistics.median
    L = _lib.lib()
    res = {"kernels": []}
    st = current_stream_ptr(dev)
    p = lambda t: 0 if t is None else t.data_ptr()
    with torch.no_grad():
        for B, C, edge in ((1, 4, 2048), (2, 13, 512)):
            for f, r in ((2, 3), (4, 6), (6, 9), (8, 12)):
                H = W = edge - edge % f
                g = torch.Generator(device=dev).manual_seed(1)
                x = torch.randn((B, C, H, W), device=dev, generator=g)
                vals = torch.randn((B, C, H, W), device=dev, generator=g)
                cvals = torch.randn((B, C, H // f, W // f), device=dev, generator=g)
                q, out = torch.empty_like(cvals), torch.empty_like(x)
                h = gaussian_psf(f, 0.3, radius=r)
                taps = (ctypes.c_float * h.size)(*h.tolist())
                chans = (ctypes.c_int32 * C)(*range(C))
                factors = (ctypes.c_int32 * C)(*([f] * C))
                step = psf_tau(h, f, H, W) / (f * f)
                plain = lambda: L.eod_obs_project(p(x), p(vals), 0, 1.0, factors, B, C, H, W, 0, 0, 0, p(out), st)
                resid = lambda: L.eod_psf_residual(p(x), p(cvals), 0, 1.0, taps, r, f, chans, C, B, C, H, W, 0, 0, 0, p(q), st)
                updat = lambda: L.eod_psf_update(p(x), p(q), step, taps, r, f, chans, C, B, C, H, W, p(out), st)
                arms = {"obs_project": plain, "psf_residual": resid, "psf_update": updat}
                for fn in arms.values():
                    assert fn() == 0, L.eod_last_error()
                    timed(fn, 5)
                ts = {k: [] for k in arms}
                for _ in range(args.reps):                            # the arms alternate
                    for k, fn in arms.items():
                        ts[k].append(timed(fn, args.launches))
                tp, tr, tu = (med(ts[k]) for k in ("obs_project", "psf_residual", "psf_update"))
                ratio = (3 + 3 / (f * f)) / 3
                row = {"shape": [B, C, H, W], "f": f, "r": r, "obs_project_us": round(tp * 1e3, 2), "psf_residual_us": round(tr * 1e3, 2),
                       "psf_update_us": round(tu * 1e3, 2),
                       "min_max_us": {k: [round(min(v) * 1e3, 2), round(max(v) * 1e3, 2)] for k, v in ts.items()},
                       "obs_project_GB_per_s": round(3 * 4 * x.numel() / (tp * 1e-3) / 1e9, 1), "byte_ratio": round(ratio, 3),
                       "time_over_obs_project_x_byte_ratio": round((tr + tu) / (tp * ratio), 3)}
                res["kernels"].append(row)
                print(json.dumps(row), flush=True)
        if not args.no_call:
            m = build_model(args.arch, args.size, args.precision, dev, timesteps=args.timesteps)
            shape = (3, args.size, args.size)
            x_T = m._philox((args.batch,) + shape, dev, 1, 0, args.timesteps, 0)
            truth = torch.tanh(m._philox((args.batch,) + shape, dev, 2, 0, 0, 0))
            groups = (((0, 1), 2), ((2,), 4))
            psfs = [gaussian_psf(f) for _, f in groups]
            ys = [psf_observe(truth, h, f, cs) for (cs, f), h in zip(groups, psfs)]
            chain = lambda iters: [PsfObservation(y, h, f, cs, iters=iters) for (cs, f), h, y in zip(groups, psfs, ys)]
            dpm = DPMSolverSampler(m)
            call = lambda **kw: dpm.sample(args.steps, args.batch, shape, x_T=x_T, clip_denoised=True, progress=False, **kw)
            arms = {"plain": call, "psf_iters1": lambda: call(observation=chain(1)), "psf_iters4": lambda: call(observation=chain(4))}

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
            resid = lambda z: [float((psf_observe(z, h, f, cs) - y).abs().max()) for (cs, f), h, y in zip(groups, psfs, ys)]
            res["call"] = {
                "workload": f"{args.arch} @ {args.size}x{args.size}, batch {args.batch}, {args.precision}, T = {args.timesteps}: DPM-Solver++ 2M, "
                            f"S = {args.steps} ({dpm.num_evaluations} evaluations), clip, PSF chain [bands 0, 1 at f = 2; band 2 at f = 4], weights 1",
                **{k + "_s": stat(v) for k, v in tw.items()},
                "plain_spread": round((max(tw["plain"]) - min(tw["plain"])) / med(tw["plain"]), 4),
                "ratio_iters1": round(med(tw["psf_iters1"]) / med(tw["plain"]), 4), "ratio_iters4": round(med(tw["psf_iters4"]) / med(tw["plain"]), 4),
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
