#!/usr/bin/env python3
"""What the exact PSF data consistency costs.

One process, profiler off, the arms alternating, at the shapes of tools/psf_bench.py (1 x 4 x 2048 x 2048 and 2 x 13 x 512 x 512, all channels
observed, (f, r) = (2, 3), (4, 6), (6, 9), (8, 12), Gaussian taps of MTF 0.3; f = 6: 2046 and 510 pixels):
  (1) one CG iteration, (eod_psf_cg at 9 iterations - eod_psf_cg at 1) / 8, next to one Landweber step (eod_psf_residual + eod_psf_update);
  (2) the whole projection at iters = 16 (eod_psf_residual + eod_psf_cg + eod_psf_update) next to Landweber at iters = 8
      (8 x (eod_psf_residual + eod_psf_update)), HIP events around back-to-back launches;
  (3) the call: a 25-evaluation `DPMSolverSampler.sample` with the 2-link PSF chain of tools/psf_bench.py (bands 0, 1 at f = 2; band 2 at
      f = 4) under solver="cg", iters = 16 and under Landweber, iters = 4, next to the same call without an observation, each with the last
      prediction's residuals max |A x - y|.

    python tools/psf_cg_bench.py [--arch A0] [--size 64] [--batch 16] [--steps 25] [--reps 5] [--no-call] [--out FILE]
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
    ap.add_argument("--launches", type=int, default=20, help="back-to-back calls per timing")
    ap.add_argument("--no-call", action="store_true", help="kernels only")
    ap.add_argument("--out", default=None, help="the JSON object is written here, too (default: profiles/psf_cg_bench_<arch>_<size>_T<timesteps>.json)")
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", f"psf_cg_bench_{args.arch}_{args.size}_T{args.timesteps}.json")
    if not torch.cuda.is_available():
        raise SystemExit("psf_cg_bench.py measures on the GPU; there is nothing to time without one")
    from eo_diffusion_amd.diffusion.consistency import PsfObservation, gaussian_psf, psf_gram, psf_observe, psf_tau
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
                Hc, Wc = H // f, W // f
                g = torch.Generator(device=dev).manual_seed(1)
                x = torch.randn((B, C, H, W), device=dev, generator=g)
                cvals = torch.randn((B, C, Hc, Wc), device=dev, generator=g)
                c, q, out = torch.empty_like(cvals), torch.empty_like(cvals), torch.empty_like(x)
                h = gaussian_psf(f, 0.3, radius=r)
                taps = (ctypes.c_float * h.size)(*h.tolist())
                chans = (ctypes.c_int32 * C)(*range(C))
                step = psf_tau(h, f, H, W) / (f * f)
                gy, b = psf_gram(h, f, H)
                gy = gx = torch.from_numpy(gy).to(dev)
                ws = torch.empty(int(L.eod_psf_cg_workspace_size(B, C, Hc, Wc)), device=dev, dtype=torch.uint8)
                resid = lambda dst=q: L.eod_psf_residual(p(x), p(cvals), 0, 1.0, taps, r, f, chans, C, B, C, H, W, 0, 0, 0, p(dst), st)
                updat = lambda s=step: L.eod_psf_update(p(x), p(q), s, taps, r, f, chans, C, B, C, H, W, p(out), st)
                solve = lambda n: L.eod_psf_cg(p(c), 0, 0.0, 1.0, p(gy), p(gx), b, n, B, C, Hc, Wc, 0, 0, p(q), p(ws), ws.numel(), st)

                def landweber(n):
                    rc = 0
                    for _ in range(n):
                        rc |= resid() | updat()
                    return rc

                arms = {"landweber_1": lambda: landweber(1), "cg_1": lambda: solve(1), "cg_9": lambda: solve(9),
                        "landweber_8": lambda: landweber(8), "project_cg_16": lambda: resid(c) | solve(16) | updat(1.0 / (f * f))}
                for fn in arms.values():
                    assert fn() == 0, L.eod_last_error()
                    timed(fn, 3)
                ts = {k: [] for k in arms}
                for _ in range(args.reps):                            # the arms alternate
                    for k, fn in arms.items():
                        ts[k].append(timed(fn, args.launches))
                m = {k: med(v) for k, v in ts.items()}
                row = {"shape": [B, C, H, W], "f": f, "r": r, "b": b, "landweber_step_us": round(m["landweber_1"] * 1e3, 2),
                       "cg_iteration_us": round((m["cg_9"] - m["cg_1"]) / 8 * 1e3, 2), "cg_1_us": round(m["cg_1"] * 1e3, 2),
                       "landweber_8_us": round(m["landweber_8"] * 1e3, 2), "project_cg_16_us": round(m["project_cg_16"] * 1e3, 2),
                       "min_max_us": {k: [round(min(v) * 1e3, 2), round(max(v) * 1e3, 2)] for k, v in ts.items()},
                       "cg_iteration_over_landweber_step": round((m["cg_9"] - m["cg_1"]) / 8 / m["landweber_1"], 4),
                       "project_cg_16_over_landweber_8": round(m["project_cg_16"] / m["landweber_8"], 4)}
                res["kernels"].append(row)
                print(json.dumps(row), flush=True)
        if not args.no_call:
            mdl = build_model(args.arch, args.size, args.precision, dev, timesteps=args.timesteps)
            shape = (3, args.size, args.size)
            x_T = mdl._philox((args.batch,) + shape, dev, 1, 0, args.timesteps, 0)
            truth = torch.tanh(mdl._philox((args.batch,) + shape, dev, 2, 0, 0, 0))
            groups = (((0, 1), 2), ((2,), 4))
            psfs = [gaussian_psf(f) for _, f in groups]
            ys = [psf_observe(truth, h, f, cs) for (cs, f), h in zip(groups, psfs)]
            chain = lambda **kw: [PsfObservation(y, h, f, cs, **kw) for (cs, f), h, y in zip(groups, psfs, ys)]
            dpm = DPMSolverSampler(mdl)
            call = lambda **kw: dpm.sample(args.steps, args.batch, shape, x_T=x_T, clip_denoised=True, progress=False, **kw)
            arms = {"plain": call, "landweber_iters4": lambda: call(observation=chain(iters=4)),
                    "cg_iters16": lambda: call(observation=chain(iters=16, solver="cg"))}

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
                "ratio_landweber_iters4": round(med(tw["landweber_iters4"]) / med(tw["plain"]), 4),
                "ratio_cg_iters16": round(med(tw["cg_iters16"]) / med(tw["plain"]), 4),
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
