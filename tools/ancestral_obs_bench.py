#!/usr/bin/env python3
"""What observations on the ancestral samplers cost.

One process, profiler off, the arms alternating:
  (1) kernels, HIP events around back-to-back launches: eod_ddpm_pred_x0 and eod_ddpm_step_p0 next to eod_ddpm_step (clip = 1) on a batch
      (16 x 3 x 256 x 256) and on a scene (1 x 3 x 2048 x 2048).  The yardstick is the byte ratio: eod_ddpm_step moves 4 tensors (x, pred,
      noise, out), eod_ddpm_pred_x0 3 (x, pred, p0) and eod_ddpm_step_p0 4 (x, p0c, noise, out).  Reported per kernel:
      time / (eod_ddpm_step time x byte ratio);
  (2) the call: a T-step ancestral `EODiffusion.sampling` (T = 250) without an observation, with a block-mean Observation (factors 1, 2, 4)
      and with a 2-link chain [a pan band as a SpectralObservation at f = 1, the three bands at f = 4], alternating, timed by a host clock
      around a call that ends in a synchronise, after a warm-up call of each.  Recorded: whether the observed calls' medians lie within the
      plain call's own spread (its min .. max over the alternations).

    python tools/ancestral_obs_bench.py [--arch A0] [--size 64] [--batch 16] [--timesteps 250] [--reps 5] [--no-call] [--out FILE]
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
    ap.add_argument("--timesteps", type=int, default=250, help="T of the ancestral call")
    ap.add_argument("--reps", type=int, default=5, help="alternations")
    ap.add_argument("--launches", type=int, default=50, help="back-to-back launches per timing")
    ap.add_argument("--no-call", action="store_true", help="kernels only")
    ap.add_argument("--out", default=None, help="the JSON object is written here, too (default: profiles/ancestral_obs_bench_<arch>_<size>.json)")
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", f"ancestral_obs_bench_{args.arch}_{args.size}.json")
    if not torch.cuda.is_available():
        raise SystemExit("ancestral_obs_bench.py measures on the GPU; there is nothing to time without one")
    from eo_diffusion_amd.diffusion.consistency import Observation, SpectralObservation, block_mean, spectral_response
    dev = torch.device("cuda", 0)
    med = statistics.median
    L = _lib.lib()
    res = {"kernels": []}
    st = current_stream_ptr(dev)
    p = lambda t: t.data_ptr()
    with torch.no_grad():
        from eo_diffusion_amd.diffusion.model import EODiffusion
        sched = EODiffusion(torch.nn.Identity(), args.size, 3, timesteps=1000).to(dev)     # (the schedule buffers of T = 1000)
        T = sched.timesteps
        for N, C, edge in ((16, 3, 256), (1, 3, 2048)):
            g = torch.Generator(device=dev).manual_seed(1)
            x, e, z = (torch.randn((N, C, edge, edge), device=dev, generator=g) for _ in range(3))
            p0, out = torch.empty_like(x), torch.empty_like(x)
            t = torch.full((N,), 500, dtype=torch.int64, device=dev)
            chw = C * edge * edge
            arms = {
                "ddpm_step": lambda: L.eod_ddpm_step(p(x), p(e), p(z), p(t), p(sched.betas), p(sched.alphas), p(sched.alphas_cumprod),
                                                     p(sched.sqrt_one_minus_alphas_cumprod), p(out), N, chw, T, 1, st),
                "ddpm_pred_x0": lambda: L.eod_ddpm_pred_x0(p(x), p(e), p(t), p(sched.alphas_cumprod), p(p0), N, chw, T, 1, st),
                "ddpm_step_p0": lambda: L.eod_ddpm_step_p0(p(x), p(p0), p(z), p(t), p(sched.betas), p(sched.alphas), p(sched.alphas_cumprod), p(out),
                                                           N, chw, T, st),
            }
            for fn in arms.values():
                assert fn() == 0, L.eod_last_error()
                timed(fn, 5)
            ts = {k: [] for k in arms}
            for _ in range(args.reps):                                # the arms alternate
                for k, fn in arms.items():
                    ts[k].append(timed(fn, args.launches))
            tf, tp, tq = (med(ts[k]) for k in ("ddpm_step", "ddpm_pred_x0", "ddpm_step_p0"))
            row = {"shape": [N, C, edge, edge], **{k + "_us": round(med(v) * 1e3, 2) for k, v in ts.items()},
                   "min_max_us": {k: [round(min(v) * 1e3, 2), round(max(v) * 1e3, 2)] for k, v in ts.items()},
                   "ddpm_step_GB_per_s": round(4 * 4 * x.numel() / (tf * 1e-3) / 1e9, 1),
                   "byte_ratio": {"ddpm_pred_x0": 0.75, "ddpm_step_p0": 1.0},
                   "pred_x0_time_over_ddpm_step_x_byte_ratio": round(tp / (tf * 0.75), 3),
                   "step_p0_time_over_ddpm_step_x_byte_ratio": round(tq / (tf * 1.0), 3),
                   "pair_over_ddpm_step": round((tp + tq) / tf, 3)}
            res["kernels"].append(row)
            print(json.dumps(row), flush=True)
        del sched
        if not args.no_call:
            m = build_model(args.arch, args.size, args.precision, dev, timesteps=args.timesteps)
            shape = (args.batch, 3, args.size, args.size)
            truth = torch.tanh(m._philox(shape, dev, 2, 0, 0, 0))
            pan = [[0.3, 0.5, 0.2]]
            block = Observation(block_mean(truth, (1, 2, 4)), (1, 2, 4))
            chain = [SpectralObservation(spectral_response(truth, pan, 1), pan, 1), Observation(block_mean(truth, (4, 4, 4)), (4, 4, 4))]
            call = lambda **kw: m.sampling(args.batch, device=str(dev), rng="philox", seed=1, progress=False, **kw)
            arms = {"plain": call, "block": lambda: call(observation=block), "chain2": lambda: call(observation=chain)}

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
                    dt, last[k] = wall(fn)
                    tw[k].append(dt)
            stat = lambda v: {"median": round(med(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
            lo, hi = min(tw["plain"]), max(tw["plain"])
            miss = lambda o: float((block_mean(o, (1, 2, 4)) - block.values.to(dev)).abs().max())
            res["call"] = {
                "workload": f"{args.arch} @ {args.size}x{args.size}, batch {args.batch}, {args.precision}: ancestral sampling, T = {args.timesteps} "
                            f"evaluations, clip, philox; block: factors (1, 2, 4); chain2: [pan band at f = 1, three bands at f = 4]; weights 1",
                **{k + "_s": stat(v) for k, v in tw.items()},
                "plain_spread": round((hi - lo) / med(tw["plain"]), 4),
                "ratio_block": round(med(tw["block"]) / med(tw["plain"]), 4), "ratio_chain2": round(med(tw["chain2"]) / med(tw["plain"]), 4),
                "per_evaluation_extra_us": {k: round((med(tw[k]) - med(tw["plain"])) / args.timesteps * 1e6, 1) for k in ("block", "chain2")},
                "within_plain_spread": {k: bool(lo <= med(tw[k]) <= hi) for k in ("block", "chain2")},
                "returned_sample_max_abs_block_mean_miss": {k: miss(o) for k, o in last.items()},
                "finite": all(bool(torch.isfinite(o).all()) for o in last.values()),
            }
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
