#!/usr/bin/env python3
"""What reading a model output as x0 or v costs (DESIGN.md sections 8.2 and 9.16).  Nothing here is a gate.

One process, profiler off, the arms alternating:
  (1) kernels, HIP events around back-to-back launches, at 16 x 3 x 64 x 64, 16 x 3 x 256 x 256 and 1 x 4 x 2048 x 2048:
      eod_param_pred (v, with and without e_t) next to eod_pred_x0 -- the byte model is 4/3 of eod_pred_x0 (x, o, p0, e_t against x, e_t,
      p0) with e_t and 1.0 without; eod_q_sample_v next to eod_q_sample -- 4/3 of it (x0, noise, x_t, v against x0, noise, x_t), and 4/6 of
      the two-pass form (eod_q_sample, then a second pass of two reads and one write for v, timed here as a second eod_q_sample).
      Reported per kernel: time / (the yardstick's time x byte ratio);
  (2) the cancellation table of the design, re-measured on the kernels: max |error of the prediction| of a v output on 65 536
      standard-normal elements against float64 on the same rounded inputs -- eod_param_pred, and the via-eps route as the kernels would run
      it (the noise estimate eod_param_pred writes, fed to eod_pred_x0);
  (3) the calls: a 25-evaluation DPM-Solver++ call and a 250-step DDIM call (eta 0) on the same weights read as eps and as v, alternating,
      timed by a host clock around a call that ends in a synchronise, after a warm-up call of each.

    python tools/param_bench.py [--arch A0] [--size 64] [--batch 16] [--timesteps 1000] [--reps 5] [--no-call] [--out FILE]
"""
import argparse
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
LEVELS = (2.43e-9, 2.4e-6, 1e-4, 0.37)


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
    ap.add_argument("--reps", type=int, default=5, help="alternations")
    ap.add_argument("--launches", type=int, default=50, help="back-to-back launches per timing")
    ap.add_argument("--no-call", action="store_true", help="kernels and the cancellation table only")
    ap.add_argument("--out", default=None, help="the JSON object is written here, too (default: profiles/param_bench_<arch>_<size>_T<timesteps>.json)")
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", f"param_bench_{args.arch}_{args.size}_T{args.timesteps}.json")
    if not torch.cuda.is_available():
        raise SystemExit("param_bench.py measures on the GPU; there is nothing to time without one")
    dev = torch.device("cuda", 0)
    med = statistics.median
    L = _lib.lib()
    st = current_stream_ptr(dev)
    p = lambda t: t.data_ptr()
    res = {"kernels": [], "cancellation": []}
    with torch.no_grad():
        from eo_diffusion_amd.diffusion.model import EODiffusion
        sched = EODiffusion(torch.nn.Identity(), args.size, 3, timesteps=1000).to(dev)     # (the schedule buffers of T = 1000)
        T, sa, sb = sched.timesteps, sched.sqrt_alphas_cumprod, sched.sqrt_one_minus_alphas_cumprod
        a, s1 = 0.37, float(np.sqrt(np.float32(1.0) - np.float32(0.37)))
        for N, C, edge in ((16, 3, 64), (16, 3, 256), (1, 4, 2048)):
            g = torch.Generator(device=dev).manual_seed(1)
            x, o = (torch.randn((N, C, edge, edge), device=dev, generator=g) for _ in range(2))
            p0, e_t = torch.empty_like(x), torch.empty_like(x)
            t = torch.full((N,), 500, dtype=torch.int64, device=dev)
            n, chw = x.numel(), C * edge * edge
            arms = {
                "pred_x0": lambda: L.eod_pred_x0(p(x), p(o), a, s1, 0, p(p0), n, st),
                "param_pred_e": lambda: L.eod_param_pred(p(x), p(o), 2, a, s1, 0, p(p0), p(e_t), n, st),
                "param_pred": lambda: L.eod_param_pred(p(x), p(o), 2, a, s1, 0, p(p0), 0, n, st),
                "q_sample": lambda: L.eod_q_sample(p(x), p(o), p(t), p(sa), p(sb), p(p0), N, chw, T, st),
                "q_sample_v": lambda: L.eod_q_sample_v(p(x), p(o), p(t), p(sa), p(sb), p(p0), p(e_t), N, chw, T, st),
            }
            for fn in arms.values():
                assert fn() == 0, L.eod_last_error()
                timed(fn, 5)
            ts = {k: [] for k in arms}
            for _ in range(args.reps):                                # the arms alternate
                for k, fn in arms.items():
                    ts[k].append(timed(fn, args.launches))
            m = {k: med(v) for k, v in ts.items()}
            row = {"shape": [N, C, edge, edge], **{k + "_us": round(v * 1e3, 2) for k, v in m.items()},
                   "min_max_us": {k: [round(min(v) * 1e3, 2), round(max(v) * 1e3, 2)] for k, v in ts.items()},
                   "pred_x0_GB_per_s": round(3 * 4 * n / (m["pred_x0"] * 1e-3) / 1e9, 1),
                   "byte_ratio": {"param_pred_e / pred_x0": round(4 / 3, 4), "param_pred / pred_x0": 1.0, "q_sample_v / q_sample": round(4 / 3, 4),
                                  "q_sample_v / two passes": round(4 / 6, 4)},
                   "param_pred_e_time_over_pred_x0_x_byte_ratio": round(m["param_pred_e"] / (m["pred_x0"] * 4 / 3), 3),
                   "param_pred_time_over_pred_x0_x_byte_ratio": round(m["param_pred"] / m["pred_x0"], 3),
                   "q_sample_v_time_over_q_sample_x_byte_ratio": round(m["q_sample_v"] / (m["q_sample"] * 4 / 3), 3),
                   "q_sample_v_over_two_q_sample_passes": round(m["q_sample_v"] / (2 * m["q_sample"]), 3)}
            res["kernels"].append(row)
            print(json.dumps(row), flush=True)
        del sched
        # (2) the cancellation table on the kernels
        rng = np.random.default_rng(0)
        xh, vh = rng.standard_normal(65536).astype(np.float32), rng.standard_normal(65536).astype(np.float32)
        x, v = torch.from_numpy(xh).to(dev), torch.from_numpy(vh).to(dev)
        p0, e_t, via = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        for a in LEVELS:
            sa32, s1_32 = np.sqrt(np.float32(a)), np.sqrt(np.float32(1.0) - np.float32(a))
            assert L.eod_param_pred(p(x), p(v), 2, a, float(s1_32), 0, p(p0), p(e_t), x.numel(), st) == 0, L.eod_last_error()
            assert L.eod_pred_x0(p(x), p(e_t), a, float(s1_32), 0, p(via), x.numel(), st) == 0, L.eod_last_error()
            want = float(sa32) * xh.astype(np.float64) - float(s1_32) * vh.astype(np.float64)
            row = {"a": a, "via_eps_max_abs_error": float(np.abs(via.cpu().numpy().astype(np.float64) - want).max()),
                   "direct_max_abs_error": float(np.abs(p0.cpu().numpy().astype(np.float64) - want).max())}
            res["cancellation"].append(row)
            print(json.dumps(row), flush=True)
        if not args.no_call:
            from eo_diffusion_amd.diffusion.ddim import DDIMSampler
            from eo_diffusion_amd.diffusion.dpm_solver import DPMSolverSampler
            m = build_model(args.arch, args.size, args.precision, dev, timesteps=args.timesteps)
            shape = (3, args.size, args.size)
            x_T = m._philox((args.batch,) + shape, dev, 2, 0, 0, 0)

            def call(which, parameterization):
                m.parameterization = parameterization
                if which == "dpm":
                    return DPMSolverSampler(m).sample(25, args.batch, shape, x_T=x_T, progress=False)[0]
                return DDIMSampler(m).sample(250, args.batch, shape, eta=0.0, x_T=x_T, verbose=False, progress=False)[0]

            arms = {f"{w}_{k}": (lambda w=w, k=k: call(w, k)) for w in ("dpm", "ddim") for k in ("eps", "v")}

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
            m.parameterization = "eps"
            stat = lambda v: {"median": round(med(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
            res["call"] = {
                "workload": f"{args.arch} @ {args.size}x{args.size}, batch {args.batch}, {args.precision}, T = {args.timesteps}: DPM-Solver++ (2M) with "
                            f"25 levels and DDIM with 250 steps (eta 0), the same weights read as eps (the fused step kernels) and as v "
                            f"(eod_param_pred, then the _p0 step)",
                **{k + "_s": stat(v) for k, v in tw.items()},
                "ratio_dpm_v_over_eps": round(med(tw["dpm_v"]) / med(tw["dpm_eps"]), 4),
                "ratio_ddim_v_over_eps": round(med(tw["ddim_v"]) / med(tw["ddim_eps"]), 4),
                "eps_spread": {w: round((max(tw[w + "_eps"]) - min(tw[w + "_eps"])) / med(tw[w + "_eps"]), 4) for w in ("dpm", "ddim")},
                "per_evaluation_extra_us": {"dpm": round((med(tw["dpm_v"]) - med(tw["dpm_eps"])) / 25 * 1e6, 1),
                                            "ddim": round((med(tw["ddim_v"]) - med(tw["ddim_eps"])) / 250 * 1e6, 1)},
                "finite": {k: bool(torch.isfinite(o).all()) for k, o in last.items()},
            }
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
