#!/usr/bin/env python3
"""What learned variance costs (DESIGN.md sections 8.3 and 9.17).  Nothing here is a gate.

One process, profiler off, the arms alternating:
  (1) kernels, HIP events around back-to-back launches, at 16 x 3 x 64 x 64, 16 x 3 x 256 x 256 and 1 x 4 x 2048 x 2048, each next to its
      neighbour with the byte model of the pair:
        eod_ddpm_var_pred     / eod_ddpm_pred_x0    1.0   (x, mean half, p0 against x, e, p0; the variance half is not read)
        eod_ddpm_step_p0_var  / eod_ddpm_step_p0    5/4   (x, p0, z, v, out against x, p0, z, out)
        eod_hybrid_loss       / eod_diffusion_loss  7/3   (o twice over, target, x_0, x_t, grad twice over against pred, target, dpred)
      Reported per kernel: time / (the neighbour's time x byte ratio);
      and eod_hybrid_loss with every sample at t = 0 (the erfc branch) and without the gradient (5/7 of the bytes, the same arithmetic);
  (2) the calls: a whole ancestral `sampling` call with the 2 C head against the C-head call on the same architecture, and a training step
      (forward, loss, backward, AdamW) under HybridLoss against DiffusionLoss("l2"), alternating, a host clock around a call that ends in a
      synchronise, after a warm-up of each.

    python tools/var_bench.py [--arch A0] [--size 64] [--batch 16] [--timesteps 1000] [--reps 5] [--no-call] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bench import ARCHS  # noqa: E402
from eo_diffusion_amd import _lib, optim  # noqa: E402
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


def build(arch, size, precision, dev, timesteps, learned):
    """bench.build_model with a head of C or 2 C channels"""
    from eo_diffusion_amd.backbones.unet_openai import UNetModel
    from eo_diffusion_amd.diffusion.model import EODiffusion
    torch.manual_seed(0)
    u = UNetModel(size, in_channels=3, out_channels=6 if learned else 3, **ARCHS[arch]).set_precision(precision)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for p in u.parameters():
            if p.dim() > 1 and float(p.abs().max()) == 0.0:
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    return EODiffusion(u, timesteps=timesteps, image_size=size, in_channels=3, device=str(dev), learned_variance=learned).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="A0")
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--precision", default="fp32x3")
    ap.add_argument("--train-precision", default="fp16")
    ap.add_argument("--timesteps", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5, help="alternations")
    ap.add_argument("--launches", type=int, default=50, help="back-to-back launches per timing")
    ap.add_argument("--no-call", action="store_true", help="kernels only")
    ap.add_argument("--out", default=None, help="the JSON object is written here, too (default: profiles/var_bench_<arch>_<size>_T<timesteps>.json)")
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", f"var_bench_{args.arch}_{args.size}_T{args.timesteps}.json")
    if not torch.cuda.is_available():
        raise SystemExit("var_bench.py measures on the GPU; there is nothing to time without one")
    dev = torch.device("cuda", 0)
    med = statistics.median
    L = _lib.lib()
    st = current_stream_ptr(dev)
    p = lambda t: 0 if t is None else t.data_ptr()
    res = {"kernels": []}
    from eo_diffusion_amd.diffusion.model import EODiffusion
    with torch.no_grad():
        sched = EODiffusion(torch.nn.Identity(), args.size, 3, timesteps=1000, learned_variance=True).to(dev)
        T, vt = sched.timesteps, sched.variance_tables()
        for N, C, edge in ((16, 3, 64), (16, 3, 256), (1, 4, 2048)):
            g = torch.Generator(device=dev).manual_seed(1)
            x, e, z, tgt = (torch.randn((N, C, edge, edge), device=dev, generator=g) for _ in range(4))
            x0 = torch.rand((N, C, edge, edge), device=dev, generator=g) * 2 - 1
            o = torch.randn((N, 2 * C, edge, edge), device=dev, generator=g)
            out, dp, grad = torch.empty_like(x), torch.empty_like(x), torch.empty_like(o)
            t = torch.randint(0, T, (N,), device=dev, generator=g)
            t[0] = 500
            t_pos, t_zero = t.clamp(min=1), torch.zeros_like(t)
            chw = C * edge * edge
            loss, per = torch.empty(1, device=dev), torch.empty(N, device=dev)
            vlb = torch.empty(N, dtype=torch.float64, device=dev)
            nb0, nb1 = L.eod_diffusion_loss_workspace_size(N, C, edge, edge), L.eod_hybrid_loss_workspace_size(N, C, edge, edge)
            ws = torch.empty(max(nb0, nb1) // 8, dtype=torch.float64, device=dev)
            s = sched
            arms = {
                "ddpm_pred_x0": lambda: L.eod_ddpm_pred_x0(p(x), p(e), p(t), p(s.alphas_cumprod), p(out), N, chw, T, 1, st),
                "ddpm_var_pred": lambda: L.eod_ddpm_var_pred(p(x), p(o), p(t), p(s.alphas_cumprod), 0, 0, 0, 1, p(out), N, chw, T, st),
                "ddpm_step_p0": lambda: L.eod_ddpm_step_p0(p(x), p(e), p(z), p(t_pos), p(s.betas), p(s.alphas), p(s.alphas_cumprod), p(out), N, chw, T, st),
                "ddpm_step_p0_var": lambda: L.eod_ddpm_step_p0_var(p(x), p(e), p(o), p(z), p(t_pos), p(s.betas), p(s.alphas), p(s.alphas_cumprod),
                                                                   p(vt["sigma_min"]), p(vt["half_gap"]), p(out), N, chw, T, st),
                "diffusion_loss": lambda: L.eod_diffusion_loss(p(e), p(tgt), 0, 0, 0, 0, N, C, edge, edge, 0, 1.0, p(loss), p(per), p(dp), p(ws), nb0, st),
                "hybrid_loss": lambda: L.eod_hybrid_loss(p(o), p(tgt), p(x0), p(x), p(t), 0, 0, 0, 0, p(s.sqrt_alphas_cumprod),
                                                         p(s.sqrt_one_minus_alphas_cumprod), p(vt["c1"]), p(vt["lmin"]), p(vt["gap"]), N, C, edge, edge, T, 0, 0,
                                                         1.0, 1e-3, 1.0 / 255.0, p(loss), p(per), p(vlb), p(grad), p(ws), nb1, st),
                # (every sample at t = 0: the erfc branch in place of the two exps -- if the float64 arithmetic binds, the time follows the branch)
                "hybrid_loss_t0": lambda: L.eod_hybrid_loss(p(o), p(tgt), p(x0), p(x), p(t_zero), 0, 0, 0, 0, p(s.sqrt_alphas_cumprod),
                                                            p(s.sqrt_one_minus_alphas_cumprod), p(vt["c1"]), p(vt["lmin"]), p(vt["gap"]), N, C, edge, edge, T, 0,
                                                            0, 1.0, 1e-3, 1.0 / 255.0, p(loss), p(per), p(vlb), p(grad), p(ws), nb1, st),
                "hybrid_loss_no_grad": lambda: L.eod_hybrid_loss(p(o), p(tgt), p(x0), p(x), p(t), 0, 0, 0, 0, p(s.sqrt_alphas_cumprod),
                                                                 p(s.sqrt_one_minus_alphas_cumprod), p(vt["c1"]), p(vt["lmin"]), p(vt["gap"]), N, C, edge, edge,
                                                                 T, 0, 0, 1.0, 1e-3, 1.0 / 255.0, p(loss), p(per), p(vlb), 0, p(ws), nb1, st),
            }
            for k, fn in arms.items():
                assert fn() == 0, (k, L.eod_last_error())
                timed(fn, 5)
            ts = {k: [] for k in arms}
            for _ in range(args.reps):
                for k, fn in arms.items():
                    ts[k].append(timed(fn, args.launches))
            m = {k: med(v) for k, v in ts.items()}
            pairs = (("ddpm_var_pred", "ddpm_pred_x0", 1.0), ("ddpm_step_p0_var", "ddpm_step_p0", 5 / 4), ("hybrid_loss", "diffusion_loss", 7 / 3))
            row = {"shape": [N, C, edge, edge], **{k + "_us": round(v * 1e3, 2) for k, v in m.items()},
                   "min_max_us": {k: [round(min(v) * 1e3, 2), round(max(v) * 1e3, 2)] for k, v in ts.items()},
                   "byte_ratio": {f"{a} / {b}": round(r, 4) for a, b, r in pairs},
                   "time_over_neighbour_x_byte_ratio": {a: round(m[a] / (m[b] * r), 3) for a, b, r in pairs},
                   "hybrid_loss_GB_per_s": round(7 * 4 * N * chw / (m["hybrid_loss"] * 1e-3) / 1e9, 1),
                   "hybrid_loss_ns_per_element": round(m["hybrid_loss"] * 1e6 / (N * chw), 4)}
            res["kernels"].append(row)
            print(json.dumps(row), flush=True)
        del sched
    if not args.no_call:
        shape = (args.batch, 3, args.size, args.size)
        models = {k: build(args.arch, args.size, args.precision, dev, args.timesteps, k == "var").eval() for k in ("plain", "var")}
        x_T = models["plain"]._philox(shape, dev, 2, 0, 0, 0)

        def wall(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out

        arms = {"sampling_" + k: (lambda m=m: m.sampling(args.batch, device=str(dev), x_T=x_T, rng="philox", seed=3, progress=False)) for k, m in models.items()}
        for fn in arms.values():
            wall(fn)
        tw, last = {k: [] for k in arms}, {}
        for _ in range(args.reps):
            for k, fn in arms.items():
                dt, last[k] = wall(fn)
                tw[k].append(dt)
        stat = lambda v: {"median": round(med(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        res["sampling"] = {"workload": f"{args.arch} @ {args.size}x{args.size}, batch {args.batch}, {args.precision}, T = {args.timesteps}: the ancestral call, "
                                       f"C head (eod_ddpm_step) against 2 C head (eod_ddpm_var_pred, eod_ddpm_step_p0_var)",
                           **{k + "_s": stat(v) for k, v in tw.items()},
                           "ratio_var_over_plain": round(med(tw["sampling_var"]) / med(tw["sampling_plain"]), 4),
                           "plain_spread": round((max(tw["sampling_plain"]) - min(tw["sampling_plain"])) / med(tw["sampling_plain"]), 4),
                           "per_evaluation_extra_us": round((med(tw["sampling_var"]) - med(tw["sampling_plain"])) / args.timesteps * 1e6, 1),
                           "finite": {k: bool(torch.isfinite(o).all()) for k, o in last.items()}}
        print(json.dumps(res["sampling"]), flush=True)
        del models
        # the training step
        train = {k: build(args.arch, args.size, args.train_precision, dev, 1000, k == "var").train() for k in ("plain", "var")}
        opts = {k: optim.AdamW(m.model.parameters(), lr=1e-5) for k, m in train.items()}
        losses = {"plain": optim.DiffusionLoss("l2"), "var": optim.HybridLoss(train["var"], "l2")}
        g = torch.Generator(device=dev).manual_seed(5)
        x = torch.rand(shape, device=dev, generator=g) * 2 - 1
        noise = torch.randn(shape, device=dev, generator=g)
        t = torch.randint(0, 1000, (args.batch,), device=dev, generator=g)

        def step(k):
            m, opt = train[k], opts[k]
            if k == "plain":
                pred, target = m(x, noise, t=t, return_target=True)
                loss = losses[k](pred, target)
            else:
                o, target, x_t, tt = m(x, noise, t=t, return_target=True, return_state=True)
                loss = losses[k](o, target, x, x_t, tt)
            loss.backward()
            opt.step()
            opt.zero_grad()
            return loss.detach()

        for k in train:
            for _ in range(3):
                wall(lambda k=k: step(k))
        tw = {k: [] for k in train}
        for _ in range(max(args.reps, 10)):
            for k in train:
                tw[k].append(wall(lambda k=k: step(k))[0])
        res["training_step"] = {"workload": f"{args.arch} @ {args.size}x{args.size}, batch {args.batch}, {args.train_precision}: forward, loss, backward, AdamW; "
                                            f"DiffusionLoss('l2') on a C head against HybridLoss on a 2 C head",
                                **{k + "_ms": {a: round(b * 1e3, 3) for a, b in stat(v).items()} for k, v in tw.items()},
                                "ratio_var_over_plain": round(med(tw["var"]) / med(tw["plain"]), 4)}
        print(json.dumps(res["training_step"]), flush=True)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
