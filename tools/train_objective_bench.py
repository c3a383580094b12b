#!/usr/bin/env python3
"""What the masked / weighted loss and gradient clipping cost.

One process, profiler off, the arms alternating:
  (1) eod_diffusion_loss next to eod_mse_loss, HIP events around back-to-back calls, at 16 x 3 x 256^2 and 2 x 13 x 512^2: no mask (huber),
      a one-channel mask and a full mask.  Byte model: pred, target and dpred once each = 3 tensors for both; the mask adds its own size
      twice (the count pass and the fused pass): 3 + 2/C tensors with a one-channel mask, 5 with a full one;
  (2) eod_grad_sumsq + eod_adamw_step_clipped next to eod_adamw_step_guarded on the model's parameter count: both read g twice (the scan,
      the update) and read and write p, m, v once = 8 tensors, ratio 1; the scan of the clipped step adds two float64 operations per element;
  (3) a whole training step (the shape of tools/train_bench.py: q_sample, UNetTrainer forward, loss, backward, optimizer) with
      optim.mse_loss + AdamW() -- the step as it was before this objective existed: neither entry point changed -- against
      diffusion_loss("huber") with a blob mask and min-SNR weights + AdamW(max_grad_norm=1.0), host clock around steps that end in a
      synchronise, the two alternating.

    python tools/train_objective_bench.py [--arch A0] [--size 64] [--batch 16] [--precision fp16] [--steps 10] [--reps 3] [--no-step] [--out FILE]
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
from eo_diffusion_amd import _lib, optim  # noqa: E402
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


def alternate(forms, reps, rounds=5):
    """{form: [ms per call] over `rounds` alternating rounds}, after a checked call and a warm-up of every form"""
    for name, fn in forms.items():
        assert fn() == 0, name
        timed(fn, 10)
    ts = {form: [] for form in forms}
    for _ in range(rounds):
        for form, fn in forms.items():
            ts[form].append(timed(fn, reps))
    return ts


def blob_mask(n, c, h, w, dev, seed=3):
    """a synthetic cloud per chip: 0 inside a disc, 1 outside"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    m = torch.ones((n, c, h, w))
    for k in range(n):
        cy, cx, rad = (float(v) for v in torch.rand(3, generator=g))
        m[k, :, (yy - cy * h) ** 2 + (xx - cx * w) ** 2 < ((0.2 + 0.2 * rad) * h) ** 2] = 0.0
    return m.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="A0")
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--steps", type=int, default=10, help="training steps per timed run")
    ap.add_argument("--reps", type=int, default=3, help="alternations of the two step forms")
    ap.add_argument("--no-step", action="store_true", help="kernels only")
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_objective_bench.py measures on the GPU; there is nothing to time without one")
    dev = torch.device("cuda", 0)
    med = statistics.median
    L = _lib.lib()
    st = current_stream_ptr(dev)
    p = lambda t: 0 if t is None else t.data_ptr()
    stat = lambda t, moved: {"us": round(med(t) * 1e3, 2), "min_us": round(min(t) * 1e3, 2), "max_us": round(max(t) * 1e3, 2),
                             "GB_per_s": round(moved / (med(t) * 1e-3) / 1e9, 1)}
    res = {"loss": {}}
    # ---- (1) the loss
    for name, (N, C, H, W) in (("16x3x256", (16, 3, 256, 256)), ("2x13x512", (2, 13, 512, 512))):
        pred, target = torch.randn((N, C, H, W), device=dev), torch.randn((N, C, H, W), device=dev)
        m1, mc = blob_mask(N, 1, H, W, dev), blob_mask(N, C, H, W, dev)
        weight = torch.rand(N, device=dev) + 0.5
        loss, per, dp = torch.empty(1, device=dev), torch.empty(N, device=dev), torch.empty_like(pred)
        scr = torch.empty(1024, device=dev)
        nws = L.eod_diffusion_loss_workspace_size(N, C, H, W)
        ws = torch.empty(nws // 8, dtype=torch.float64, device=dev)

        def dl(mask, kind, w=None):
            return lambda: L.eod_diffusion_loss(p(pred), p(target), p(mask), 0 if mask is None else mask.shape[0], 0 if mask is None else mask.shape[1], p(w),
                                                N, C, H, W, kind, 1.0, p(loss), p(per), p(dp), p(ws), nws, st)
        forms = {"mse_loss": lambda: L.eod_mse_loss(p(pred), p(target), pred.numel(), p(loss), p(dp), p(scr), 1024, st),
                 "l2_no_mask": dl(None, 0), "huber_no_mask": dl(None, 2, weight), "huber_mask_1ch": dl(m1, 2, weight), "huber_mask_full": dl(mc, 2, weight)}
        ts = alternate(forms, 100)
        tensor = pred.numel() * 4
        moved = {"mse_loss": 3 * tensor, "l2_no_mask": 3 * tensor, "huber_no_mask": 3 * tensor, "huber_mask_1ch": 3 * tensor + 2 * m1.numel() * 4,
                 "huber_mask_full": 5 * tensor}
        row = {"shape": [N, C, H, W]}
        for form, t in ts.items():
            row[form] = stat(t, moved[form])
            if form != "mse_loss":
                row[form]["ratio_over_mse"] = round(med(t) / med(ts["mse_loss"]), 3)
                row[form]["byte_model_ratio"] = round(moved[form] / moved["mse_loss"], 3)
        res["loss"][name] = row
    # ---- (2) the optimizer step on the model's parameter count
    model = build_model(args.arch, args.size, args.precision, dev)
    n = sum((q.numel() + 3) // 4 * 4 for q in model.model.parameters())
    P, M, V = (torch.randn(n, device=dev) * s for s in (1.0, 0.01, 1e-3))
    V.abs_()
    G = torch.randn(n, device=dev) * 0.01
    guard, clip, scratch = torch.zeros(4, dtype=torch.int32, device=dev), torch.zeros(10, dtype=torch.int32, device=dev), torch.zeros(8192, dtype=torch.int32, device=dev)
    sumsq = torch.zeros(1, dtype=torch.float64, device=dev)
    nslots = L.eod_grad_sumsq_workspace_size(optim.SUMSQ_SLOTS)
    slots = torch.zeros(nslots // 8, dtype=torch.float64, device=dev)
    calls = [0, 0]

    def guarded():
        calls[0] += 1
        return L.eod_adamw_step_guarded(p(P), p(G), p(M), p(V), n, 1e-4, 0.9, 0.999, 1e-8, 0.01, calls[0], p(guard), p(scratch), 8192, st)

    def clipped():
        calls[1] += 1
        return L.eod_grad_sumsq(p(G), n, p(sumsq), p(slots), nslots, optim.SUMSQ_SLOTS, st) or \
            L.eod_adamw_step_clipped(p(P), p(G), p(M), p(V), n, 1e-4, 0.9, 0.999, 1e-8, 0.01, calls[1], 1.0, p(sumsq), 1, p(clip), st)
    forms = {"guarded": guarded, "clipped": clipped, "sumsq_scan_alone": lambda: L.eod_grad_sumsq(p(G), n, p(sumsq), p(slots), nslots, optim.SUMSQ_SLOTS, st)}
    ts = alternate(forms, 50)
    res["adamw"] = {"parameters": n, "guarded": stat(ts["guarded"], 8 * 4 * n), "clipped": stat(ts["clipped"], 8 * 4 * n),
                    "sumsq_scan_alone": stat(ts["sumsq_scan_alone"], 4 * n), "ratio_clipped_over_guarded": round(med(ts["clipped"]) / med(ts["guarded"]), 3),
                    "byte_model_ratio": 1.0, "scan_slots": optim.SUMSQ_SLOTS, "coef": float(clip[6:7].view(torch.float32)[0]), "norm": float(clip[8:10].view(torch.float64)[0])}
    del P, M, V, G
    # ---- (3) the whole step
    if not args.no_step:
        from eo_diffusion_amd.training import UNetTrainer
        B, S = args.batch, args.size
        x, noise = torch.rand((B, 3, S, S), device=dev), torch.randn((B, 3, S, S), device=dev)
        t = torch.randint(0, 1000, (B,), device=dev)
        mask = blob_mask(B, 1, S, S, dev)
        weight = model.loss_weights("min_snr", 5.0)[t]
        unet = model.model.train()
        scale = 1024.0 if args.precision == "fp16" else 1.0
        # one optimizer for both arms (two would each move the parameters into a flat buffer of their own): max_grad_norm = None takes
        # exactly the guarded step's calls.  The two arms share the step counter, which only moves the bias corrections.
        opt = optim.AdamW(unet.parameters(), lr=1e-5, max_grad_norm=1.0)
        tr = UNetTrainer(unet, B, S, S, dev, loss_scale=scale)
        arms = {"mse_guarded": None, "huber_mask_minsnr_clip": 1.0}

        def step(arm):
            pred = tr.forward(model._forward_diffusion(x, t, noise), t)
            if arm == "mse_guarded":
                _, dpred = optim.mse_loss(pred, noise)
            else:
                _, dpred = optim.diffusion_loss(pred, noise, mask=mask, weight=weight, kind="huber")
            tr.backward(dpred)
            opt.max_grad_norm = arms[arm]
            opt.step()

        def run(arm):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(arm)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / args.steps
        for arm in arms:
            run(arm)
        tt = {arm: [] for arm in arms}
        for _ in range(args.reps):
            for arm in arms:
                tt[arm].append(run(arm))
        a, b = tt["mse_guarded"], tt["huber_mask_minsnr_clip"]
        res["step"] = {"workload": f"{args.arch} @ {S}x{S}, batch {B}, {args.precision}: q_sample, forward, loss, backward, optim.AdamW, {args.steps} steps per run",
                       "mse_guarded_ms": {"median": round(med(a) * 1e3, 3), "min": round(min(a) * 1e3, 3), "max": round(max(a) * 1e3, 3)},
                       "huber_mask_minsnr_clip_ms": {"median": round(med(b) * 1e3, 3), "min": round(min(b) * 1e3, 3), "max": round(max(b) * 1e3, 3)},
                       "mse_guarded_spread": round((max(a) - min(a)) / med(a), 4), "difference_ms": round((med(b) - med(a)) * 1e3, 3),
                       "ratio": round(med(b) / med(a), 4), "clipped_steps": opt.clipped_steps(), "skipped_steps": opt.skipped_steps(),
                       "last_grad_norm": opt.last_grad_norm()}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
