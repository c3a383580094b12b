#!/usr/bin/env python3
"""What one tap vector per axis costs and buys.

One process, profiler off, the arms alternating:
  (1) kernels, HIP events around back-to-back launches, all channels observed on a scene-sized tensor (1 x 4 x 2048 x 2048) at f = 4:
      - the price of the general form: eod_psf_residual_xy / eod_psf_update_xy next to eod_psf_residual / eod_psf_update (the same library:
        the old kernels are untouched) at equal symmetric Gaussian taps, r = 6 and r = 12;
      - what the per-axis halo buys: the _xy pair at (ry, rx) = (12, 2) and (2, 12) next to (12, 12);
  (2) the call: a 25-evaluation `DPMSolverSampler.sample` with a 2-link PSF chain (bands 0, 1 at f = 2; band 2 at f = 4) under
      SeparablePsf(gaussian_psf(f)) next to the same chain under the bare taps gaussian_psf(f) and the call without an observation,
      alternating, timed by a host clock around a call that ends in a synchronise, after a warm-up call of each; the two chains must
      return the same bits.  A third chain, anisotropic and shifted (MTF 0.3 along y, 0.5 along x, +-0.37 f), is timed beside them.

    python tools/psf_xy_bench.py [--arch A0] [--size 64] [--batch 16] [--steps 25] [--reps 5] [--no-call] [--out FILE]

With --against LIB (another build of libeodiff.so, e.g. tools/build_lib_at.sh <commit> parent -> scratch/altlib/libeodiff_parent.so) it
does one thing instead: LIB is loaded into this process beside the tree's library and the same entry points of both are timed on the same
tensors, arms alternating (the bare pair and the _mix pair with K = 4 at r = 6 and r = 12, the _xy pair at (12, 12) and (12, 2)).  Per
arm: new / LIB median, LIB's own spread (max - min) / median in this run, and whether the two libraries wrote the same bits; an arm passes
when the ratio exceeds 1 by no more than that spread and the bits are equal.  The default --out is then profiles/psf_against.json.
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


def against(args, dev):
    """the PSF entry points of this tree's library next to those of args.against, in one process"""
    from eo_diffusion_amd.diffusion.consistency import SeparablePsf, gaussian_psf, psf_tau
    L, old = _lib.lib(), ctypes.CDLL(os.path.abspath(args.against))
    for name, (res, argtypes) in _lib.SYMBOLS.items():
        if name.startswith("eod_psf_") or name == "eod_last_error":
            fn = getattr(old, name)
            fn.restype, fn.argtypes = res, argtypes
    st = current_stream_ptr(dev)
    p = lambda t: t.data_ptr()
    floats = lambda h: (ctypes.c_float * h.size)(*h.ravel().tolist())
    B, C, f, H, W = 1, 4, 4, 2048, 2048
    K = C
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn((B, C, H, W), device=dev, generator=g)
    cvals = torch.randn((B, K, H // f, W // f), device=dev, generator=g)
    qin, q, out = cvals.clone(), torch.empty_like(cvals), torch.empty_like(x)      # both libraries read and write the SAME tensors: no arm is
                                                                                   # timed on another allocation than the arm it is compared with
    chans = (ctypes.c_int32 * C)(*range(C))
    R = floats(torch.randn((K, C), generator=torch.Generator().manual_seed(2)).numpy())
    G = floats(torch.randn((C, K), generator=torch.Generator().manual_seed(3)).numpy())
    arms = {}                                                         # name -> the call of one library: (rc, the tensor it wrote)
    for r in (6, 12):
        h = gaussian_psf(f, 0.3, radius=r)
        t, step = floats(h), psf_tau(h, f, H, W) / (f * f)
        arms[f"psf_residual r={r}"] = lambda lib, t=t, r=r: (lib.eod_psf_residual(p(x), p(cvals), 0, 1.0, t, r, f, chans, C, B, C, H, W, 0, 0, 0, p(q), st), q)
        arms[f"psf_update r={r}"] = lambda lib, t=t, r=r, step=step: (lib.eod_psf_update(p(x), p(qin), step, t, r, f, chans, C, B, C, H, W, p(out), st), out)
        arms[f"psf_residual_mix r={r}"] = lambda lib, t=t, r=r: (lib.eod_psf_residual_mix(p(x), p(cvals), 0, 1.0, t, r, f, R, K, B, C, H, W, 0, 0, p(q), st), q)
        arms[f"psf_update_mix r={r}"] = lambda lib, t=t, r=r, step=step: (lib.eod_psf_update_mix(p(x), p(qin), step, t, r, f, G, K, B, C, H, W, p(out), st), out)
    for ry, rx in ((12, 12), (12, 2)):
        hy, hx = gaussian_psf(f, 0.3, radius=ry), gaussian_psf(f, 0.3, radius=rx)
        ty, tx, step = floats(hy), floats(hx), psf_tau(SeparablePsf(hx, hy), f, H, W) / (f * f)
        arms[f"psf_residual_xy ({ry}, {rx})"] = lambda lib, ty=ty, tx=tx, ry=ry, rx=rx: (
            lib.eod_psf_residual_xy(p(x), p(cvals), 0, 1.0, ty, ry, tx, rx, f, chans, None, C, B, C, H, W, 0, 0, 0, p(q), st), q)
        arms[f"psf_update_xy ({ry}, {rx})"] = lambda lib, ty=ty, tx=tx, ry=ry, rx=rx, step=step: (
            lib.eod_psf_update_xy(p(x), p(qin), step, ty, ry, tx, rx, f, chans, None, C, B, C, H, W, p(out), st), out)
    us = lambda v: round(v * 1e3, 2)
    rows = []
    for name, arm in arms.items():
        wrote = []
        for lib in (L, old):                                          # warm-up of each arm, and the bits
            rc, dst = arm(lib)
            assert rc == 0, lib.eod_last_error()
            wrote.append(dst.clone())
            dst.fill_(float("nan"))
            timed(lambda: arm(lib), 5)
        same = bool(torch.equal(*wrote))
        ts = {L: [], old: []}
        for rep in range(args.reps):                                  # the libraries alternate, and so does which of them goes first
            for lib in ((L, old) if rep % 2 == 0 else (old, L)):
                ts[lib].append(timed(lambda: arm(lib), args.launches))
        m_new, m_old = statistics.median(ts[L]), statistics.median(ts[old])
        spread = (max(ts[old]) - min(ts[old])) / m_old
        row = {"arm": name, "shape": [B, C, H, W], "f": f, "K": K, "new_us": us(m_new), "against_us": us(m_old), "new_over_against": round(m_new / m_old, 4),
               "against_spread": round(spread, 4), "new_min_max_us": [us(min(ts[L])), us(max(ts[L]))], "against_min_max_us": [us(min(ts[old])), us(max(ts[old]))],
               "same_bits": same, "pass": bool(same and m_new / m_old <= 1.0 + spread)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return {"against": os.path.basename(args.against), "launches": args.launches, "reps": args.reps, "arms": rows, "pass": all(r["pass"] for r in rows)}


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
    ap.add_argument("--against", default=None, metavar="LIB", help="another build of libeodiff.so: time its PSF entry points next to this tree's, nothing else")
    ap.add_argument("--out", default=None, help="the JSON object is written here, too (default: profiles/psf_xy_bench_<arch>_<size>_T<timesteps>.json)")
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", "psf_against.json" if args.against else f"psf_xy_bench_{args.arch}_{args.size}_T{args.timesteps}.json")
    if not torch.cuda.is_available():
        raise SystemExit("psf_xy_bench.py measures on the GPU; there is nothing to time without one")
    if args.against:
        with torch.no_grad():
            res = against(args, torch.device("cuda", 0))
        line = json.dumps(res)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
        return
    from eo_diffusion_amd.diffusion.consistency import PsfObservation, SeparablePsf, gaussian_psf, psf_observe, psf_tau
    from eo_diffusion_amd.diffusion.dpm_solver import DPMSolverSampler
    dev = torch.device("cuda", 0)
    med = statistics.median
    L = _lib.lib()
    res = {"kernels": []}
    st = current_stream_ptr(dev)
    p = lambda t: 0 if t is None else t.data_ptr()
    floats = lambda h: (ctypes.c_float * h.size)(*h.tolist())
    us = lambda v: round(v * 1e3, 2)
    with torch.no_grad():
        B, C, f = 1, 4, 4
        H = W = 2048
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.randn((B, C, H, W), device=dev, generator=g)
        cvals = torch.randn((B, C, H // f, W // f), device=dev, generator=g)
        q, out = torch.empty_like(cvals), torch.empty_like(x)
        q2, out2 = torch.empty_like(cvals), torch.empty_like(x)
        chans = (ctypes.c_int32 * C)(*range(C))

        def pair(hy, hx, old=False):
            ty, tx, ry, rx = floats(hy), floats(hx), hy.size // 2, hx.size // 2
            step = psf_tau(SeparablePsf(hx, hy), f, H, W) / (f * f)
            if old:
                return (lambda: L.eod_psf_residual(p(x), p(cvals), 0, 1.0, tx, rx, f, chans, C, B, C, H, W, 0, 0, 0, p(q), st),
                        lambda: L.eod_psf_update(p(x), p(q), step, tx, rx, f, chans, C, B, C, H, W, p(out), st))
            return (lambda: L.eod_psf_residual_xy(p(x), p(cvals), 0, 1.0, ty, ry, tx, rx, f, chans, None, C, B, C, H, W, 0, 0, 0, p(q2), st),
                    lambda: L.eod_psf_update_xy(p(x), p(q), step, ty, ry, tx, rx, f, chans, None, C, B, C, H, W, p(out2), st))

        def measure(arms):
            for fn in arms.values():
                assert fn() == 0, L.eod_last_error()
                timed(fn, 5)
            ts = {k: [] for k in arms}
            for _ in range(args.reps):                                # the arms alternate
                for k, fn in arms.items():
                    ts[k].append(timed(fn, args.launches))
            return ts

        for r in (6, 12):                                             # the price of the general form
            h = gaussian_psf(f, 0.3, radius=r)
            (r_old, u_old), (r_xy, u_xy) = pair(h, h, old=True), pair(h, h)
            ts = measure({"psf_residual": r_old, "psf_residual_xy": r_xy, "psf_update": u_old, "psf_update_xy": u_xy})
            torch.cuda.synchronize()
            m = {k: med(v) for k, v in ts.items()}
            row = {"what": "equal symmetric taps", "shape": [B, C, H, W], "f": f, "ry": r, "rx": r, **{k + "_us": us(v) for k, v in m.items()},
                   "min_max_us": {k: [us(min(v)), us(max(v))] for k, v in ts.items()},
                   "spread_old_pair": round(max((max(ts[k]) - min(ts[k])) / m[k] for k in ("psf_residual", "psf_update")), 4),
                   "xy_over_old_residual": round(m["psf_residual_xy"] / m["psf_residual"], 4), "xy_over_old_update": round(m["psf_update_xy"] / m["psf_update"], 4),
                   "xy_over_old_pair": round((m["psf_residual_xy"] + m["psf_update_xy"]) / (m["psf_residual"] + m["psf_update"]), 4),
                   "same_bits": bool(torch.equal(q, q2) and torch.equal(out, out2))}
            res["kernels"].append(row)
            print(json.dumps(row), flush=True)
        arms = {}                                                     # what the per-axis halo buys
        for ry, rx in ((12, 12), (12, 2), (2, 12)):
            rr, uu = pair(gaussian_psf(f, 0.3, radius=ry), gaussian_psf(f, 0.3, radius=rx))
            arms[f"residual_{ry}_{rx}"], arms[f"update_{ry}_{rx}"] = rr, uu
        ts = measure(arms)
        m = {k: med(v) for k, v in ts.items()}
        pair_us = {k: m[f"residual_{k}"] + m[f"update_{k}"] for k in ("12_12", "12_2", "2_12")}
        row = {"what": "per-axis halo", "shape": [B, C, H, W], "f": f, **{k + "_us": us(v) for k, v in m.items()},
               "min_max_us": {k: [us(min(v)), us(max(v))] for k, v in ts.items()},
               "pair_us": {k: us(v) for k, v in pair_us.items()},
               "pair_over_12_12": {k: round(v / pair_us["12_12"], 4) for k, v in pair_us.items()}}
        res["kernels"].append(row)
        print(json.dumps(row), flush=True)
        if not args.no_call:
            m = build_model(args.arch, args.size, args.precision, dev, timesteps=args.timesteps)
            shape = (3, args.size, args.size)
            x_T = m._philox((args.batch,) + shape, dev, 1, 0, args.timesteps, 0)
            truth = torch.tanh(m._philox((args.batch,) + shape, dev, 2, 0, 0, 0))
            groups = (((0, 1), 2), ((2,), 4))
            bare = [gaussian_psf(f) for _, f in groups]
            sep = [SeparablePsf(h) for h in bare]
            skew = [SeparablePsf(gaussian_psf(f, 0.5, shift=-0.37 * f), gaussian_psf(f, 0.3, shift=0.37 * f)) for _, f in groups]
            chain = lambda psfs: [PsfObservation(psf_observe(truth, h, f, cs), h, f, cs, iters=1) for (cs, f), h in zip(groups, psfs)]
            dpm = DPMSolverSampler(m)
            call = lambda **kw: dpm.sample(args.steps, args.batch, shape, x_T=x_T, clip_denoised=True, progress=False, **kw)
            arms = {"plain": call, "bare_taps": lambda: call(observation=chain(bare)), "separable_same_taps": lambda: call(observation=chain(sep)),
                    "separable_anisotropic_shifted": lambda: call(observation=chain(skew))}

            def wall(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                o = fn()
                torch.cuda.synchronize()
                return time.perf_counter() - t0, o

            for fn in arms.values():
                wall(fn)
            tw, last = {k: [] for k in arms}, {}
            for _ in range(args.reps):
                for k, fn in arms.items():
                    dt, (o, inter) = wall(fn)
                    tw[k].append(dt)
                    last[k] = o
            stat = lambda v: {"median": round(med(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
            res["call"] = {
                "workload": f"{args.arch} @ {args.size}x{args.size}, batch {args.batch}, {args.precision}, T = {args.timesteps}: DPM-Solver++ 2M, "
                            f"S = {args.steps} ({dpm.num_evaluations} evaluations), clip, PSF chain [bands 0, 1 at f = 2; band 2 at f = 4], iters 1, weights 1",
                **{k + "_s": stat(v) for k, v in tw.items()},
                "plain_spread": round((max(tw["plain"]) - min(tw["plain"])) / med(tw["plain"]), 4),
                "separable_over_bare": round(med(tw["separable_same_taps"]) / med(tw["bare_taps"]), 4),
                "anisotropic_over_bare": round(med(tw["separable_anisotropic_shifted"]) / med(tw["bare_taps"]), 4),
                "bare_over_plain": round(med(tw["bare_taps"]) / med(tw["plain"]), 4),
                "same_bits_bare_and_separable": bool(torch.equal(last["bare_taps"], last["separable_same_taps"])),
                "finite": bool(all(torch.isfinite(z).all() for z in last.values())),
            }
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
