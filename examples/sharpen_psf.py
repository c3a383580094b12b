#!/usr/bin/env python3
"""Sharpening the coarse bands of a Sentinel-2-like stack against the sensor's point spread function: one DPM-Solver++ scene call with two
PSF-aware observations.

    python examples/sharpen_psf.py                                     # 384 x 576, 13 bands, MTF 0.3 at Nyquist
    python examples/sharpen_psf.py --mtf 0.2 --iters 4 --steps 25
    python examples/sharpen_psf.py --solver cg --iters 16                # the exact projection: the residuals fall to rounding
    python examples/sharpen_psf.py --solver cg --iters 8 --damping 0.05  # the regularised solve for noisy observations
    python examples/sharpen_psf.py --mtf-along 0.2 --mtf-across 0.35 --shift 0.3 --solver cg --iters 16  # an anisotropic PSF, the coarse bands 0.3 coarse pixels off the grid

A synthetic 13-band truth is "observed" the way the instrument does it: the six 20 m bands (B5, B6, B7, B8A, B11, B12) blurred by a Gaussian
PSF and sampled on a 2x coarser grid, the three 60 m bands (B1, B9, B10) on a 6x coarser one, each group with the PSF of its own grid
(gaussian_psf: the MTF at that grid's Nyquist frequency).  `observation=[PsfObservation(20 m group), PsfObservation(60 m group)]` takes
`iters` Landweber steps toward each constraint set after every evaluation's prediction, or with --solver cg `iters`
conjugate-gradient iterations of the exact projection onto it (section 9.9); the 10 m bands are left to the network.  The script prints both residuals, max |A x - y| on the coarse grids, of the last prediction and of the returned scene, next to
those of the same call without an observation.  The network is UNTRAINED unless --ckpt is given: the script shows the mechanics and the
constraints, not image quality.  --mtf-along / --mtf-across give the PSF one MTF per axis (along-track: y, across-track: x) and --shift
registers the coarse bands that fraction of a COARSE pixel off the fine grid along both axes (SeparablePsf, gaussian_psf(shift=); section
9.11); without them the call and its output are the ones above.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eo_diffusion_amd.backbones.unet_openai import UNetModel  # noqa: E402
from eo_diffusion_amd.diffusion.consistency import PsfObservation, SeparablePsf, gaussian_psf, psf_observe  # noqa: E402
from eo_diffusion_amd.diffusion.dpm_solver import DPMSolverSampler  # noqa: E402
from eo_diffusion_amd.diffusion.model import EODiffusion  # noqa: E402

BANDS = 13                                  # B1 B2 B3 B4 B5 B6 B7 B8 B8A B9 B10 B11 B12
GROUPS = {"20 m": ((4, 5, 6, 8, 11, 12), 2), "60 m": ((0, 9, 10), 6)}


def synthetic_scene(h, w, seed):
    """[1, 13, h, w] in [0, 1]: smooth fields plus a fine texture the coarse bands cannot show"""
    r = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.zeros((BANDS, h, w), np.float32)
    for c in range(BANDS):
        for _ in range(4):
            fy, fx, ph = r.uniform(0.002, 0.02), r.uniform(0.002, 0.02), r.uniform(0, 6.28)
            img[c] += np.sin(fy * yy + fx * xx + ph)
        img[c] += 0.3 * np.sin(0.9 * yy + r.uniform(0, 6.28)) * np.sin(0.7 * xx + r.uniform(0, 6.28))
    img = (img - img.min()) / (img.max() - img.min())
    return torch.from_numpy(img)[None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=576)
    ap.add_argument("--mtf", type=float, default=0.3, help="the PSF's MTF at each coarse grid's Nyquist frequency")
    ap.add_argument("--mtf-along", type=float, default=None, help="the MTF along y (along-track) in the place of --mtf: a SeparablePsf")
    ap.add_argument("--mtf-across", type=float, default=None, help="the MTF along x (across-track) in the place of --mtf: a SeparablePsf")
    ap.add_argument("--shift", type=float, default=None, help="misregistration of the coarse bands in COARSE pixels along both axes, |shift| <= 0.5: a SeparablePsf")
    ap.add_argument("--iters", type=int, default=2, help="Landweber steps (1 .. 8) or cg iterations (1 .. 64) per evaluation and link")
    ap.add_argument("--solver", default="landweber", choices=["landweber", "cg"])
    ap.add_argument("--damping", type=float, default=0.0, help="--solver cg: the Tikhonov term mu of (A A^T + mu I)")
    ap.add_argument("--image-size", type=int, default=64, help="the UNet's tile size")
    ap.add_argument("--overlap", type=int, default=16)
    ap.add_argument("--timesteps", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--precision", default="fp32x3", choices=["fp32", "fp32x3", "fp16"])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--out", default="sharpened_psf_scene.npy")
    ap.add_argument("--metrics", action="store_true", help="score the returned scene against the synthetic truth (eo_diffusion_amd.metrics.quality)")
    args = ap.parse_args()
    device = "cuda:0"
    torch.manual_seed(args.seed)
    unet = UNetModel(args.image_size, in_channels=BANDS, model_channels=64, out_channels=BANDS, channel_mult=[1, 2, 3], attention_resolutions=[],
                     num_res_blocks=1, num_heads=1).set_precision(args.precision)
    model = EODiffusion(unet, timesteps=args.timesteps, image_size=args.image_size, in_channels=BANDS, device=device)
    if args.ckpt:
        model.load_state_dict(torch.load(args.ckpt, map_location="cpu")["model"])
    else:
        with torch.no_grad():  # the reference zero-initialises the output convs: give the untrained network something to say
            for p in unet.parameters():
                if p.dim() > 1 and float(p.abs().max()) == 0.0:
                    p.normal_(0.0, 0.02)
    model = model.to(device).eval()
    truth = synthetic_scene(args.height, args.width, args.seed).to(device) * 2.0 - 1.0
    if args.mtf_along is None and args.mtf_across is None and args.shift is None:
        psf_of = lambda f: gaussian_psf(f, args.mtf)
    else:                                       # one tap vector per axis: anisotropic and / or shifted
        along, across, shift = args.mtf_along or args.mtf, args.mtf_across or args.mtf, args.shift or 0.0
        psf_of = lambda f: SeparablePsf(gaussian_psf(f, across, shift=shift * f), gaussian_psf(f, along, shift=shift * f))
    seen = {name: (cs, f, psf_of(f)) for name, (cs, f) in GROUPS.items()}
    values = {name: psf_observe(truth, h, f, cs) for name, (cs, f, h) in seen.items()}          # what the sensor delivered, on the coarse grids
    links = [PsfObservation(values[name], h, f, cs, iters=args.iters, solver=args.solver, damping=args.damping) for name, (cs, f, h) in seen.items()]
    sampler = DPMSolverSampler(model)
    x_T = torch.randn((1, BANDS, args.height, args.width), device=device)
    call = lambda **kw: sampler.sample_scene(args.steps, (args.height, args.width), overlap=args.overlap, clip_denoised=False, progress=False,
                                             x_T=x_T, **kw)
    free, free_inter = call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    scene, inter = call(observation=links)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    np.save(args.out, ((scene + 1.0) / 2.0)[0].cpu().numpy())
    print(f"{args.height} x {args.width}, {BANDS} bands, MTF {args.mtf} at Nyquist, {args.iters} "
          f"{'cg iteration(s)' if args.solver == 'cg' else 'Landweber step(s)'} per evaluation"
          f"{f', damping {args.damping}' if args.damping else ''}: "
          f"{sampler.num_evaluations} evaluations in {dt:.2f} s (the network is {'the checkpoint' if args.ckpt else 'UNTRAINED'})")
    for name, (cs, f, h) in seen.items():
        taps = f"{h.taps_y.size} x {h.taps_x.size}" if isinstance(h, SeparablePsf) else str(h.size)
        print(f"  {name} group: channels {list(cs)} at f = {f}, {taps} taps")
    for title, z in (("last prediction", inter["pred_x0"][-1]), ("returned scene", scene), ("without an observation: last prediction", free_inter["pred_x0"][-1]),
                     ("without an observation: returned scene", free)):
        res = ", ".join(f"{name} {float((psf_observe(z, h, f, cs) - values[name]).abs().max()):.2e}" for name, (cs, f, h) in seen.items())
        print(f"  {title}: max |A x - y|: {res}")
    print(f"  wrote {args.out}")
    if args.metrics:                                                   # (both in [-1, 1]: scored as reflectance-like [0, 1])
        from eo_diffusion_amd import metrics
        print(metrics.describe(metrics.quality(scene, truth, affine=(0.5, 0.5), ratio=min(f for _, f in GROUPS.values())), "returned scene against the truth"))


if __name__ == "__main__":
    main()
