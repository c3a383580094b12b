#!/usr/bin/env python3
"""Pansharpening with the sensors' physics: one DPM-Solver++ scene call with a panchromatic band seen through its own PSF and the
multispectral bands seen through theirs.

    python examples/pansharpen_psf.py                                   # 384 x 576, 4 bands at f = 4, MTF 0.3 at both Nyquist frequencies
    python examples/pansharpen_psf.py --pan-mtf 0.15 --mtf 0.25 --iters 24
    python examples/pansharpen_psf.py --damping 0.02                    # noisy observations: the regularised solve

A synthetic 4-band truth is "observed" twice.  The panchromatic band is a weighted sum of the bands blurred by the pan detector's PSF on
the full-resolution grid: psf_observe(truth, gaussian_psf(1, pan_mtf), 1, response=[pan weights]).  The multispectral bands are blurred by
their own PSF and sampled on an f x coarser grid: psf_observe(truth, gaussian_psf(f, mtf), f).  `observation=[PsfObservation(pan, ...,
response=...), PsfObservation(bands, ...)]`, both with solver="cg", projects every evaluation's prediction exactly onto each constraint in
turn (DESIGN.md sections 9.9 and 9.10): the band mix in front of the PSF factorises, so the pan constraint is one plane solve on the fine
grid.  The script prints both residuals, max |A x - y|, of the last prediction and of the returned scene, next to those of the same call
without an observation.  examples/pansharpen.py is the same task with ideal box averages in place of the PSFs.  The network is UNTRAINED
unless --ckpt is given: the script shows the mechanics and the constraints, not image quality.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eo_diffusion_amd.backbones.unet_openai import UNetModel  # noqa: E402
from eo_diffusion_amd.diffusion.consistency import PsfObservation, gaussian_psf, psf_observe  # noqa: E402
from eo_diffusion_amd.diffusion.dpm_solver import DPMSolverSampler  # noqa: E402
from eo_diffusion_amd.diffusion.model import EODiffusion  # noqa: E402

BANDS = 4


def synthetic_scene(h, w, seed):
    """[1, 4, h, w] in [0, 1]: smooth fields plus a fine texture the coarse bands cannot show"""
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
    ap.add_argument("--factor", type=int, default=4, help="the multispectral grid is this many times coarser (1 .. 8); divides height and width")
    ap.add_argument("--pan", type=float, nargs=BANDS, default=[0.25, 0.35, 0.25, 0.15], help="the panchromatic band's weight per band")
    ap.add_argument("--pan-mtf", type=float, default=0.3, help="the pan detector's MTF at the fine grid's Nyquist frequency")
    ap.add_argument("--mtf", type=float, default=0.3, help="the multispectral PSF's MTF at the coarse grid's Nyquist frequency")
    ap.add_argument("--iters", type=int, default=16, help="cg iterations (1 .. 64) per evaluation and link")
    ap.add_argument("--damping", type=float, default=0.0, help="the Tikhonov term of both solves")
    ap.add_argument("--image-size", type=int, default=64, help="the UNet's tile size")
    ap.add_argument("--overlap", type=int, default=16)
    ap.add_argument("--timesteps", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--precision", default="fp32x3", choices=["fp32", "fp32x3", "fp16"])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--out", default="pansharpened_psf_scene.npy")
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
    response, f = [args.pan], args.factor
    h_pan, h_ms = gaussian_psf(1, args.pan_mtf), gaussian_psf(f, args.mtf)
    pan = psf_observe(truth, h_pan, 1, response=response)              # [1, 1, H, W]: the panchromatic band through its PSF
    bands = psf_observe(truth, h_ms, f)                                # [1, 4, H / f, W / f]: what the multispectral sensor delivered
    kw = dict(iters=args.iters, solver="cg", damping=args.damping)
    links = [PsfObservation(pan, h_pan, 1, response=response, **kw), PsfObservation(bands, h_ms, f, **kw)]
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
    print(f"{args.height} x {args.width}, {BANDS} bands at f = {f} (MTF {args.mtf}, {h_ms.size} taps), pan = {args.pan} (MTF {args.pan_mtf}, "
          f"{h_pan.size} taps), {args.iters} cg iterations per evaluation and link{f', damping {args.damping}' if args.damping else ''}: "
          f"{sampler.num_evaluations} evaluations in {dt:.2f} s (the network is {'the checkpoint' if args.ckpt else 'UNTRAINED'})")
    for title, z in (("last prediction", inter["pred_x0"][-1]), ("returned scene", scene), ("without an observation: last prediction", free_inter["pred_x0"][-1]),
                     ("without an observation: returned scene", free)):
        r_pan = float((psf_observe(z, h_pan, 1, response=response) - pan).abs().max())
        r_ms = float((psf_observe(z, h_ms, f) - bands).abs().max())
        print(f"  {title}: max |A x - y|: pan {r_pan:.2e}, bands {r_ms:.2e}")
    print(f"  wrote {args.out}")
    if args.metrics:                                                   # (both in [-1, 1]: scored as reflectance-like [0, 1])
        from eo_diffusion_amd import metrics
        print(metrics.describe(metrics.quality(scene, truth, affine=(0.5, 0.5), ratio=args.factor), "returned scene against the truth"))


if __name__ == "__main__":
    main()
