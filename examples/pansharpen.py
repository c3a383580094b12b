#!/usr/bin/env python3
"""Pansharpening as sampling: the multispectral bands are known on a 4x coarser grid, their weighted sum (a panchromatic band) at full
resolution; one DPM-Solver++ scene call with a chain of two observations.

    python examples/pansharpen.py                                      # 384 x 576, 4 bands at f = 4, pan = 0.25 0.35 0.25 0.15 of them
    python examples/pansharpen.py --pan 0.1 0.4 0.4 0.1 --factor 8 --steps 25

A synthetic truth is "observed" twice: every band as its mean over factor x factor blocks (an Observation), and a known mix of the bands at
full resolution (a SpectralObservation with a 1 x 4 response).  `observation=[pan, bands]` projects the data prediction of every evaluation
onto the first and then onto the second; both were made from one image, so the two projections commute and the
prediction meets both at once.  The script prints both residuals, of the last prediction and of the returned scene (which the last step
has moved on by a little).  The network is untrained unless --ckpt is given: the script shows the mechanics and the constraints, not image
quality.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eo_diffusion_amd.backbones.unet_openai import UNetModel  # noqa: E402
from eo_diffusion_amd.diffusion.consistency import Observation, SpectralObservation, block_mean, spectral_response  # noqa: E402
from eo_diffusion_amd.diffusion.dpm_solver import DPMSolverSampler  # noqa: E402
from eo_diffusion_amd.diffusion.model import EODiffusion  # noqa: E402

BANDS = 4


def synthetic_scene(h, w, seed):
    """[1, 4, h, w] in [0, 1]: smooth fields plus a fine texture the coarse bands cannot show -- stands in for a VHR tile"""
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
    ap.add_argument("--factor", type=int, default=4, help="the block edge of the multispectral bands (1 .. 8); divides height and width")
    ap.add_argument("--pan", type=float, nargs=BANDS, default=[0.25, 0.35, 0.25, 0.15], help="the panchromatic band's weight per band")
    ap.add_argument("--image-size", type=int, default=64, help="the UNet's tile size")
    ap.add_argument("--overlap", type=int, default=16)
    ap.add_argument("--timesteps", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--precision", default="fp32x3", choices=["fp32", "fp32x3", "fp16"])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--out", default="pansharpened_scene.npy")
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
    response, factors = [args.pan], [args.factor] * BANDS
    pan = spectral_response(truth, response)                           # [1, 1, H, W]: the panchromatic band, at full resolution
    bands = block_mean(truth, factors)                                 # [1, 4, H, W]: the coarse bands, replicated onto the fine grid
    sampler = DPMSolverSampler(model)
    t0 = time.perf_counter()
    scene, inter = sampler.sample_scene(args.steps, (args.height, args.width), overlap=args.overlap, clip_denoised=False, progress=False,
                                        observation=[SpectralObservation(pan, response), Observation(bands, factors)])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    np.save(args.out, ((scene + 1.0) / 2.0)[0].cpu().numpy())
    print(f"{args.height} x {args.width}, {BANDS} bands at f = {args.factor}, pan = {args.pan}: {sampler.num_evaluations} evaluations in {dt:.2f} s")
    for name, z in (("last prediction", inter["pred_x0"][-1]), ("returned scene", scene)):
        r_pan = float((spectral_response(z, response) - pan).abs().max())
        r_bands = float((block_mean(z, factors) - bands).abs().max())
        print(f"  {name}: max |pan of it - pan| = {r_pan:.2e}, max |block mean of it - bands| = {r_bands:.2e}")
    print(f"  sharpness the bands alone cannot give: max |scene - replicated bands| = {float((scene - bands).abs().max()):.2f}; wrote {args.out}")
    if args.metrics:                                                   # (both in [-1, 1]: scored as reflectance-like [0, 1])
        from eo_diffusion_amd import metrics
        print(metrics.describe(metrics.quality(scene, truth, affine=(0.5, 0.5), ratio=args.factor), "returned scene against the truth"))


if __name__ == "__main__":
    main()
