#!/usr/bin/env python3
"""Sample a scene whose bands are known at different grids: observation-consistent DPM-Solver++ over a tiled scene.

    python examples/sharpen_bands.py                                   # 384 x 576, bands observed at 1x, 2x and 4x coarser grids
    python examples/sharpen_bands.py --factors 1 2 6 --height 384 --width 576 --steps 25
    python examples/sharpen_bands.py --ancestral --timesteps 250       # the reference's own sampler: model.sampling_scene(..., observation=...)

Channel c of a synthetic scene is "observed" as its mean over every f_c x f_c block (f_c = 1: the band itself, at full resolution) --
what a 20 m or 60 m Sentinel-2 band is next to a 10 m one.  `DPMSolverSampler.sample_scene(..., observation=Observation(values,
factors))` makes the data prediction of every evaluation consistent with that observation; the script prints
how far the block means of the result are from the observation.  With --ancestral the call is the ancestral chain over all `--timesteps`
levels, `EODiffusion.sampling_scene(..., observation=...)`: there the RETURNED scene itself, not only the last
prediction, has the observation's block means for weight 1.  The network is untrained unless --ckpt is given: the script shows the
mechanics and the constraint, not image quality.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eo_diffusion_amd.backbones.unet_openai import UNetModel  # noqa: E402
from eo_diffusion_amd.diffusion.consistency import Observation, block_mean  # noqa: E402
from eo_diffusion_amd.diffusion.dpm_solver import DPMSolverSampler  # noqa: E402
from eo_diffusion_amd.diffusion.model import EODiffusion  # noqa: E402


def synthetic_scene(h, w, seed):
    """[1, 3, h, w] in [0, 1]: a few smooth fields (low-frequency sinusoids) -- stands in for a Sentinel-2 tile"""
    r = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.zeros((3, h, w), np.float32)
    for c in range(3):
        for _ in range(4):
            fy, fx, ph = r.uniform(0.002, 0.02), r.uniform(0.002, 0.02), r.uniform(0, 6.28)
            img[c] += np.sin(fy * yy + fx * xx + ph)
    img = (img - img.min()) / (img.max() - img.min())
    return torch.from_numpy(img)[None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=576)
    ap.add_argument("--factors", type=int, nargs=3, default=[1, 2, 4], help="the block edge per band (1 .. 8); each divides height and width")
    ap.add_argument("--image-size", type=int, default=64, help="the UNet's tile size")
    ap.add_argument("--overlap", type=int, default=16)
    ap.add_argument("--timesteps", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--ancestral", action="store_true", help="the ancestral sampler over all --timesteps levels instead of DPM-Solver++ over --steps")
    ap.add_argument("--weight", type=float, default=1.0, help="1: the block means are imposed; below 1: pulled towards (a noisy observation)")
    ap.add_argument("--precision", default="fp32x3", choices=["fp32", "fp32x3", "fp16"])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--out", default="sharpened_scene.npy")
    ap.add_argument("--metrics", action="store_true", help="score the returned scene against the synthetic truth (eo_diffusion_amd.metrics.quality)")
    args = ap.parse_args()
    device = "cuda:0"
    torch.manual_seed(args.seed)
    unet = UNetModel(args.image_size, in_channels=3, model_channels=64, out_channels=3, channel_mult=[1, 2, 3], attention_resolutions=[],
                     num_res_blocks=1, num_heads=1).set_precision(args.precision)
    model = EODiffusion(unet, timesteps=args.timesteps, image_size=args.image_size, in_channels=3, device=device)
    if args.ckpt:
        model.load_state_dict(torch.load(args.ckpt, map_location="cpu")["model"])
    else:
        with torch.no_grad():  # the reference zero-initialises the output convs: give the untrained network something to say
            for p in unet.parameters():
                if p.dim() > 1 and float(p.abs().max()) == 0.0:
                    p.normal_(0.0, 0.02)
    model = model.to(device).eval()
    truth = synthetic_scene(args.height, args.width, args.seed).to(device) * 2.0 - 1.0
    values = block_mean(truth, args.factors)                         # A+ A x: what the coarse bands show, on the full-resolution grid
    observation = Observation(values, args.factors, weight=args.weight)
    sampler = DPMSolverSampler(model)
    t0 = time.perf_counter()
    if args.ancestral:
        scene = model.sampling_scene((args.height, args.width), True, device, overlap=args.overlap, seed=args.seed, progress=False,
                                     observation=observation)
    else:
        scene, _ = sampler.sample_scene(args.steps, (args.height, args.width), overlap=args.overlap, clip_denoised=True, progress=False,
                                        observation=observation)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    evaluations = args.timesteps if args.ancestral else sampler.num_evaluations
    np.save(args.out, ((scene + 1.0) / 2.0)[0].cpu().numpy())
    res = (block_mean(scene, args.factors) - values).abs().amax(dim=(0, 2, 3)).tolist()
    print(f"{args.height} x {args.width}, factors {tuple(args.factors)}, weight {args.weight}: {evaluations} evaluations in {dt:.2f} s; "
          f"max |block mean of the result - observation| per band: " + ", ".join(f"{r:.2e}" for r in res) + f"; wrote {args.out}")
    if args.metrics:                                                   # (both in [-1, 1]: scored as reflectance-like [0, 1])
        from eo_diffusion_amd import metrics
        ratio = max(args.factors) if max(args.factors) > 1 else None
        print(metrics.describe(metrics.quality(scene, truth, affine=(0.5, 0.5), ratio=ratio), "returned scene against the truth"))


if __name__ == "__main__":
    main()
