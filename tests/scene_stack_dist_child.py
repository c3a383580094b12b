"""Child process of tests/test_gpu_scene_stack.py: a ONE-rank RCCL ("nccl") process group on the GPU, in a process that has not touched
the GPU before.  Runs dist.sharded_sampling_scene with the all-gather forced (all_gather_into_tensor on HBM tensors), compares it bit
for bit with the plain stacked EODiffusion.sampling_scene of the same seed, and prints one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import torch.distributed as dist
    from eo_diffusion_amd.backbones.unet_openai import UNetModel, unet_param_shapes
    from eo_diffusion_amd.diffusion.model import EODiffusion
    from eo_diffusion_amd.dist import sharded_sampling_scene
    from tests.synth import synth_input, synth_state_dict

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1)
    res = {"backend": dist.get_backend(), "world": dist.get_world_size()}
    try:
        cfg = dict(image_size=16, in_channels=3, model_channels=32, out_channels=3, num_res_blocks=1, attention_resolutions=[2],
                   channel_mult=[1, 2], num_heads=4)
        u = UNetModel(**cfg).set_precision(os.environ.get("EOD_PRECISION", "fp32x3"))
        u.load_state_dict(synth_state_dict(unet_param_shapes(**cfg), 7))
        m = EODiffusion(u, timesteps=6, image_size=16, in_channels=3, cond_type="sum", device=str(dev)).to(dev).eval()
        B, H, W = 3, 40, 57
        gt = synth_input("dgt", (B, 3, H, W), 3, uniform=True) * 2 - 1
        mask = torch.ones(B, 1, H, W)
        mask[0, 0, 14:20, 10:30] = 0.0
        mask[2, 0, 26:32, 40:50] = 0.0                               # (scene 1 has nothing to do)
        cond = torch.cat([gt, mask], 1)
        ok = {}
        for name, sk in (("sharded_equals_stacked_bits", False), ("skip_known_equals_stacked_bits", True)):
            full = sharded_sampling_scene(m, (H, W), B, seed=7, cond=cond, overlap=4, tile_batch=16, resample=(2, 2), skip_known=sk,
                                          device=str(dev), force_gather=True)
            ref = m.sampling_scene((H, W), True, str(dev), cond=cond, overlap=4, tile_batch=16, seed=7, resample=(2, 2), skip_known=sk,
                                   n_scenes=B, progress=False)
            torch.cuda.synchronize()
            res[name] = bool(torch.equal(full, ref)) and full.data_ptr() != ref.data_ptr()
        res["members_differ"] = not bool(torch.equal(full[0], full[2]))
        res["finite"] = bool(torch.isfinite(full).all())
        res["on_gpu"] = full.is_cuda
        res["shape"] = list(full.shape)
    finally:
        dist.destroy_process_group()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
