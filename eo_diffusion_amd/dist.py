"""Batch-sharded sampling across the GPUs of one node.

The reference has no distributed code at all (single hard-coded device, train.py:46, inference.py:55).
Each sample's reverse chain is independent (GroupNorm is per-sample, no BatchNorm on the path), so the
path shards by samples with NO per-step communication: rank r of W runs samples [r*B/W, (r+1)*B/W),
draws its noise from the counter-based Philox generator keyed by the GLOBAL sample index (results are
therefore identical for every W, including W = 1), and the final images are concatenated with ONE
all-gather (RCCL over xGMI with backend "nccl"; gloo on CPU tensors in the tests).
"""
import torch
import torch.distributed as dist


def shard_bounds(n_total, world, rank):
    """[lo, hi) of rank's samples; the first n_total % world ranks take one extra sample."""
    if not (0 <= rank < world):
        raise ValueError(f"rank {rank} outside world {world}")
    base, rem = divmod(n_total, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def gather_samples(local, n_total, group=None, force_gather=False):
    """All-gather ragged per-rank shards [n_r, ...] into [n_total, ...] on every rank (one collective).  A single rank returns its
    shard as it is -- unless force_gather: then the collective runs even in a one-rank group (the RCCL all_gather_into_tensor on
    device memory, executed for real on a one-GPU box; tests/test_gpu_dist.py)."""
    initialised = dist.is_available() and dist.is_initialized()
    if force_gather and not initialised:
        raise RuntimeError("gather_samples(force_gather=True) needs an initialised process group")
    if not initialised or (dist.get_world_size(group) == 1 and not force_gather):
        assert local.shape[0] == n_total
        return local
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    sizes = [shard_bounds(n_total, world, r)[1] - shard_bounds(n_total, world, r)[0] for r in range(world)]
    assert local.shape[0] == sizes[rank], (local.shape, sizes, rank)
    nmax = max(sizes)
    tail = local.shape[1:]
    if all(s == nmax for s in sizes):
        out = torch.empty((n_total,) + tuple(tail), dtype=local.dtype, device=local.device)
        dist.all_gather_into_tensor(out, local.contiguous(), group=group)
        return out
    # ragged: pad to the largest shard, gather, strip
    pad = torch.zeros((nmax,) + tuple(tail), dtype=local.dtype, device=local.device)
    pad[: local.shape[0]] = local
    buf = torch.empty((world * nmax,) + tuple(tail), dtype=local.dtype, device=local.device)
    dist.all_gather_into_tensor(buf, pad, group=group)
    return torch.cat([buf[r * nmax: r * nmax + sizes[r]] for r in range(world)], 0)


@torch.no_grad()
def sharded_sampling(model, n_samples, *, seed=0, clipped_reverse_diffusion=True, cond=None, y=None, device=None,
                     group=None, progress=False, force_gather=False, observation=None, threshold=None):
    """EODiffusion.sampling over all ranks of `group`: every rank returns the full [n_samples, C, H, W] tensor.
    cond / y are the GLOBAL tensors (each rank slices its own rows), and so is `observation` (an observation of diffusion/consistency.py
    or a list of them: each rank takes its shard(n_samples, lo, hi), tensors with leading dimension 1 stay).  threshold (a
    diffusion/threshold.py DynamicThreshold) is passed on unchanged: it is per sample, so nothing needs sharding.  force_gather: see
    gather_samples."""
    from .diffusion import consistency
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    lo, hi = shard_bounds(n_samples, world, rank)
    dev = device or f"cuda:{torch.cuda.current_device()}"
    c = cond[lo:hi] if cond is not None else None
    yy = y[lo:hi] if y is not None else None
    obs = {} if observation is None else dict(observation=consistency.shard(observation, n_samples, lo, hi))   # (None: the call of before)
    if threshold is not None:
        obs["threshold"] = threshold
    local = model.sampling(hi - lo, clipped_reverse_diffusion=clipped_reverse_diffusion, device=dev, cond=c, y=yy,
                           rng="philox", seed=seed, sample_offset=lo, progress=progress, **obs)
    return gather_samples(local, n_samples, group=group, force_gather=force_gather)


def _shard_of(z, n_total, lo, hi):
    """rows [lo, hi) of a GLOBAL per-scene argument; one with leading dimension 1 (the same for every scene) is passed on as it is"""
    if z is None:
        return None
    z = torch.as_tensor(z)
    return z if z.shape[0] == 1 and n_total != 1 else z[lo:hi]


@torch.no_grad()
def sharded_sampling_scene(model, scene_size, n_scenes, *, seed=0, clipped_reverse_diffusion=True, cond=None, y=None, overlap=0,
                           tile_batch=16, resample=None, skip_known=False, device=None, group=None, progress=False, force_gather=False,
                           observation=None, threshold=None):
    """EODiffusion.sampling_scene(n_scenes=...) over all ranks of `group`: scenes shard like samples do.  Rank r runs the scenes
    shard_bounds(n_scenes, world, r) as one stacked call with rng="philox" and sample_offset = lo -- scene b is sample b of `seed` on
    every rank, so the result does not depend on the world size -- and the scenes are concatenated with ONE all-gather: every rank
    returns [n_scenes, C, H, W].  cond / y are the GLOBAL tensors (leading dimension n_scenes, or 1 for one known scene / label shared
    by all); `observation` is the GLOBAL observation (or list of them), each rank takes its shard(n_scenes, lo, hi); `threshold` is passed on unchanged (it is per scene).  A rank whose shard is empty launches nothing and still takes part in the collective.  Every rank first checks the
    GLOBAL arguments (EODiffusion.check_scene_args), so a bad argument is refused on all ranks alike, before any of them launches or
    enters the collective -- a rank with an empty shard included."""
    from .diffusion import consistency
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    dev = device or f"cuda:{torch.cuda.current_device()}"
    obs = {} if observation is None else dict(observation=observation)                                         # (None: the calls of before)
    thr = {} if threshold is None else dict(threshold=threshold)
    model.check_scene_args(scene_size, dev, n_scenes=n_scenes, cond=cond, y=y, overlap=overlap, tile_batch=tile_batch, resample=resample,
                           skip_known=skip_known, **obs, **thr)
    lo, hi = shard_bounds(n_scenes, world, rank)
    h, w = (int(v) for v in scene_size)
    if hi > lo:
        yy = None if y is None else torch.as_tensor(y).reshape(-1)
        local = model.sampling_scene((h, w), clipped_reverse_diffusion, dev, cond=_shard_of(cond, n_scenes, lo, hi),
                                     y=None if yy is None else _shard_of(yy, n_scenes, lo, hi), overlap=overlap, tile_batch=tile_batch,
                                     rng="philox", seed=seed, progress=progress, resample=resample, skip_known=skip_known,
                                     n_scenes=hi - lo, sample_offset=lo, **thr,
                                     **({} if observation is None else dict(observation=consistency.shard(observation, n_scenes, lo, hi))))
    else:
        local = torch.empty((0, model.in_channels, h, w), dtype=torch.float32, device=dev)
    return gather_samples(local, n_scenes, group=group, force_gather=force_gather)
