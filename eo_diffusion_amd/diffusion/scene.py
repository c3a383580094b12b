"""The argument walk of a scene call, once: what EODiffusion.sampling_scene, DDIMSampler.sample_scene and DPMSolverSampler.sample_scene do
in front of their first step.  A scene is a stack of one: every call runs on a tiling.TileStack and a state [B, C, H, W], B = n_scenes >= 1.

    hs = check(m, what, ...)    the host half: touches no device, launches nothing, and does EVERY refusal.  EODiffusion.check_scene_args
                                is this half alone, which is what lets all ranks of dist.sharded_sampling_scene refuse together.
    sc = setup(m, hs, start)    the device half: the known region, conditioning and x_T on the device, the tiles to evaluate
                                (tiling.tiles_to_evaluate: the call's one host synchronisation), the conditioning cut into them, the
                                observation / threshold bound.  It refuses nothing that the arguments alone could have shown.

What differs between the samplers is passed in: `walk` (a callable -> (visits, jump_after) that fixes the walk and counts the injected
draws), `known` (the sampler's own known region: a pair (check(sized, state) -> bool, on_device(as_scene, state) -> (x0, mask)) for
the state (B, C, H, W); EODiffusion cuts it out of `cond`, the DDIM / DPM-Solver++ samplers take mask / x0), and `start` (the draw
of a state that was not given)."""
from types import SimpleNamespace

import torch

from .. import _lib
from ..tiling import TileStack, gather_padded, tile_slots, tiles_to_evaluate
from . import threshold as thresholding


def check(m, what, scene_size, overlap, device, n_scenes, walk, tile_batch, skip_known, observation, threshold, *, needs, known=None,
          rng="philox", x_T=None, conditioning=None, conditioning_name="conditioning", unconditional_conditioning=None, guidance_scale=1.0,
          y=None):
    """The host half.  `m`: the EODiffusion; `needs`: what this sampler takes a known region from (for skip_known's refusal).  Returns
    the namespace setup() goes on from; nothing in it is on a device."""
    plan, dev = m._scene_args(what, scene_size, overlap, device)
    if rng not in ("philox", "torch"):
        raise _lib.EodError(f"{what}: rng is 'philox' or 'torch', got {rng!r}")
    if skip_known and observation is not None:
        raise _lib.EodError(f"{what}: skip_known=True cannot be combined with `observation`: a skipped tile has no estimate whose "
                            "prediction could be projected")
    thresholding.no_skip(what, skip_known, threshold)
    B = m._scene_count(what, n_scenes)
    state = (B, m.in_channels, plan.H, plan.W)
    visits, jump_after = walk()
    tile_slots(plan, tile_batch)  # (refuses a bad tile_batch)
    thresholding.bind(threshold, observation, what, state, len(visits), None)
    sized = lambda name, z, channels: m._scene_shape(what, name, z, channels, plan, B)
    guided = unconditional_conditioning is not None and guidance_scale != 1.0
    if x_T is not None:
        sized("x_T", x_T, state[1])
    has_known = known is not None and known[0](sized, state)
    if conditioning is not None:
        conditioning = sized(conditioning_name, conditioning, None)
    if unconditional_conditioning is not None:
        sized("unconditional_conditioning", unconditional_conditioning, conditioning.shape[1] if guided and conditioning is not None else None)
    if skip_known and not has_known:
        tiles_to_evaluate(what, plan, None, skip_known, needs)  # (its refusal of skip_known without a mask; nothing else happens)
    if y is not None and torch.as_tensor(y).numel() not in (1, B):
        raise _lib.EodError(f"{what}: a stack of {B} scenes takes one class label, or one per scene; got {torch.as_tensor(y).numel()}")
    if guided and conditioning is None:
        raise _lib.EodError(f"{what}: classifier-free guidance needs `conditioning` next to `unconditional_conditioning`")
    return SimpleNamespace(what=what, plan=plan, device=dev, state=state, visits=visits, jump_after=jump_after, tile_batch=tile_batch,
                           skip_known=skip_known, needs=needs, known=known[1] if has_known else None, observation=observation,
                           threshold=threshold, x_T=x_T, conditioning=conditioning,
                           unconditional_conditioning=unconditional_conditioning if guided else None, y=y)


def setup(m, hs, start):
    """The device half, after check().  start(shape, device) draws the state when x_T was not given.  Returns a namespace: `tiles` (the
    TileStack that goes through the UNet -- with skip_known a listed one), `full` (the stack of every tile; the result goes through
    keep_known iff tiles is not full), x0 / mask [B, ...] or None, c_tiles / uc_tiles / y_slots (conditioning and labels per tile
    slot) or None, img (the start state), obs (the bound observation / threshold or None), as_scene(name, z) for the injected draws.
    `known` is not None when no tile is active: the call returns it and the UNet is never called."""
    what, plan, dev, (B, C, _, _) = hs.what, hs.plan, hs.device, hs.state
    m._tables_on(dev)
    as_scene = lambda name, z, channels=C, expand=True: m._scene_tensor(what, name, z, channels, plan, dev, B, expand)
    sc = SimpleNamespace(full=TileStack(plan, B), B=B, device=dev, tile_batch=hs.tile_batch, visits=hs.visits, jump_after=hs.jump_after,
                         as_scene=as_scene, known=None)
    # (a known region with leading dimension 1 stands for every scene: it is classified once, then expanded)
    x0, mask = hs.known(as_scene, hs.state) if hs.known is not None else (None, None)
    sc.tiles = tiles = tiles_to_evaluate(what, sc.full, mask, hs.skip_known, hs.needs)
    if mask is not None:
        x0, mask = (z.expand(B, *z.shape[1:]).contiguous() for z in (x0, mask))
    sc.x0, sc.mask = x0, mask
    if tiles is None:
        sc.known = x0.clone()
        return sc
    sc.chunk, slots = tile_slots(tiles, hs.tile_batch)
    cut = lambda name, z: None if z is None else gather_padded(as_scene(name, z, None), tiles, hs.tile_batch)
    sc.c_tiles, sc.uc_tiles = cut("conditioning", hs.conditioning), cut("unconditional_conditioning", hs.unconditional_conditioning)
    sc.y_slots = None
    if hs.y is not None:  # the label of the scene each tile slot belongs to (padding slots repeat the last listed tile, and its label)
        scene_of = torch.from_numpy(tiles.index // plan.n_tiles).to(torch.int64)
        scene_of = torch.cat([scene_of, scene_of[-1:].expand(slots - tiles.n_tiles)])
        sc.y_slots = torch.as_tensor(hs.y).reshape(-1).to(torch.int64).expand(B).to(dev)[scene_of.to(dev)].contiguous()
    sc.img = as_scene("x_T", hs.x_T) if hs.x_T is not None else start(hs.state, dev)
    sc.obs = thresholding.bind(hs.threshold, hs.observation, what, hs.state, len(hs.visits), dev, getattr(m, "parameterization", "eps"))
    return sc
