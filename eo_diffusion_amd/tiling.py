"""Whole-scene sampling: the tile plan and the two kernels between a scene-sized tensor and UNet-sized tiles.

    plan  = TilePlan(H, W, tile, overlap)        host-side (numpy), importable without a GPU
    tiles = gather_tiles(scene, plan)            [1,C,H,W] (or [C,H,W]) -> [n_tiles, C, tile, tile]    eod_scene_stack_gather
    scene = blend_tiles(tiles, plan)             [n_tiles, C, tile, tile] -> [1, C, H, W]              eod_scene_stack_blend
    e     = tiled_estimate(scene, plan, tile_batch, fn)   gather -> fn on chunks of tile_batch tiles -> blend
    idx   = active_tiles(mask, plan)             the tiles whose window holds a hole pixel of a RePaint mask      eod_scene_stack_tile_active
    sub   = plan.subset(idx)                     a TileSubset: goes wherever a plan goes above, on the listed tiles only
    out   = keep_known(x, known, sub)            x at estimated pixels, known elsewhere                           eod_scene_stack_keep_known
    tiles = tiles_to_evaluate(what, plan, mask, skip_known, needs)   what a scene sampler evaluates: plan | sub | None (nothing active)
    stack = TileStack(plan, B)                   B scenes of one plan ([B, C, H, W]): goes wherever a plan goes above; tiles of every scene
    part  = TileStack(plan, B, indices)          ... or the listed tiles only (global numbers b * n_tiles + i), like a TileSubset
    mean, std = scene_stats(scenes)              [B, C, H, W] -> per-pixel mean and sample standard deviation, each [1, C, H, W]   eod_scene_stats
    qs = scene_quantiles(scenes, (0.05, 0.5, 0.95))   [B, C, H, W] -> per-pixel quantiles over the B members, [Q, C, H, W]        eod_scene_quantiles

One path: a scene is a stack of one.  Whatever kind of plan an operation is given, it makes ONE library call, the eod_scene_stack_* entry
point, with B = 1 for a TilePlan / TileSubset and a null index / slot_of for the full form (_launch_form).  The library's single-scene
entry points (eod_scene_gather ...) are the same launches with B = 1 and remain for C callers; nothing here calls them.

Plan, per axis of length L: origins min(i * (tile - overlap), L - tile) until the axis is covered -- the last tile is shifted
inwards, never padded.  Weights, per axis, [n][tile]: 1 in a tile's interior, a linear ramp (k + 1) / (o + 1) across the o pixels
a tile shares with its neighbour (rising on the left side, falling on the right; o is the ACTUAL shared width, which is larger than
`overlap` next to a shifted last tile; where both ramps of a tile meet they are multiplied), then normalised in float64 so that the
weights of the tiles covering a coordinate sum to one, then rounded to fp32.  A coordinate covered by ONE tile gets exactly 1.0f,
which is what makes overlap = 0 (and every tile interior) pass the UNet's estimate through bit for bit.  The 2-D weight of tile
(iy, ix) at its local (ly, lx) is the fp32 product wy[iy][ly] * wx[ix][lx]; tiles are numbered row-major, i = iy * ntx + ix.

The blend is  e[c, y, x] = sum over the tiles covering (y, x), in ascending i, of w_i * e_i : products rounded once, added left to
right, no atomics -- a pure function of its inputs (csrc/scene.hip).  This maps to the reference's patch cutting in its data
loaders (data_utils' patch_overlap), not to a line of its samplers: the reference never puts the patches back together.

Tile subsets (skip_known of the scene samplers).  Known: mask == 1.  A HOLE pixel has a mask value other than exactly 1.0f in some mask
channel (soft values and NaN included).  A tile is ACTIVE iff its window holds a hole pixel; a pixel is ESTIMATED iff every tile that
covers it is active (every hole pixel is; a pixel that is not estimated is known).  With only the active tiles evaluated the blend has
the unchanged weights, order and roundings at every estimated pixel and is 0.0f elsewhere -- where the RePaint mix replaces the state
by q_sample(gt) before every network evaluation anyway, so the active tiles see the inputs of the full call.

Stacks (n_scenes of the scene samplers).  B scenes of ONE plan are tiled together: tile i of scene b has the global number
g = b * n_tiles + i, the tiles of the whole stack go through the network in one sequence of chunks (a chunk may hold tiles of several
scenes), and every rule above holds per scene: scene b is blended from its own tiles with the single scene's arithmetic, and a pixel
of scene b is estimated iff every tile of scene b covering it is listed."""
import numpy as np

from . import _lib


def axis_plan(L, tile, overlap):
    """origins (int32 [n]) and weights (float32 [n][tile]) of one axis; see the module docstring."""
    L, tile, overlap = int(L), int(tile), int(overlap)
    if tile < 1:
        raise _lib.EodError(f"tile size must be positive, got {tile}")
    if L < tile:
        raise _lib.EodError(f"scene axis of {L} pixels is smaller than the {tile}-pixel tile (tiles are never padded)")
    if not 0 <= overlap <= tile // 2:
        raise _lib.EodError(f"overlap must be in [0, tile // 2] = [0, {tile // 2}], got {overlap}")
    stride = tile - overlap
    origins = []
    while True:
        o = min(len(origins) * stride, L - tile)
        origins.append(o)
        if o + tile >= L:
            break
    n = len(origins)
    raw = np.ones((n, tile), dtype=np.float64)
    for i in range(n - 1):
        o = origins[i] + tile - origins[i + 1]  # pixels tile i shares with tile i + 1 (>= overlap; 0: they only touch)
        if o > 0:
            ramp = (np.arange(o, dtype=np.float64) + 1.0) / (o + 1.0)
            raw[i + 1, :o] *= ramp
            raw[i, tile - o:] *= ramp[::-1]
    total = np.zeros(L, dtype=np.float64)
    for i, o in enumerate(origins):
        total[o:o + tile] += raw[i]
    w = np.empty((n, tile), dtype=np.float32)
    for i, o in enumerate(origins):
        w[i] = (raw[i] / total[o:o + tile]).astype(np.float32)
    return np.asarray(origins, dtype=np.int32), w


class TilePlan:
    """Tiling of an H x W scene into tile x tile windows that overlap by at least `overlap` pixels.

    origins_y / origins_x: int32 [nty] / [ntx];  wy / wx: float32 [nty][tile] / [ntx][tile];  n_tiles = nty * ntx, row-major.
    Raises EodError when the scene is smaller than a tile or overlap is outside [0, tile // 2]."""

    def __init__(self, H, W, tile, overlap=0):
        self.H, self.W, self.tile, self.overlap = int(H), int(W), int(tile), int(overlap)
        self.origins_y, self.wy = axis_plan(H, tile, overlap)
        self.origins_x, self.wx = axis_plan(W, tile, overlap)
        self.nty, self.ntx = len(self.origins_y), len(self.origins_x)
        self.n_tiles = self.nty * self.ntx
        self._dev = {}

    def __repr__(self):
        return f"TilePlan(H={self.H}, W={self.W}, tile={self.tile}, overlap={self.overlap}: {self.nty} x {self.ntx} tiles)"

    def origin(self, i):
        """(y0, x0) of tile i"""
        iy, ix = divmod(int(i), self.ntx)
        return int(self.origins_y[iy]), int(self.origins_x[ix])

    def origins(self):
        return [self.origin(i) for i in range(self.n_tiles)]

    def weight(self, i):
        """the fp32 2-D weight [tile][tile] of tile i (host copy; the kernel forms the same product per element)"""
        iy, ix = divmod(int(i), self.ntx)
        return self.wy[iy][:, None] * self.wx[ix][None, :]

    def cover_count(self):
        """int [H][W]: how many tiles cover each pixel"""
        cy = np.zeros(self.H, dtype=np.int64)
        cx = np.zeros(self.W, dtype=np.int64)
        for o in self.origins_y:
            cy[o:o + self.tile] += 1
        for o in self.origins_x:
            cx[o:o + self.tile] += 1
        return cy[:, None] * cx[None, :]

    def active_tiles(self, mask):
        """ascending int32 indices of the tiles whose window holds a hole pixel of the host array `mask` ([H, W] or [..., H, W]: a
        value != 1 in any leading index makes the pixel a hole, NaN included)"""
        m = np.asarray(mask)
        if m.ndim < 2 or tuple(m.shape[-2:]) != (self.H, self.W):
            raise _lib.EodError(f"active_tiles: the mask must be [..., {self.H}, {self.W}], got {tuple(m.shape)}")
        hole = (m != 1).reshape(-1, self.H, self.W).any(axis=0)
        # an integral image answers every window in one pass
        ii = np.zeros((self.H + 1, self.W + 1), dtype=np.int64)
        ii[1:, 1:] = hole.cumsum(axis=0).cumsum(axis=1)
        y0, x0 = self.origins_y.astype(np.int64)[:, None], self.origins_x.astype(np.int64)[None, :]
        s = self.tile
        count = ii[y0 + s, x0 + s] - ii[y0, x0 + s] - ii[y0 + s, x0] + ii[y0, x0]
        return np.flatnonzero(count.reshape(-1) > 0).astype(np.int32)

    def subset(self, indices):
        """the TileSubset of the listed tiles (ascending, unique, in range -- refused otherwise)"""
        return TileSubset(self, indices)

    def device_tables(self, device):
        """(origins_y, origins_x, wy, wx) as device tensors, uploaded once per device"""
        import torch
        dev = torch.device(device)
        hit = self._dev.get(dev)
        if hit is None:
            hit = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (self.origins_y, self.origins_x, self.wy, self.wx))
            self._dev[dev] = hit
        return hit


def _tile_list(who, noun, indices, total):
    """(index int32 [n], slot_of int32 [total]) of a tile list that is 1-D, non-empty, integer, in [0, total), ascending and unique;
    refused otherwise, in the name of the class `who` that is being made"""
    raw = np.asarray(list(indices) if not isinstance(indices, np.ndarray) else indices)
    if raw.ndim != 1 or raw.size < 1:
        raise _lib.EodError(f"{who}: the tile list must be a non-empty 1-D sequence of {noun}, got shape {tuple(raw.shape)}")
    if not np.issubdtype(raw.dtype, np.integer):
        raise _lib.EodError(f"{who}: {noun} are integers, got {raw.dtype}")
    idx = raw.astype(np.int64)
    if idx.min() < 0 or idx.max() >= total:
        raise _lib.EodError(f"{who}: {noun} must be in [0, {total}), got {int(idx.min())} .. {int(idx.max())}")
    if np.any(np.diff(idx) <= 0):
        raise _lib.EodError(f"{who}: {noun} must be ascending and unique")
    slot_of = np.full(total, -1, dtype=np.int32)
    slot_of[idx] = np.arange(idx.size, dtype=np.int32)
    return idx.astype(np.int32), slot_of


class _TileList:
    """what a TileSubset and a TileStack are made of: a plan and the list (index, slot_of) of the tiles that go through the network"""

    def _set(self, plan, index, slot_of):
        self.plan, self.index, self.slot_of = plan, index, slot_of
        self.n_tiles = int(index.size)
        self.H, self.W, self.tile, self.overlap = plan.H, plan.W, plan.tile, plan.overlap
        self._dev = {}

    def device_tables(self, device):
        """(index, slot_of) as device int32 tensors, uploaded once per device"""
        import torch
        dev = torch.device(device)
        hit = self._dev.get(dev)
        if hit is None:
            hit = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (self.index, self.slot_of))
            self._dev[dev] = hit
        return hit


class TileSubset(_TileList):
    """Some tiles of a TilePlan, in ascending order: what gather_tiles / blend_tiles / tile_slots / gather_padded / tiled_estimate
    work on when only these tiles go through the network.

    plan; index int32 [n_tiles] (the listed tiles; n_tiles = how many are LISTED); slot_of int32 [plan.n_tiles] (position of a tile in
    the list, -1 = absent); H, W, tile, overlap as the plan's.  Raises EodError for an empty, unsorted, repeated or out-of-range list."""

    def __init__(self, plan, indices):
        if not isinstance(plan, TilePlan):
            raise _lib.EodError(f"TileSubset: a subset is taken of a TilePlan, got {type(plan).__name__}")
        self._set(plan, *_tile_list("TileSubset", "tile indices", indices, plan.n_tiles))

    def __repr__(self):
        return f"TileSubset({self.n_tiles} of {self.plan.n_tiles} tiles of {self.plan!r})"

    def origin(self, k):
        """(y0, x0) of the tile in slot k"""
        return self.plan.origin(self.index[int(k)])

    def estimated(self):
        """bool [H][W]: the pixels whose covering tiles are all listed"""
        p = self.plan
        est = np.ones((p.H, p.W), dtype=bool)
        for i in np.flatnonzero(self.slot_of < 0):
            y0, x0 = p.origin(i)
            est[y0:y0 + p.tile, x0:x0 + p.tile] = False
        return est


class TileStack(_TileList):
    """n_scenes copies of one TilePlan, tiled together; with `indices` only the listed global tiles g = b * plan.n_tiles + i (ascending,
    unique, in range -- refused otherwise, like a TileSubset).  Goes wherever a plan or a subset goes; scenes are then [B, C, H, W].

    plan; n_scenes; listed (were indices given); index int32 [n_tiles] (the global numbers; n_tiles = how many tiles go through the
    network); slot_of int32 [n_scenes * plan.n_tiles] (position in the list, -1 = absent; the identity without indices); H, W, tile,
    overlap as the plan's."""

    def __init__(self, plan, n_scenes, indices=None):
        if not isinstance(plan, TilePlan):
            raise _lib.EodError(f"TileStack: a stack is made of a TilePlan, got {type(plan).__name__}")
        if isinstance(n_scenes, bool) or not isinstance(n_scenes, (int, np.integer)) or n_scenes < 1:
            raise _lib.EodError(f"TileStack: n_scenes must be an integer >= 1, got {n_scenes!r}")
        total = int(n_scenes) * plan.n_tiles
        if total > 0x7fffffff:
            raise _lib.EodError(f"TileStack: {n_scenes} scenes of {plan.n_tiles} tiles cannot be numbered in an int32")
        self.n_scenes, self.listed = int(n_scenes), indices is not None
        if indices is None:
            index = np.arange(total, dtype=np.int32)
            self._set(plan, index, index)
        else:
            self._set(plan, *_tile_list("TileStack", "global tile numbers", indices, total))

    def __repr__(self):
        return f"TileStack({self.n_tiles} of {self.n_scenes} x {self.plan.n_tiles} tiles of {self.plan!r})"

    def scene_of(self, k):
        """(b, i): the scene and the tile of that scene's plan in slot k"""
        return divmod(int(self.index[int(k)]), self.plan.n_tiles)

    def origin(self, k):
        """(y0, x0) of the tile in slot k"""
        return self.plan.origin(self.scene_of(k)[1])

    def per_scene(self):
        """per scene, the ascending int32 tile numbers of its plan that are listed"""
        nt = self.plan.n_tiles
        return [(self.index[(self.index >= b * nt) & (self.index < (b + 1) * nt)] - b * nt).astype(np.int32) for b in range(self.n_scenes)]

    def estimated(self):
        """bool [n_scenes][H][W]: the pixels of each scene whose covering tiles (of that scene) are all listed"""
        p = self.plan
        est = np.ones((self.n_scenes, p.H, p.W), dtype=bool)
        for g in np.flatnonzero(self.slot_of < 0):
            b, i = divmod(int(g), p.n_tiles)
            y0, x0 = p.origin(i)
            est[b, y0:y0 + p.tile, x0:x0 + p.tile] = False
        return est

    def active_tiles(self, mask):
        """ascending int32 GLOBAL numbers of the tiles whose window holds a hole pixel of the host array `mask` [n_scenes, ..., H, W]
        (TilePlan.active_tiles, scene by scene)"""
        m = np.asarray(mask)
        if m.ndim < 3 or m.shape[0] != self.n_scenes or tuple(m.shape[-2:]) != (self.H, self.W):
            raise _lib.EodError(f"active_tiles: the mask of a stack must be [{self.n_scenes}, ..., {self.H}, {self.W}], got {tuple(m.shape)}")
        nt = self.plan.n_tiles
        return np.concatenate([self.plan.active_tiles(m[b]).astype(np.int64) + b * nt for b in range(self.n_scenes)]).astype(np.int32)


def _launch_form(plan):
    """(base, B, tile list, single) of any of the three plan kinds, as a launch needs it: the TilePlan, the number of scenes, the object
    whose device_tables() hold (index, slot_of) or None for the full form, and whether the argument was a single-scene kind (a TilePlan
    or a TileSubset: B = 1, and a scene may come without its leading dimension)"""
    if isinstance(plan, TilePlan):
        return plan, 1, None, True
    if isinstance(plan, TileSubset):
        return plan.plan, 1, plan, True
    if isinstance(plan, TileStack):
        return plan.plan, plan.n_scenes, (plan if plan.listed else None), False
    raise _lib.EodError(f"a TilePlan, a TileSubset or a TileStack is needed, got {type(plan).__name__}")


def active_tiles(mask, plan):
    """TilePlan.active_tiles for a mask on the GPU ([H, W] or [..., H, W]): eod_scene_stack_tile_active, then ONE device-to-host copy of
    plan.n_tiles ints (the only synchronisation).  Ascending int32 tile indices (numpy).  With a TileStack: a stacked mask
    [B, ..., H, W] and the global numbers, still one launch and one copy."""
    import torch
    from .engine import current_stream_ptr, f32c, require_gpu
    require_gpu(mask, "active_tiles")
    plan, B, lst, single = _launch_form(plan)
    if single and lst is not None:
        raise _lib.EodError(f"active_tiles: `plan` is a TilePlan, got {type(lst).__name__}")
    if tuple(mask.shape[-2:]) != (plan.H, plan.W) or (mask.dim() < 2 if single else mask.dim() < 3 or mask.shape[0] != B):
        want = "the mask must be [" if single else f"the mask of a stack must be [{B}, "
        raise _lib.EodError(f"active_tiles: {want}..., {plan.H}, {plan.W}], got {tuple(mask.shape)}")
    m = f32c(mask.reshape(B, -1, plan.H, plan.W))
    active = torch.empty(B * plan.n_tiles, dtype=torch.int32, device=m.device)
    oy, ox, _, _ = plan.device_tables(m.device)
    _lib.check(_lib.lib().eod_scene_stack_tile_active(m.data_ptr(), active.data_ptr(), B, m.shape[1], plan.H, plan.W, plan.tile, oy.data_ptr(),
                                                      ox.data_ptr(), plan.nty, plan.ntx, current_stream_ptr(m.device)), "eod_scene_stack_tile_active")
    return np.flatnonzero(active.cpu().numpy()).astype(np.int32)


def tiles_to_evaluate(what, plan, mask, skip_known, needs):
    """The tiles a scene sampler `what` sends through the UNet: the plan itself, with skip_known the TileSubset of the active tiles
    of the known region's `mask` (the plan when every tile is active; active_tiles: the call's one host synchronisation), or None
    when no tile is active.  skip_known without a mask is refused; `needs` says what the sampler takes a known region from.
    For a TileStack: the stack, a listed stack of the active (b, i) in ascending global order, or None; a mask with leading dimension
    1 stands for every scene and is classified once."""
    if not skip_known:
        return plan
    if mask is None:
        raise _lib.EodError(f"{what}: skip_known=True needs a known region ({needs}); there is nothing to skip without one")
    base, B, lst, single = _launch_form(plan)
    if B > 1 and mask.shape[0] == 1:
        one = active_tiles(mask, base).astype(np.int64)
        active = (np.arange(B, dtype=np.int64)[:, None] * base.n_tiles + one[None, :]).reshape(-1).astype(np.int32)
    else:
        active = active_tiles(mask, plan)
    if active.size == 0:
        return None
    if lst is None and active.size == plan.n_tiles:
        return plan
    return base.subset(active) if single else TileStack(base, B, active)


def _scene4(scene, what, B, single):
    from .engine import f32c, require_gpu
    require_gpu(scene, what)
    if not single:
        if scene.dim() != 4 or scene.shape[0] != B:
            raise _lib.EodError(f"{what}: a stack of {B} scene(s) is [{B}, C, H, W], got {tuple(scene.shape)}")
        return f32c(scene)
    x = scene if scene.dim() == 4 else scene[None]
    if x.dim() != 4 or x.shape[0] != 1:
        raise _lib.EodError(f"{what}: a scene is [1, C, H, W] or [C, H, W], got {tuple(scene.shape)}")
    return f32c(x)


def gather_tiles(scene, plan, out=None):
    """scene [1, C, H, W] (or [C, H, W]) fp32 on the GPU -> tiles [n_tiles, C, tile, tile], tile i = the window at plan.origin(i).
    `out`: a contiguous fp32 buffer of at least n_tiles tiles (its first n_tiles are written, and returned).
    `plan` may be a TileSubset: its n_tiles listed tiles, in the list's order; or a TileStack: scene [B, C, H, W], the tiles of every
    scene or the listed ones.  One call for all of them: eod_scene_stack_gather, B = 1 for a single scene, a null index for the full form."""
    import torch
    from .engine import current_stream_ptr
    plan, B, lst, single = _launch_form(plan)
    n = B * plan.n_tiles if lst is None else lst.n_tiles
    x = _scene4(scene, "gather_tiles", B, single)
    _, c, h, w = x.shape
    if (h, w) != (plan.H, plan.W):
        raise _lib.EodError(f"gather_tiles: scene is {h} x {w}, the plan is for {plan.H} x {plan.W}")
    s = plan.tile
    if out is None:
        out = torch.empty((n, c, s, s), dtype=torch.float32, device=x.device)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.dim() == 4 and out.shape[0] >= n
              and tuple(out.shape[1:]) == (c, s, s)):
        raise _lib.EodError(f"gather_tiles: `out` must be a contiguous fp32 GPU tensor [>= {n}, {c}, {s}, {s}], got {tuple(out.shape)}")
    oy, ox, _, _ = plan.device_tables(x.device)
    index = None if lst is None else lst.device_tables(x.device)[0]
    _lib.check(_lib.lib().eod_scene_stack_gather(x.data_ptr(), out.data_ptr(), B, c, h, w, s, oy.data_ptr(), ox.data_ptr(), plan.nty, plan.ntx,
                                                 _lib.ptr(index), n, current_stream_ptr(x.device)), "eod_scene_stack_gather")
    return out[:n]


def blend_tiles(tiles, plan, out=None):
    """tiles [>= n_tiles, C, tile, tile] fp32 on the GPU (the first n_tiles are read) -> scene [1, C, H, W]: the weighted sum of the
    module docstring.  Every scene element is written.
    `plan` may be a TileSubset: tiles holds its n_tiles listed tiles in the list's order; the result is the full blend at the
    subset's estimated pixels and 0.0 at every other pixel.  Or a TileStack: the result is [B, C, H, W], each scene blended from its own
    tiles.  One call for all of them: eod_scene_stack_blend, B = 1 for a single scene, a null slot_of for the full form."""
    import torch
    from .engine import current_stream_ptr, f32c, require_gpu
    require_gpu(tiles, "blend_tiles")
    plan, B, lst, single = _launch_form(plan)
    n = B * plan.n_tiles if lst is None else lst.n_tiles
    s = plan.tile
    if tiles.dim() != 4 or tiles.shape[0] < n or tuple(tiles.shape[2:]) != (s, s):
        raise _lib.EodError(f"blend_tiles: tiles must be [>= {n}, C, {s}, {s}], got {tuple(tiles.shape)}")
    e = f32c(tiles)
    c = e.shape[1]
    if out is None:
        out = torch.empty((B, c, plan.H, plan.W), dtype=torch.float32, device=e.device)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == B * c * plan.H * plan.W):
        raise _lib.EodError(f"blend_tiles: `out` must be a contiguous fp32 GPU tensor of {'' if single else f'{B} x '}{c} x {plan.H} x {plan.W} elements")
    oy, ox, wy, wx = plan.device_tables(e.device)
    slot_of = None if lst is None else lst.device_tables(e.device)[1]
    _lib.check(_lib.lib().eod_scene_stack_blend(e.data_ptr(), out.data_ptr(), wy.data_ptr(), wx.data_ptr(), oy.data_ptr(), ox.data_ptr(),
                                                _lib.ptr(slot_of), n, B, c, plan.H, plan.W, s, plan.nty, plan.ntx,
                                                current_stream_ptr(e.device)), "eod_scene_stack_blend")
    return out


def keep_known(x, known, subset, out=None):
    """x, known [1, C, H, W] (or [C, H, W]) fp32 on the GPU -> [1, C, H, W]: x at the subset's estimated pixels, `known` at every
    other pixel (the end of a skip_known call: what was never estimated is the known image itself).  With a listed TileStack both are
    [B, C, H, W] and every scene keeps its own.  One call: eod_scene_stack_keep_known, B = 1 for a TileSubset."""
    import torch
    from .engine import current_stream_ptr
    plan, B, lst, single = _launch_form(subset)
    if lst is None:
        raise _lib.EodError(f"keep_known: a TileSubset (or a TileStack with a tile list) is needed, got {type(subset).__name__}")
    a, b = _scene4(x, "keep_known", B, single), _scene4(known, "keep_known", B, single)
    if a.shape != b.shape or tuple(a.shape[2:]) != (plan.H, plan.W) or a.device != b.device:
        raise _lib.EodError(f"keep_known: x {tuple(a.shape)} and known {tuple(b.shape)} must both be [{B}, C, {plan.H}, {plan.W}] on one GPU")
    if out is None:
        out = torch.empty_like(a)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == a.numel()):
        raise _lib.EodError(f"keep_known: `out` must be a contiguous fp32 GPU tensor of {a.numel()} elements")
    oy, ox, _, _ = plan.device_tables(a.device)
    _, slot_of = lst.device_tables(a.device)
    _lib.check(_lib.lib().eod_scene_stack_keep_known(a.data_ptr(), b.data_ptr(), slot_of.data_ptr(), lst.n_tiles, oy.data_ptr(), ox.data_ptr(),
                                                     B, a.shape[1], plan.H, plan.W, plan.tile, plan.nty, plan.ntx, out.data_ptr(),
                                                     current_stream_ptr(a.device)), "eod_scene_stack_keep_known")
    return out


def tile_slots(plan, tile_batch):
    """(chunk, slots): tiles go through the network `chunk` = min(tile_batch, n_tiles) at a time; the last chunk is padded with copies
    of the last tile up to `slots` = a multiple of chunk, so ONE launch program (one batch size) serves the whole call.
    For a TileSubset n_tiles is the number of LISTED tiles."""
    tile_batch = int(tile_batch)
    if tile_batch < 1:
        raise _lib.EodError(f"tile_batch must be at least 1, got {tile_batch}")
    chunk = min(tile_batch, plan.n_tiles)
    return chunk, -(-plan.n_tiles // chunk) * chunk


def gather_padded(scene, plan, tile_batch):
    """gather_tiles into a buffer of tile_slots(...) tiles; the padding slots repeat the last (listed) tile"""
    import torch
    _, B, _, single = _launch_form(plan)
    x = _scene4(scene, "gather_padded", B, single)
    chunk, slots = tile_slots(plan, tile_batch)
    buf = torch.empty((slots, x.shape[1], plan.tile, plan.tile), dtype=torch.float32, device=x.device)
    gather_tiles(x, plan, out=buf)
    if slots > plan.n_tiles:
        buf[plan.n_tiles:] = buf[plan.n_tiles - 1]
    return buf


def tiled_estimate(scene, plan, tile_batch, fn):
    """One scene-sized network estimate: gather the plan's tiles, call fn(x_chunk, lo) -> e_chunk on consecutive chunks (x_chunk
    [chunk, C, tile, tile], tile indices lo .. lo + chunk - 1; indices past n_tiles - 1 are padding, their output is dropped),
    blend.  Allowed because a sample's bits do not depend on the batch it rides in: the result is the same for every tile_batch.
    With a TileSubset for `plan` only the listed tiles are gathered and evaluated: `lo` is then a SLOT number (slot k holds tile
    subset.index[k]; slots past n_tiles - 1 repeat the last listed tile), and the result is 0.0 at pixels that are not estimated."""
    import torch
    chunk, slots = tile_slots(plan, tile_batch)
    x_tiles = gather_padded(scene, plan, tile_batch)
    e_tiles = None
    for lo in range(0, slots, chunk):
        e = fn(x_tiles[lo:lo + chunk], lo)
        if e_tiles is None:
            e_tiles = torch.empty((slots,) + tuple(e.shape[1:]), dtype=torch.float32, device=e.device)
        e_tiles[lo:lo + chunk].copy_(e)  # (a graph-replayed network returns the same buffer every call)
    return blend_tiles(e_tiles, plan)


def scene_stats(stack, out=None):
    """stack [B, C, H, W] fp32 on the GPU (B draws of one scene, or any B scenes of one size) -> (mean, std), each [1, C, H, W]: the
    per-pixel mean and the sample standard deviation (divisor B - 1; B = 1: zeros) over the B members, one pass (eod_scene_stats:
    s = x_0 + x_1 + ... left to right, mean = s / B, q = sum of (x_b - mean)^2 left to right, std = sqrt(q / (B - 1)), every
    operation rounded separately in fp32).  `out`: a contiguous fp32 GPU buffer [2, C, H, W] that receives (mean, std)."""
    import torch
    from .engine import current_stream_ptr, f32c, require_gpu
    require_gpu(stack, "scene_stats")
    if stack.dim() != 4 or stack.shape[0] < 1 or stack.numel() == 0:
        raise _lib.EodError(f"scene_stats: a stack is [B, C, H, W] with B >= 1, got {tuple(stack.shape)}")
    x = f32c(stack)
    b, c, h, w = x.shape
    if out is None:
        out = torch.empty((2, c, h, w), dtype=torch.float32, device=x.device)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (2, c, h, w)):
        raise _lib.EodError(f"scene_stats: `out` must be a contiguous fp32 GPU tensor [2, {c}, {h}, {w}], got {tuple(out.shape)}")
    _lib.check(_lib.lib().eod_scene_stats(x.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), b, c * h * w, current_stream_ptr(x.device)),
               "eod_scene_stats")
    return out[0:1], out[1:2]


MAX_MEMBERS = 64    # members of a stack eod_scene_quantiles / eod_ensemble_stats sort (csrc/ensemble_body.h: ENS_MAXB)
MAX_QUANTILES = 8   # quantiles of one eod_scene_quantiles call


def quantile_ranks(what, q, members):
    """The ranks (k, frac) of the quantiles `q` (a number or a sequence of numbers in [0, 1]) over `members` sorted values, by
    engine.quantile_rank; every refusal of `q` as an EodError"""
    import numbers
    from .engine import quantile_rank
    qs = [q] if isinstance(q, numbers.Real) else q
    try:
        qs = list(qs)
    except TypeError:
        raise _lib.EodError(f"{what}: q is a number or a sequence of numbers in [0, 1], got {q!r}") from None
    for v in qs:
        if isinstance(v, bool) or not isinstance(v, numbers.Real) or not 0.0 <= float(v) <= 1.0:   # (NaN fails the comparison)
            raise _lib.EodError(f"{what}: every quantile is a number in [0, 1], got {v!r}")
    return [quantile_rank(float(v), members) for v in qs]


def scene_quantiles(stack, q=(0.05, 0.5, 0.95), out=None):
    """stack [B, C, H, W] fp32 on the GPU (B <= 64 draws of one scene) -> [Q, C, H, W]: per pixel, the quantiles `q` over the B members
    (eod_scene_quantiles: the members are sorted in registers while the stack streams through once; no temporaries).  The quantile is the
    linear one of numpy / torch.quantile: pos = q * (B - 1) in float64, k = floor(pos), frac = fp32(pos - k) (engine.quantile_rank, the
    rule of DynamicThreshold.rank), the value x_(k) itself at frac = 0 and x_(k) + frac * (x_(k+1) - x_(k)) otherwise, every operation
    rounded separately in fp32.  The order is total: -inf < .. < -0.0 < +0.0 < .. < +inf < NaN, so a NaN member sorts last and an order
    statistic that is a NaN gives a NaN.  Painted pixels of an inpainting are clipped and, at a cloud edge, bimodal: the median and a
    5 % / 95 % band describe them where mean +- std does not.  `out`: a contiguous fp32 GPU buffer [Q, C, H, W] that must not overlap
    the stack."""
    import ctypes
    import torch
    from .engine import current_stream_ptr, f32c, require_gpu
    what = "scene_quantiles"
    if not torch.is_tensor(stack) or stack.dim() != 4 or stack.numel() == 0:
        raise _lib.EodError(f"{what}: a stack is a non-empty tensor [B, C, H, W], got {tuple(getattr(stack, 'shape', ()))}")
    b, c, h, w = (int(v) for v in stack.shape)
    if b > MAX_MEMBERS:
        raise _lib.EodError(f"{what}: at most {MAX_MEMBERS} members are sorted per pixel, the stack has {b}")
    ranks = quantile_ranks(what, q, b)
    if not 1 <= len(ranks) <= MAX_QUANTILES:
        raise _lib.EodError(f"{what}: 1 .. {MAX_QUANTILES} quantiles per call, got {len(ranks)}")
    nq = len(ranks)
    if out is not None and not (torch.is_tensor(out) and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (nq, c, h, w)
                                and out.device == stack.device):
        raise _lib.EodError(f"{what}: `out` must be a contiguous fp32 tensor [{nq}, {c}, {h}, {w}] on the stack's device, got "
                            f"{tuple(getattr(out, 'shape', ()))}")
    require_gpu(stack, what)
    x = f32c(stack)
    if out is None:
        out = torch.empty((nq, c, h, w), dtype=torch.float32, device=x.device)
    else:
        lo, hi = out.data_ptr(), out.data_ptr() + out.numel() * 4
        if lo < x.data_ptr() + x.numel() * 4 and x.data_ptr() < hi:
            raise _lib.EodError(f"{what}: `out` overlaps the stack")
    ks = (ctypes.c_int32 * nq)(*[k for k, _ in ranks])
    fr = (ctypes.c_float * nq)(*[f for _, f in ranks])
    _lib.check(_lib.lib().eod_scene_quantiles(x.data_ptr(), out.data_ptr(), b, c * h * w, ks, fr, nq, current_stream_ptr(x.device)),
               "eod_scene_quantiles")
    return out
