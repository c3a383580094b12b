"""GPU: the edges of the halo conv kernels -- what runs in front of the first LDS-DMA and behind the last MFMA (csrc/igemm.hip:
edge_issue / edge_finish, ab_bound_issue / ab_bound_finish in csrc/common.h, the GroupNorm statistics of halo_epilogue_direct).

The split-product kernels load their epilogue operands (bias, per-sample bias, the weights' row exponents) and their activation bound
tables as unconditional buffer loads behind the DMA of the first chunk: descriptors with exact num_records stand in for the `if`s, so
a column tail or an absent tensor reads zeros.  The 32-entry maximum of a bound table and the 16-lane sums of the statistics go through
DPP row rotations instead of ds_bpermute.  What can go wrong shows as wrong numbers or wrong bits: a descriptor whose base or length
belongs to another table (the second image's per-sample bias row, the class block of the parity-class weights' exponents, the 256 + 128
form's column base), a quad behind Ncols that reads its neighbour's values, an absent bias that turns a per-sample -0 into +0 or an
absent per-sample bias that adds 0 to the bias, a bound maximum that misses table entries 16 .. 31 or a NaN entry, a scale consumed
before its load has landed (chunk 0's rewrite), a rotation that sums a lane twice and another never.

Every case checks two things:
1. the output and the emitted statistics slots are bit-identical to what the library BEFORE this change computed:
   tests/golden/halo_edges_parent.json holds their SHA-256 values, recorded on an MI355X with the library built from the parent commit
   (`python -m tests.test_gpu_halo_edges <file>` writes such a file with whatever library is loaded);
2. the same output is within TOL (tests/gpu_util.py: rel-L2 1e-5 for fp32x3, 5e-3 for fp16 storage) of the float64 conv of
   tests/ref64.py over the operands as stored, and the slots, summed, are within (n + 3) 2^-24 of the float64 sums of the stored output
   relative to the sums of absolute values, n the pixels per slot (any order of an fp32 sum of n terms, one rounding per square; fp16
   storage adds 2^-10: the sums may be taken before the output is rounded -- the ceilings of tests/test_gpu_up4_class_patch.py).

Operands come from tests/synth.py on the CPU (the digests must not depend on a device generator); the descriptor plumbing, the weight
packing and the reference chunks are those of tests/test_gpu_conv_programs.py.  fp32x3: the last image of a batch is scaled by 2^10,
and the maximum of an image's bound table sits at entry (7 n + 3) % 32 -- in the second 16-lane row for n = 2 -- so the images need
different scales and both rows of the table.

Cases, on the smallest shapes that can go wrong (fp32x3 unless named fp16):
- 4-wave instance, N = 2 at 16 x 32 (two tile rows and columns: every tile has border and interior sides; the second image's
  per-sample bias row), Cin 72 (three chunks, the last 8 wide): Cout 128, 72 and 200 (the last two put whole quads behind Ncols in
  the last tile) x {bias, per-sample bias, both, none}; at Cout 200 with both: GroupNorm on / off x {plain, residual, fused skip} x
  statistics on / off.  N = 1 at 8 x 16 (one tile, all four edges), Cin 32 (one chunk: prologue only): three mixes of the above.
  These small maps run the 64-column tiles of the 4-wave instance; two 32-row maps run its 128-column tiles.
- K slices (16 x 16 map at N = 1, 128 channels = four chunks), the masked half tile (8 x 8 map), the virtual-upsample instance.
- 8-wave instance: (2, 128, 128) and (4, 64, 128) with Cout 256 and 384 (256 + 128), GroupNorm and GroupNorm + skip;
  eod_conv_halo_columns proves the form that ran.
- one smallest selecting case each of both parity-class upsample forms, the stride-2 kernel, the first conv, the head conv and a
  qkv-style 1 x 1 with pre-split output (its scale comes from y_presplit_bound in the epilogue).
- fp16 storage: one GroupNorm case on each of the 4-wave and the 8-wave instance."""
import ctypes
import hashlib
import json
import math
import os

import pytest
import torch

from tests import ref64
from tests.gpu_util import TOL
from tests.helpers import rel_l2
from tests.synth import synth_input
from tests.test_gpu_conv_programs import DEV, F64, NAN, _act, _amax_input, _fields, _geom, _image_scales, _L, _lib, _ok, _p, _pack_weights, _reference, _st

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "halo_edges_parent.json")
HALO, UP4, S2, FIRST, HEAD, GENERIC = ("conv3x3_halo_kernel", "conv_up4_halo_kernel", "conv_s2_halo_kernel", "conv_first_x3_kernel",
                                       "conv_head_kernel", "igemm_kernel")


class SynthRng:
    """the randn / rand of tests.test_gpu_conv_programs.Rng, drawn on the CPU from tests/synth.py: a pure function of (tag, draw index)"""

    def __init__(self, tag):
        self.tag, self.k = tag, 0

    def _next(self, shape, uniform):
        self.k += 1
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        return synth_input(f"he:{self.tag}:{self.k}", shape, 89, uniform=uniform).to(DEV)

    def randn(self, shape, scale=1.0, shift=0.0):
        return self._next(shape, False) * scale + shift

    def rand(self, shape, lo=0.0, hi=1.0):
        return self._next(shape, True) * (hi - lo) + lo


def bound_table(amax, r):
    """[N][32] fp32 whose per-image maximum lies between 1x and 2x amax[n], at entry (7 n + 3) % 32, smaller entries elsewhere"""
    N = amax.shape[0]
    tab = r.rand((N, 32), 0.0, 0.5) * amax[:, None].float()
    n = torch.arange(N, device=DEV)
    f = 1.0 + ((n * 0.37 + 0.11) % 0.99)
    tab[n, (n * 7 + 3) % 32] = (amax.double() * f.double()).float()
    assert bool((tab.max(1).values.double() >= amax.double()).all())
    return tab.contiguous()


def _cases():
    lib = _lib()
    F32, F16 = lib.EOD_F32, lib.EOD_F16
    C = []

    def add(name, kernel, g, cols=None, ksplit=None):
        C.append((name, kernel, g, cols, ksplit))

    # 4-wave instance: operands x Cout
    for cout in (128, 72, 200):
        for ops, kw in (("bias", dict()), ("cbias", dict(bias=False, cbias=cout + 8)), ("both", dict(cbias=cout + 8)), ("none", dict(bias=False))):
            add(f"w4-2x16x32-72-{cout}-{ops}", HALO, _geom(F32, 2, 16, 32, 72, cout, w_split=1, stats=True, **kw))
    # ... flags at Cout 200 (the fused skip conv's bias rides in the per-sample bias slot: its cases carry the bias only)
    for gn in (None, "silu"):
        for form, kw in (("plain", dict(cbias=208)), ("res", dict(cbias=208, res=True)), ("skip", dict(skip=(40, 24)))):
            for stats in (True, False):
                if gn is None and form == "plain" and stats:
                    continue  # (the "both" case above)
                add(f"w4-2x16x32-72-200-{'gn' if gn else 'nogn'}-{form}-{'stats' if stats else 'nostats'}", HALO,
                    _geom(F32, 2, 16, 32, 72, 200, w_split=1, gn=gn, stats=stats, **kw))
    # ... one tile, one chunk
    add("w4-1x8x16-32-128-gn-bias", HALO, _geom(F32, 1, 8, 16, 32, 128, w_split=1, gn="silu", stats=True))
    add("w4-1x8x16-32-72-none", HALO, _geom(F32, 1, 8, 16, 32, 72, w_split=1, bias=False, stats=True))
    add("w4-1x8x16-32-200-skip", HALO, _geom(F32, 1, 8, 16, 32, 200, w_split=1, skip=(40, 0), stats=True))
    # ... the 128-column tiles (maps of 16 and more tiles per 128 columns at the nominal batch; the maps above run 64-column tiles)
    add("w4-c128-1x32x32-72-200-gn-both", HALO, _geom(F32, 1, 32, 32, 72, 200, w_split=1, gn="silu", stats=True, cbias=0), cols=128)
    add("w4-c128-1x32x64-32-128-bias-res", HALO, _geom(F32, 1, 32, 64, 32, 128, w_split=1, stats=True, res=True), cols=128)
    # other launch forms of the halo kernel
    add("kslices-1x16x16-128-128", HALO, _geom(F32, 1, 16, 16, 128, 128, w_split=1, stats=True, cbias=0), ksplit=True)
    add("halftile-1x8x8-72-136", HALO, _geom(F32, 1, 8, 8, 72, 136, w_split=1, stats=True, res=True))
    add("ups-1x8x16-32-128", HALO, _geom(F32, 1, 8, 16, 32, 128, w_split=1, upsample=1, stats=True))
    # 8-wave instance
    for N, H, W in ((2, 128, 128), (4, 64, 128)):
        for cout in (256, 384):
            add(f"w8-{N}x{H}x{W}-32-{cout}-gn", HALO, _geom(F32, N, H, W, 32, cout, w_split=1, gn="silu", stats=True, cbias=cout), cols=256)
            add(f"w8-{N}x{H}x{W}-72-{cout}-gn-skip", HALO, _geom(F32, N, H, W, 72, cout, w_split=1, gn="silu", skip=(40, 0), stats=True), cols=256)
    # other kernels
    add("up4-1x16x32-24-72", UP4, _geom(F32, 1, 16, 32, 24, 72, w_split=1, upsample=3, stats=True, cbias=0))
    add("up4-w8-1x64x128-32-256", UP4, _geom(F32, 1, 64, 128, 32, 256, w_split=1, upsample=3, stats=True), cols=256)
    add("s2-2x63x63-16-136", S2, _geom(F32, 2, 63, 63, 16, 136, w_split=1, stride=2, stats=True, cbias=136))
    add("first-2x32x32-4-128", FIRST, _geom(F32, 2, 32, 32, 4, 128, w_split=1, w_tapmajor=1, stats=True))
    add("head-2x16x32-128-3", HEAD, _geom(F32, 2, 16, 32, 128, 3, w_split=1, gn="silu", nchw=True))
    add("qkv-3x16x16-96-200-psout", GENERIC, _geom(F32, 3, 16, 16, 96, 200, ksize=1, pad=0, w_split=1, y_presplit=True))
    # fp16 storage
    add("f16-w4-2x16x32-72-128-gn", HALO, _geom(F16, 2, 16, 32, 72, 128, gn="silu", stats=True, cbias=136))
    add("f16-w8-2x128x128-64-256-gn", HALO, _geom(F16, 2, 128, 128, 64, 256, gn="silu", stats=True), cols=256)
    return C


CASES = _cases()


def digest(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def run_case(case):
    """-> dict(y as stored, statistics slots or None, float64 output, float64 reference, pixels per slot, precision)"""
    name, kernel, g, cols, ksplit = case
    L, st, lib = _L(), _st(), _lib()
    r = SynthRng(name)
    nn = set(g["nn"])
    f16 = g["dtype"] == lib.EOD_F16
    td, dt = (torch.float16, lib.EOD_F16) if f16 else (torch.float32, lib.EOD_F32)
    split = bool(g["w_split"])
    N, H, W, C0, C1, Cout, Ho, Wo = (g[k] for k in ("N", "H", "W", "C0", "C1", "Cout", "Ho", "Wo"))
    w, sw, wp, keep, K, extra = _pack_weights(g, r, f16, td, dt)
    x = _act(r, (N, H, W, C0), f16, zero_from=extra.get("creal"))
    if split and "a_bound" in nn:
        _image_scales(x, N)
    ss = torch.stack([r.randn((N, C0 + C1), 0.8), r.randn((N, C0 + C1), 0.3)], -1).contiguous() if "gn_scale_shift" in nn else None
    bias = r.randn((Cout,), 0.1) if "bias" in nn else None
    cbias = r.randn(((N - 1) * g["cbias_stride"] + Cout,), 0.2) if "cbias" in nn else None
    res = (lambda t: t.half() if f16 else t)(r.randn((N, Ho, Wo, Cout), 0.5)) if "res" in nn else None
    sx = sx2 = None
    if "skip_x" in nn:
        sx = _act(r, (N, Ho, Wo, g["skip_C0"]), f16)
        sx2 = _act(r, (N, Ho, Wo, g["skip_C1"]), f16) if g["skip_C1"] else None
        if split and "skip_bound" in nn and N >= 2:  # the launch runs on the smaller of the two operand scales: here the skip tensor's
            sx[0] *= 2.0 ** 8
    ptr = dict(wp)
    if "a_bound" in nn:
        ptr["a_bound"] = bound_table(_amax_input(g, x, None, ss), r)
    if "skip_bound" in nn:
        cat = sx if sx2 is None else torch.cat([sx, sx2], -1)
        ptr["skip_bound"] = bound_table(cat.abs().amax((1, 2, 3)).double(), r)
    ref, _ = _reference(g, x, None, w, ss, bias, cbias, res, sx, sx2, sw, extra.get("class_w"))
    ps_scale = None
    if "y_presplit_bound" in nn:
        ptr["y_presplit_bound"] = bound_table(ref.abs().amax((1, 2, 3)), r)
        ps_scale = ref64.presplit_scale(ptr["y_presplit_bound"], kmin=ref64.AB_KMIN_ATTN)
    ptr.update(x=x.contiguous(), bias=bias, cbias=cbias, res=res, gn_scale_shift=ss, skip_x=sx, skip_x2=sx2)
    nchw = bool(g["out_nchw_f32"])
    ydt = torch.float32 if (nchw or not f16) else torch.float16
    y = torch.full((N, Cout, Ho, Wo) if nchw else (N, Ho, Wo, Cout), NAN, dtype=ydt, device=DEV)
    vals, ptrs_all = _fields()
    d = lib.ConvDesc()
    for k in vals:
        setattr(d, k, g[k])
    d.workspace_bytes, d.stats_slots = 0, 0
    for k in ptrs_all:
        if k in nn and k not in ("y", "stats", "workspace"):
            assert ptr.get(k) is not None, (k, name)
            setattr(d, k, ptr[k].data_ptr())
    d.y = y.data_ptr()
    ws_bytes = L.eod_conv_workspace_size(ctypes.byref(d))
    ws = torch.full((ws_bytes // 4,), NAN, dtype=torch.float32, device=DEV) if ws_bytes else None
    d.workspace, d.workspace_bytes = _p(ws), ws_bytes
    stats, slots = None, 0
    if "stats" in nn:
        slots = L.eod_conv_stats_slots(ctypes.byref(d))
        assert slots > 0, name
        stats = torch.full((N, slots, Cout, 2), NAN, dtype=torch.float32, device=DEV)
        d.stats, d.stats_slots = stats.data_ptr(), slots
    # the form this case is about
    got_kernel = L.eod_conv_kernel_name(ctypes.byref(d)).decode()
    assert got_kernel == kernel, (got_kernel, name)
    if cols is not None:
        assert L.eod_conv_halo_columns(ctypes.byref(d)) == cols, (L.eod_conv_halo_columns(ctypes.byref(d)), name)
    if ksplit is not None:
        assert bool(ws_bytes) == ksplit, (ws_bytes, name)
    _ok(L.eod_conv2d_igemm(ctypes.byref(d), st), "conv2d_igemm " + name)
    torch.cuda.synchronize()
    if ps_scale is not None:
        got = ref64.presplit_decode(y, ps_scale)
    else:
        got = (y.permute(0, 2, 3, 1) if nchw else y).to(F64)
    return dict(y=y, stats=stats, got=got, ref=ref, n=Ho * Wo / max(slots, 1), prec="fp16" if f16 else "fp32x3" if split else "fp32")


@pytest.fixture(scope="module")
def parent():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_edges_give_the_parents_bits_and_meet_the_reference(case, parent):
    name = case[0]
    o = run_case(case)
    y, stats, got, ref, prec = o["y"], o["stats"], o["got"], o["ref"], o["prec"]
    assert bool(torch.isfinite(got).all()) and (stats is None or bool(torch.isfinite(stats).all())), name
    # 2. (printed first) float64 reference over the stored operands
    err = rel_l2(got, ref)
    print(f"{name}: rel-L2 {err:.3e} (gate {TOL[prec]:.0e})")
    serr = ceil = None
    if stats is not None:
        sref = ref64.stats_of(y)
        yd = y.to(F64)
        den = torch.stack([yd.flatten(1, -2).abs().sum(1), yd.flatten(1, -2).square().sum(1)], -1)
        serr = float(((stats.to(F64).sum(1) - sref).abs() / den.clamp_min(1e-300)).max())
        ceil = (o["n"] + 3) * 2.0 ** -24 + (2.0 ** -10 if prec == "fp16" else 0.0)
        print(f"{name}: statistics, worst sum {serr:.3e} (ceiling {ceil:.3e})")
    # 1. the parent library's bits
    rec = parent[name]
    assert digest(y) == rec["y"], "the output differs from the parent library's"
    assert (None if stats is None else digest(stats)) == rec["stats"], "the statistics slots differ from the parent library's"
    assert err < TOL[prec], err
    assert serr is None or serr <= ceil, serr


if __name__ == "__main__":  # record the digests of the loaded library: python -m tests.test_gpu_halo_edges out.json
    import sys

    out = {}
    for c in CASES:
        o = run_case(c)
        out[c[0]] = {"y": digest(o["y"]), "stats": None if o["stats"] is None else digest(o["stats"])}
        print(c[0], flush=True)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print(f"{len(out)} cases -> {sys.argv[1]}")
