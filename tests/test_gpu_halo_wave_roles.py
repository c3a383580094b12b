"""GPU: the wave roles of the 8-wave 256-column instance of conv3x3_halo_kernel.

In its 3x3 K loop waves 4-7 issue the whole next weight tile in front of their MFMAs and nothing else; waves 0-3 stage the next chunk's
patch behind theirs (all 23 piece groups, up to six per wave) and rewrite it in place; in front of a step's barrier each half waits on
what it owns.  What can go wrong shows as wrong numbers: a wave that reads a weight tile before waves 4-7's DMA has landed, a piece
rewritten before it has landed or read before its rewrite is visible, a scale / shift table read before wave 0's DMA, a piece group that
no wave stages (the zero padding at an image edge is a piece like any other), the prologue's halves of chunk 0.

Which form runs (csrc/igemm.hip, conv_plan; eod_conv_halo_columns): the 8-wave instance takes a halo conv with a fused GroupNorm (or,
split product, a fused skip conv) where N * tiles_per_image * (Cout / 256) >= 256 -- ((Cout - 128) / 256) for the 256 + 128 form of 384
columns -- with tiles_per_image = (H / 8) * (W / 16).  The smallest inputs that still select it are used: N = 2 at 128 x 128 (128 tiles
per image) and N = 4 at 64 x 128 (64 tiles per image, so every image boundary lies between two workgroups' tiles).  All four image edges
lie inside some tile of every case: every case exercises the zero padding.

1. Bit equality: with halo_bn256 = 1 and = 0 the conv output and the GroupNorm statistics it emits are bit-identical -- conv_plan says
   these forms share the K order and the MFMA tiles, and the 4-wave instances know no roles.
2. The same outputs against tests/ref64.py (float64 conv over the operands as stored, the float64 GroupNorm table) at the gates of
   tests/test_gpu_kernels.py (TOL: rel-L2 1e-5 for fp32x3, 5e-3 for fp16 storage)."""
import ctypes
import math

import pytest
import torch

from eo_diffusion_amd import _lib
from eo_diffusion_amd.engine import Act, Program
from tests import ref64
from tests.gpu_util import DEV, TOL
from tests.helpers import rel_l2
from tests.synth import synth_input

pytestmark = pytest.mark.gpu
F64 = torch.float64

GEOMETRIES = [(2, 128, 128), (4, 64, 128)]  # N, H, W
CASES = [  # name, precision, Cin, Cout, GroupNorm groups (0 = none), channels of the fused skip conv's sources
    ("gn-64-256", "fp32x3", 64, 256, 32, ()),
    ("gn-tail-72-256", "fp32x3", 72, 256, 8, ()),          # three chunks of 32, the last one 8 wide
    ("gn-one-chunk-32-256", "fp32x3", 32, 256, 32, ()),    # no next chunk: nothing is staged in the loop
    ("gn-skip-160-256", "fp32x3", 160, 256, 32, (64, 40)),
    ("gn-64-384", "fp32x3", 64, 384, 32, ()),              # 256 + 128: the 8-wave instance, then a 4-wave launch
    ("skip-64-256", "fp32x3", 64, 256, 0, (64,)),          # split product, fused skip, no GroupNorm: no table, pieces are only split
    ("skip-tail-72-256", "fp32x3", 72, 256, 0, (40,)),
    ("f16-gn-64-256", "fp16", 64, 256, 32, ()),            # one chunk of 64
    ("f16-gn-tail-72-256", "fp16", 72, 256, 8, ()),        # two chunks, the second masked
    ("f16-gn-160-256", "fp16", 160, 256, 32, ()),          # three chunks, the last one half
]


def expected_columns(N, H, W, cout, bn256):
    """the rule of the module docstring, for the cases of this file (every one has a fused GroupNorm or, split product, a fused skip)"""
    tiles = (H // 8) * (W // 16)
    if bn256 and cout % 256 == 0 and N * tiles * (cout // 256) >= 256:
        return 256
    if bn256 and cout > 256 and cout % 256 == 128 and N * tiles * ((cout - 128) // 256) >= 256:
        return 256
    return 128


def stored(t, prec):
    return t.half().float() if prec == "fp16" else t


def operands(name, prec, N, H, W, cin, cout, groups, skip_c):
    x = synth_input(f"wrx{name}", (N, cin, H, W), 83, scale=1.2) + 0.15
    w = synth_input(f"wrw{name}", (cout, cin, 3, 3), 83, scale=1.0 / math.sqrt(9 * cin))  # independent per tap
    b = synth_input(f"wrb{name}", (cout,), 83, scale=0.1)
    gn = None
    if groups:
        gn = (1.0 + 0.2 * synth_input(f"wrg{name}", (cin,), 83), 0.1 * synth_input(f"wre{name}", (cin,), 83))
    xk = wk = None
    if skip_c:
        xk = synth_input(f"wrxk{name}", (N, sum(skip_c), H, W), 83)
        wk = synth_input(f"wrwk{name}", (cout, sum(skip_c), 1, 1), 83, scale=1.0 / math.sqrt(sum(skip_c)))
    return x, w, b, gn, xk, wk


def run_conv(prec, x, w, b, gn, groups, xk, wk, skip_c, bn256):
    """-> (y NHWC as stored, statistics slots, columns per workgroup), all on the device"""
    L = _lib.lib()
    prev = L.eod_set_option(b"halo_bn256", int(bn256))
    try:
        N = x.shape[0]
        prog = Program(DEV, prec)
        to_act = lambda t: Act(prog.own(t.to(DEV).permute(0, 2, 3, 1).contiguous().to(prog.tdtype)), N, t.shape[2], t.shape[3], t.shape[1])
        a = to_act(x)
        cout = w.shape[0]
        g = sk = None
        if gn is not None:
            g = (prog.gn_stats([a], prog.f32(gn[0].to(DEV)), prog.f32(gn[1].to(DEV)), groups=groups), True)
        if skip_c:
            c0 = skip_c[0]
            ax = [to_act(xk[:, :c0])] + ([to_act(xk[:, c0:])] if len(skip_c) > 1 else [])
            assert prog.conv_skip_ok(a, cout, ax), "the fused 1x1 skip conv is what this case is about"
            sk = (ax, wk.to(DEV), None)
        y, i = prog.conv(a, prog.pack_conv(w.to(DEV)), prog.f32(b.to(DEV)), cout, gn=g, skip=sk, stats=True)
        d = prog.ops[i].u.conv
        assert L.eod_conv_kernel_name(ctypes.byref(d)).decode() == "conv3x3_halo_kernel"
        assert gn is None or d.gn_scale_shift, "the GroupNorm was not fused into the patch staging"
        assert not d.workspace and y.stats is not None, "unsplit in K, with statistics slots"
        cols = L.eod_conv_halo_columns(ctypes.byref(d))
        prog.run()
        torch.cuda.synchronize()
        return y.t.clone(), y.stats[0].clone(), cols
    finally:
        L.eod_set_option(b"halo_bn256", prev)


@pytest.mark.parametrize("geom", GEOMETRIES, ids=lambda g: "x".join(str(v) for v in g))
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_roles_give_the_bits_of_the_4_wave_form_and_meet_the_reference(case, geom):
    name, prec, cin, cout, groups, skip_c = case
    N, H, W = geom
    x, w, b, gn, xk, wk = operands(name, prec, N, H, W, cin, cout, groups, skip_c)
    y8, s8, c8 = run_conv(prec, x, w, b, gn, groups, xk, wk, skip_c, 1)
    y4, s4, c4 = run_conv(prec, x, w, b, gn, groups, xk, wk, skip_c, 0)
    assert (c8, c4) == (expected_columns(N, H, W, cout, 1), expected_columns(N, H, W, cout, 0)) == (256, 128), (c8, c4)
    assert torch.isfinite(y8).all() and torch.isfinite(s8).all()
    ny, ns = int((y8 != y4).sum()), int((s8 != s4).sum())
    print(f"{name} {geom}: {ny} of {y8.numel()} outputs and {ns} of {s8.numel()} statistics differ between the 8-wave and the 4-wave form")
    assert torch.equal(y8, y4), f"{ny} output elements differ from the 4-wave form"
    assert torch.equal(s8, s4), f"{ns} statistics slots differ from the 4-wave form"
    # float64 reference over the stored operands, on the device
    xs = stored(x, prec).to(DEV).permute(0, 2, 3, 1).to(F64)
    kw = {}
    if gn is not None:
        kw = dict(gn_scale_shift=ref64.group_norm_scale_shift(xs.reshape(N, H * W, cin), gn[0].to(DEV), gn[1].to(DEV), groups, 1e-5), gn_silu=True)
    if skip_c:
        kw.update(skip_x=stored(xk, prec).to(DEV).permute(0, 2, 3, 1).to(F64), skip_w=stored(wk, prec).to(DEV))
    ref = ref64.conv_forward(xs, None, stored(w, prec).to(DEV), ksize=3, bias=b.to(DEV), **kw)
    assert y8.shape == ref.shape
    err = rel_l2(y8.to(F64), ref)
    print(f"{name} {geom}: rel-L2 {err:.3e} (gate {TOL[prec]:.0e})")
    assert err < TOL[prec], err
