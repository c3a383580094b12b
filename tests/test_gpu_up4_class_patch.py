"""GPU: the class-exact patch of conv_up4_halo_kernel's forward instances (fp32 storage with the split product, fp16 storage) and the
8-wave 256-column instance of the split product.

A workgroup of the parity-class upsample conv stages the 9 x 17 window of the stored map that its class (p, q) reads -- origin
(ty0 - 1 + p, tx0 - 1 + q), 153 rows in 20 groups, five pieces per wave, issued 3 + 2 in the first two steps of a chunk -- instead of
the whole 10 x 18 halo patch.  What can go wrong shows as wrong numbers: a window at the wrong origin (a class at another parity, an
O(1) error with weights that are independent per tap), a fragment address that still carries the class offset, a swizzle key taken
from another column than the one the piece was written with, a piece group that no wave stages or splits (the zero padding is a piece
like any other), a row of the last group (rows 153 .. 159 of it lie behind the window) read as data.

The 8-wave instance (2 x 4 waves, two 128-column tiles of one class per workgroup, wave roles in the K loop: waves 4-7 issue the next
weight tile in front of their MFMAs, waves 0-3 stage and split the next chunk's window behind theirs) adds: a wave that reads a weight
tile before waves 4-7's DMA has landed, a piece split before it has landed or read before its split is visible, the prologue's shares
of chunk 0 (three pieces to wave row 0, two to wave row 1, half a weight tile each), the second column tile's weights and statistics.
Which form runs (csrc/igemm.hip, conv_plan; eod_conv_halo_columns): the split product takes the 8-wave form where
N * (H / 8) * ceil(W / 16) * 4 * (Cout / 256) >= 256 -- ((Cout - 128) / 256) for the 256 + 128 form of 384 columns, whose last 128 run
on the 4-wave form -- and halo_bn256 is not 0; fp16 storage never does.

Every case shows three things:
1. the output and the GroupNorm statistics slots are bit-identical with halo_bn256 = 1 and = 0 (conv_plan: every form of this family
   shares the K order and the MFMA tiles);
2. both are bit-identical to what the library BEFORE this change computed: tests/golden/up4_class_patch_parent.json holds the SHA-256
   of the output bytes and of the slot bytes of every case, recorded on an MI355X with the library built from the parent commit
   (`python -m tests.test_gpu_up4_class_patch <file>` writes such a file with whatever library is loaded);
3. the output is within the gate this kernel has in tests/test_gpu_halo_tap_order.py (tests/test_gpu_kernels.py TOL: rel-L2 1e-5 for
   fp32x3, 5e-3 for fp16 storage) of the float64 conv3x3(nearest2x(x)) of tests/ref64.py over the operands as stored -- over all of it
   and over each of the four output parities by itself -- and the slots, summed, are within (n + 3) 2^-24 of the float64 sums of the
   stored output relative to the sums of absolute values, n the pixels per slot (any order of an fp32 sum of n terms, one rounding per
   square; the ceiling of tests/test_gpu_glue_ops.py).  fp16 storage adds 2^-10: the sums may be taken before the output is rounded
   to fp16, which moves a value by 2^-11 of itself and its square by twice that.

Geometries (stored map): 8 x 16 is one tile whose every halo row and column is padding, N = 1; 16 x 32 has two tile rows and two tile
columns, so every tile has interior and border sides, N = 2; 16 x 8 leaves the right half of every tile behind the map.  Channels:
32 = one chunk of fp32 storage (prologue only), 72 = three chunks with a tail of 8, and in fp16 storage 72 = one chunk of 64 and a
tail.  Output columns: 128, 256, 384 and 512 (one to four column tiles per class).  These maps are below the rule: both option arms
run the 4-wave form.  For the 8-wave instance the smallest maps that select it: 64 x 128 at N = 1 and 32 x 64 at N = 4 (64 tiles, the
bound for 256 and 384 columns; 512 columns are two workgroups per tile and class), and 256 x 8 at N = 2 (the right half of every tile
behind the map); 32 and 72 channels; 256, 384 (256 + 128) and 512 columns."""
import ctypes
import hashlib
import json
import math
import os

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
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "up4_class_patch_parent.json")

GEOMETRIES = [(1, 8, 16), (2, 16, 32), (2, 16, 8)]  # N, H, W of the stored map
CHANNELS = [("fp32x3", 32), ("fp32x3", 72), ("fp16", 72)]
COUTS = [128, 256, 384, 512]
GEOMETRIES_W8 = [(1, 64, 128), (4, 32, 64), (2, 256, 8)]
CASES = [(prec, cin, cout, geom) for prec, cin in CHANNELS for cout in COUTS for geom in GEOMETRIES]
CASES += [("fp32x3", cin, cout, geom) for cin in (32, 72) for cout in (256, 384, 512) for geom in GEOMETRIES_W8]


def expected_columns(prec, N, H, W, cout, bn256):
    """the rule of the module docstring"""
    wg = N * (H // 8) * ((W + 15) // 16) * 4
    if prec == "fp32x3" and bn256 and cout % 256 == 0 and wg * (cout // 256) >= 256:
        return 256
    if prec == "fp32x3" and bn256 and cout > 256 and cout % 256 == 128 and wg * ((cout - 128) // 256) >= 256:
        return 256
    return 128


def case_id(case):
    prec, cin, cout, (N, H, W) = case
    return f"{prec}-{cin}-{cout}-{N}x{H}x{W}"


def operands(case):
    prec, cin, cout, (N, H, W) = case
    tag = case_id(case)
    x = synth_input(f"cpx{tag}", (N, cin, H, W), 97, scale=1.2) + 0.15
    w = synth_input(f"cpw{tag}", (cout, cin, 3, 3), 97, scale=1.0 / math.sqrt(9 * cin))  # independent per tap
    b = synth_input(f"cpb{tag}", (cout,), 97, scale=0.1)
    return x, w, b


def run_conv(prec, x, w, b, bn256):
    """-> (y NHWC as stored, statistics slots [N][P][C][2], P, columns per workgroup), on the device"""
    L = _lib.lib()
    prev = L.eod_set_option(b"halo_bn256", int(bn256))
    try:
        N, cin, H, W = x.shape
        cout = w.shape[0]
        prog = Program(DEV, prec)
        a = Act(prog.own(x.to(DEV).permute(0, 2, 3, 1).contiguous().to(prog.tdtype)), N, H, W, cin)
        assert prog.conv_up4_ok(a, cout)
        y, i = prog.conv(a, prog.pack_conv_up4(w.to(DEV)), prog.f32(b.to(DEV)), cout, upsample="up4", stats=True)
        d = prog.ops[i].u.conv
        assert L.eod_conv_kernel_name(ctypes.byref(d)).decode() == "conv_up4_halo_kernel"
        assert y.stats is not None and y.stats[1] == (H // 8) * ((W + 15) // 16) * 8, "(tile, class, wave row) slots"
        cols = L.eod_conv_halo_columns(ctypes.byref(d))
        prog.run()
        torch.cuda.synchronize()
        return y.t.clone(), y.stats[0].clone(), y.stats[1], cols
    finally:
        L.eod_set_option(b"halo_bn256", prev)


def digest(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


@pytest.fixture(scope="module")
def parent():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_class_window_gives_the_parents_bits_and_meets_the_reference(case, parent):
    prec, cin, cout, (N, H, W) = case
    x, w, b = operands(case)
    y1, s1, P, c1 = run_conv(prec, x, w, b, 1)
    y0, s0, _, c0 = run_conv(prec, x, w, b, 0)
    assert (c1, c0) == (expected_columns(prec, N, H, W, cout, 1), expected_columns(prec, N, H, W, cout, 0)), (c1, c0)
    assert (c1, c0) == ((256, 128) if (N, H, W) in GEOMETRIES_W8 else (128, 128)), "the instance this case is about did not run"
    assert y1.shape == (N, 2 * H, 2 * W, cout) and torch.isfinite(y1).all() and torch.isfinite(s1).all()
    # 1. the option arms
    assert torch.equal(y1, y0), f"{int((y1 != y0).sum())} output elements differ between halo_bn256 = 1 and 0"
    assert torch.equal(s1, s0), f"{int((s1 != s0).sum())} statistics slots differ between halo_bn256 = 1 and 0"
    # 2. the parent library's bits
    rec = parent[case_id(case)]
    assert digest(y1) == rec["y"], "the output differs from the parent library's"
    assert digest(s1) == rec["stats"], "the statistics slots differ from the parent library's"
    # 3. float64 reference over the stored operands, on the device (the class kernels are summed in fp32 before they are rounded:
    #    the weight enters unrounded, as in tests/test_gpu_halo_tap_order.py)
    xs = (x.half().float() if prec == "fp16" else x).to(DEV).permute(0, 2, 3, 1).to(F64)
    ref = ref64.conv_forward(xs, None, w.to(DEV), ksize=3, upsample=1, bias=b.to(DEV))
    assert y1.shape == ref.shape
    got = y1.to(F64)
    err = rel_l2(got, ref)
    cls = [rel_l2(got[:, p::2, q::2], ref[:, p::2, q::2]) for p in (0, 1) for q in (0, 1)]
    print(f"{case_id(case)}: rel-L2 {err:.3e}, per class {' '.join(f'{e:.3e}' for e in cls)} (gate {TOL[prec]:.0e})")
    assert err < TOL[prec], err
    assert max(cls) < TOL[prec], cls
    n = 4 * H * W / P
    sref = ref64.stats_of(y1)
    den = torch.stack([got.flatten(1, -2).abs().sum(1), got.flatten(1, -2).square().sum(1)], -1)
    serr = float(((s1.to(F64).sum(1) - sref).abs() / den).max())
    ceil = (n + 3) * 2.0 ** -24 + (2.0 ** -10 if prec == "fp16" else 0.0)
    print(f"{case_id(case)}: statistics, worst sum {serr:.3e} (ceiling {ceil:.3e})")
    assert serr <= ceil, serr


if __name__ == "__main__":  # record the digests of the loaded library: python -m tests.test_gpu_up4_class_patch out.json
    import sys

    out = {}
    for c in CASES:
        y, s = run_conv(c[0], *operands(c), 1)[:2]
        out[case_id(c)] = {"y": digest(y), "stats": digest(s)}
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print(f"{len(out)} cases -> {sys.argv[1]}")
