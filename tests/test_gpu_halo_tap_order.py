"""GPU: the tap order and the A-fragment row window of the halo convs (conv3x3_halo_kernel's 16x16x32 paths, conv_up4_halo_kernel).

The 3x3 taps of a channel chunk run dx-major and the A fragments of the three steps of one dx live in a rotating window of patch rows;
on the 8-wave 256-column instance steps 1..8 of a chunk read their new rows one step early, the first step behind its barrier.  What can go wrong: a weight
tile paired with another tap's window (the weights here are independent per tap, so a swapped or transposed tap is an O(1) error), a
window row in the wrong register after a rotation (chunk boundaries, tile rows), a fragment read from the next chunk's patch buffer
before that chunk's rewrite is visible, a window that leaks into the fused skip phase.

Reference: tests/ref64.py (float64 conv over the operands as stored), at the gates of tests/test_gpu_kernels.py (TOL: rel-L2 1e-5 for
fp32x3, 5e-3 for fp16 storage).  fp16 storage: the reference is built from the fp16-rounded input and weight.  The GroupNorm table of
the reference is the float64 one of ref64.group_norm_scale_shift over the same stored input."""
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


def _stored(t, prec):
    return t.half().float() if prec == "fp16" else t


def _gamma_beta(C, wide):
    """wide: per-channel gamma of 32-channel blocks 1e3, 1e-3, 1e1, 1e-1, ... (the chunks of a conv differ by up to 10^6), signs mixed"""
    g = 1.0 + 0.2 * synth_input("tog", (C,), 71)
    if wide:
        mag = torch.tensor([1e3, 1e-3, 1e1, 1e-1])[(torch.arange(C) // 32) % 4]
        g = g * mag * torch.where(torch.arange(C) % 3 == 0, -1.0, 1.0)
    return g, 0.1 * synth_input("toe", (C,), 71) * (g.abs() if wide else 1.0)


class Options:
    """library options for the length of a with block (name -> value), restored afterwards"""

    def __init__(self, **kw):
        self.kw, self.prev = kw, {}

    def __enter__(self):
        for k, v in self.kw.items():
            self.prev[k] = _lib.lib().eod_set_option(k.encode(), int(v))

    def __exit__(self, *exc):
        for k, v in self.prev.items():
            _lib.lib().eod_set_option(k.encode(), v)


def run_conv(prec, x, w, b, *, gn=None, skip=None, up4=False, n=None):
    """x NCHW fp32 (cpu), first n images -> (y NHWC as stored (cpu), GroupNorm table the kernel used or None, workspace used)"""
    n = n or x.shape[0]
    prog = Program(DEV, prec)
    to_act = lambda t: Act(prog.own(t[:n].to(DEV).permute(0, 2, 3, 1).contiguous().to(prog.tdtype)), n, t.shape[2], t.shape[3], t.shape[1])
    a = to_act(x)
    Cout = w.shape[0]
    g = ss = None
    if gn is not None:
        ss = prog.gn_stats([a], prog.f32(gn[0].to(DEV)), prog.f32(gn[1].to(DEV)))
        g = (ss, True)
    sk = None
    if skip is not None:
        ax = [to_act(skip[0])]
        assert prog.conv_skip_ok(a, Cout, ax), "the fused 1x1 skip conv is what this case is about"
        sk = (ax, skip[1].to(DEV), None)
    if up4:
        assert prog.conv_up4_ok(a, Cout)
        y, i = prog.conv(a, prog.pack_conv_up4(w.to(DEV)), prog.f32(b.to(DEV)), Cout, upsample="up4")
    else:
        y, i = prog.conv(a, prog.pack_conv(w.to(DEV)), prog.f32(b.to(DEV)), Cout, gn=g, skip=sk)
    d = prog.ops[i].u.conv
    name = _lib.lib().eod_conv_kernel_name(ctypes.byref(d)).decode()
    assert name.startswith("conv_up4_halo_kernel" if up4 else "conv3x3_halo_kernel"), name
    assert gn is None or d.gn_scale_shift, "the GroupNorm was not fused into the patch staging"
    used = bool(d.workspace)
    prog.run()
    torch.cuda.synchronize()
    return y.t.cpu(), (ss.cpu() if ss is not None else None), used


def reference(prec, x, w, b, *, gn=None, skip=None, up=False, table=None):
    """float64 NHWC reference over the stored operands; table: a GroupNorm {scale, shift} table to use instead of the float64 one"""
    xs = _stored(x, prec).permute(0, 2, 3, 1).to(F64)
    kw = {}
    if gn is not None:
        N, H, W, C = xs.shape
        kw = dict(gn_scale_shift=table if table is not None else ref64.group_norm_scale_shift(xs.reshape(N, H * W, C), gn[0], gn[1], 32, 1e-5),
                  gn_silu=True)
    if skip is not None:
        kw.update(skip_x=_stored(skip[0], prec).permute(0, 2, 3, 1).to(F64), skip_w=_stored(skip[1], prec))
    wr = w if up else _stored(w, prec)  # (up4: the class kernels are summed in fp32 before they are rounded)
    return kw, ref64.conv_forward(xs, None, wr, ksize=3, upsample=1 if up else 0, bias=b, **kw)


def operands(tag, N, Cin, H, W, Cout):
    x = synth_input(f"tox{tag}", (N, Cin, H, W), 71, scale=1.2) + 0.15
    w = synth_input(f"tow{tag}", (Cout, Cin, 3, 3), 71, scale=1.0 / math.sqrt(9 * Cin))  # independent per tap
    b = synth_input(f"tob{tag}", (Cout,), 71, scale=0.1)
    return x, w, b


def plan_arm(prec, N, H, W, cin, cout, *, gn, skip=False, splitk=True):
    """which conv3x3_halo_kernel instance the launcher takes for a 128- or 256-column conv (csrc/igemm.hip: conv_splitk, conv_plan),
    stated here so that a case can say which arm it is about:
    - K slices (128-column KSPLIT instance): fewer than 256 workgroups at the nominal batch of 16 and at least four channel chunks;
    - else 64-column tiles on maps with fewer than 256 such workgroups;
    - else the 8-wave 256-column instance where Cout % 256 == 0, N * tiles * Cout / 256 >= 256 and the conv has a fused GroupNorm
      (or, split product, a fused skip conv); else the 4-wave 128-column instance."""
    tiles_pi, ct = (H // 8) * ((W + 15) // 16), -(-cout // 128)
    kc = -(-cin // (32 if prec == "fp32x3" else 64))
    ksplit = bool(splitk) and 16 * tiles_pi * ct < 256 and kc >= 4
    if ksplit:
        bn = 128
    elif 16 * tiles_pi * ct < 256:
        bn = 64
    elif cout % 256 == 0 and N * tiles_pi * (cout // 256) >= 256 and (gn or (prec == "fp32x3" and skip)):
        bn = 256
    else:
        bn = 128
    return dict(bn=bn, ksplit=ksplit)


def check(prec, x, w, b, *, expect=None, splitk=True, **kw):
    """run, compare with the float64 reference at the gate; expect: the arm (plan_arm) this case is about.  The K-slice arm is also
    observed: it is the one that needs a workspace."""
    N, cin, H, W = x.shape
    arm = plan_arm(prec, N, H, W, cin, w.shape[0], gn=kw.get("gn") is not None, skip=kw.get("skip") is not None, splitk=splitk)
    if expect is not None and not kw.get("up4"):
        assert {k: arm[k] for k in expect} == expect, (arm, expect)
    with Options(halo_splitk=int(splitk)):
        got, _, used = run_conv(prec, x, w, b, **kw)
    if not kw.get("up4"):
        assert used == arm["ksplit"], ("K slices", used, arm)
    _, ref = reference(prec, x, w, b, gn=kw.get("gn"), skip=kw.get("skip"), up=kw.get("up4", False))
    assert got.shape == ref.shape and torch.isfinite(got).all()
    err = rel_l2(got.to(F64), ref)
    print(f"rel-L2 {err:.3e}  {arm}")
    assert err < TOL[prec], err
    return got


@pytest.mark.parametrize("prec", ["fp32x3", "fp16"])
@pytest.mark.parametrize("gn", [False, True])
@pytest.mark.parametrize("cout", [128, 256])
@pytest.mark.parametrize("cin", [32, 96, 80])
def test_chunks_on_a_two_tile_row_map(prec, gn, cout, cin):
    """N = 2, 16 x 16: two tile rows (the row window crosses a tile row; every border row and column of a patch is zero padding); one
    chunk (prologue path only), three chunks (both patch buffers, chunk-boundary reads), a K tail (80); with and without the fused
    GroupNorm + SiLU.  (80 channels have no GroupNorm(32): that case runs without one.)  Maps this small run on the 64-column 4-wave
    instances (two MFMA column blocks per wave); the 128- and 256-column ones are the next test's."""
    x, w, b = operands((cin, cout), 2, cin, 16, 16, cout)
    check(prec, x, w, b, gn=_gamma_beta(cin, False) if gn and cin % 32 == 0 else None, expect=dict(bn=64, ksplit=False))


WIDE_CASES = [  # prec, N, Cin, Cout, fused GroupNorm, fused skip channels -> columns per workgroup
    # 64 x 32 maps (16 pixel tiles per image): the 4-wave 128-column instance; one chunk, three chunks, K tails (fp32 storage: 80 % 32,
    # fp16 storage: 32 / 96 / 80 % 64)
    *[(p, 4, c, 128, g, 0, 128) for p in ("fp32x3", "fp16") for c in (32, 96, 80) for g in ((False, True) if c % 32 == 0 else (False,))],
    # batch 16, 256 columns behind a fused GroupNorm: the 8-wave instance (early A reads); fp16 storage has its K tails at 32 and 96
    *[(p, 16, c, 256, True, 0, 256) for p in ("fp32x3", "fp16") for c in (32, 96)],
    # a K tail of fp32 storage excludes a GroupNorm(32): the split product reaches the 8-wave instance with a fused skip conv instead
    ("fp32x3", 16, 80, 256, False, 64, 256),
]


@pytest.mark.parametrize("case", WIDE_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_chunks_on_the_128_and_256_column_instances(case):
    prec, N, cin, cout, gn, sc, bn = case
    x, w, b = operands(case[1:], N, cin, 64, 32, cout)
    skip = None
    if sc:
        skip = (synth_input(f"toxk{case}", (N, sc, 64, 32), 71), synth_input(f"towk{case}", (cout, sc, 1, 1), 71, scale=1.0 / math.sqrt(9 * cin)))
    check(prec, x, w, b, gn=_gamma_beta(cin, False) if gn else None, skip=skip, expect=dict(bn=bn, ksplit=False))


def every_element(prec, x, w, b, gn, *, f64_table):
    """wide-gamma GroupNorm: EVERY output element against the float64 conv over the table the kernel itself used,
    |got - ref| <= ceil * sum |a| |w| (+ 2^-11 |ref|, the fp16 output rounding), ceil = (K + 4) 2^-24 for the fp32 accumulation of K
    terms + 2^-22 for the v_exp / v_rcp SiLU + 3 * 2^-22 for the split product (fp32x3) or + 2^-11 for the normalised operand rounded
    to fp16 (fp16 storage); and rel-L2 at the gate, against the float64 table (f64_table) or that same reference"""
    cin = x.shape[1]
    got, ss, _ = run_conv(prec, x, w, b, gn=gn)
    kw, ref_t = reference(prec, x, w, b, gn=gn, table=ss)
    err = rel_l2(got.to(F64), reference(prec, x, w, b, gn=gn)[1] if f64_table else ref_t)
    bound = ref64.conv_abs_bound(_stored(x, prec).permute(0, 2, 3, 1).to(F64), None, _stored(w, prec), ksize=3, bias=b, **kw)
    ceil = (9 * cin + 4) * 2.0 ** -24 + 2.0 ** -22 + (3 * 2.0 ** -22 if prec == "fp32x3" else 2.0 ** -11)
    slack = (got.to(F64) - ref_t).abs() - (2.0 ** -11 * ref_t.abs() if prec == "fp16" else 0.0)
    worst = float((slack / bound).max())
    print(f"rel-L2 {err:.3e}  worst element {worst:.3e} (ceiling {ceil:.3e})")
    assert torch.isfinite(got).all() and err < TOL[prec], err
    assert worst < ceil, (worst, ceil)


@pytest.mark.parametrize("prec", ["fp32x3", "fp16"])
@pytest.mark.parametrize("cout", [128, 256])
@pytest.mark.parametrize("cin", [32, 96])
def test_no_fragment_is_read_before_its_chunk_is_rewritten(prec, cout, cin):
    """8 x 16 map, GroupNorm scale / shift that differ by up to 10^6 between the chunks: a fragment read from the next chunk's patch
    buffer before that chunk's barrier (raw or half-rewritten rows) is a gross error (every_element).  One pixel tile per image: these
    cases run the 64-column instances, whose window rows are all read behind a step's barrier -- what they pin is that no row of the
    window outlives its chunk.  The instance that reads rows AHEAD of a barrier is the next test's."""
    x, w, b = operands(("st", cin, cout), 2, cin, 8, 16, cout)
    assert plan_arm(prec, 2, 8, 16, cin, cout, gn=True)["bn"] == 64
    every_element(prec, x, w, b, _gamma_beta(cin, True), f64_table=True)


@pytest.mark.parametrize("prec", ["fp32x3", "fp16"])
@pytest.mark.parametrize("cin", [32, 96])
def test_no_early_read_crosses_a_chunk_on_the_8_wave_instance(prec, cin):
    """the same wide-gamma, every-element comparison where A rows ARE read one step early: the 8-wave 256-column instance (batch 16,
    64 x 32 map, fused GroupNorm).  Its steps 1..8 take their new rows in front of the next barrier, step 0 of a chunk behind its own:
    an early read that reached into the next chunk's buffer would see rows another wave is still rewriting.  One chunk (fp32x3 at
    32 channels: no chunk boundary, the early reads alone) and three / two chunks with both patch buffers (96)."""
    x, w, b = operands(("st8", cin), 16, cin, 64, 32, 256)
    arm = plan_arm(prec, 16, 64, 32, cin, 256, gn=True)
    assert arm == dict(bn=256, ksplit=False), arm
    every_element(prec, x, w, b, _gamma_beta(cin, True), f64_table=False)


@pytest.mark.parametrize("prec", ["fp32x3", "fp16"])
@pytest.mark.parametrize("gn", [False, True])
def test_fused_skip_phase_behind_the_window(prec, gn):
    """3x3 (64 channels) + fused 1x1 skip conv over 96 channels at 16 x 16: the skip phase reuses the operand ring and its own fragments"""
    x, w, b = operands("sk", 2, 64, 16, 16, 128)
    xk = synth_input("toxk", (2, 96, 16, 16), 71)
    wk = synth_input("towk", (128, 96, 1, 1), 71, scale=4.0 / math.sqrt(9 * 64))
    check(prec, x, w, b, gn=_gamma_beta(64, False) if gn else None, skip=(xk, wk))


@pytest.mark.parametrize("prec", ["fp32x3", "fp16"])
def test_a_16x32_map_and_an_8_wide_map(prec):
    """a 16 x 32 map: two pixel tiles side by side per image, on 64-column tiles, with and without the fused GroupNorm; an 8-wide map:
    the right half of every tile masked"""
    x, w, b = operands("tpw2", 2, 96, 16, 32, 128)
    check(prec, x, w, b, gn=_gamma_beta(96, False), expect=dict(bn=64))
    check(prec, x, w, b, expect=dict(bn=64))
    x, w, b = operands("wide8", 2, 96, 16, 8, 128)
    check(prec, x, w, b, gn=_gamma_beta(96, False), expect=dict(bn=64))


@pytest.mark.parametrize("case", [(2, 96, 128, False, 128), (2, 96, 128, True, 128), (2, 32, 128, True, 128), (16, 96, 256, True, 256)],
                         ids=lambda c: "-".join(str(v) for v in c))
def test_split_product_on_the_128_and_256_column_instances_at_64x32(case):
    """split product without a skip conv on a 64 x 32 map (sixteen pixel tiles per image): the 4-wave 128-column instance with and without
    the fused GroupNorm, one chunk and three, and the 8-wave 256-column instance at batch 16"""
    N, cin, cout, gn, bn = case
    x, w, b = operands(("stream",) + case, N, cin, 64, 32, cout)
    check("fp32x3", x, w, b, gn=_gamma_beta(cin, False) if gn else None, expect=dict(bn=bn, ksplit=False))


@pytest.mark.parametrize("prec", ["fp32x3", "fp16"])
@pytest.mark.parametrize("cin", [128, 256])
def test_k_slices(prec, cin):
    """halo_splitk on a 16 x 16 map: 128 channels are four chunks of fp32 storage (K slices) but two of fp16 storage (unsplit: fewer
    than four chunks), 256 channels are K slices in both; the first step of every slice reads behind its barrier"""
    x, w, b = operands(("splitk", cin), 2, cin, 16, 16, 128)
    check(prec, x, w, b, gn=_gamma_beta(cin, False), expect=dict(ksplit=(prec, cin) != ("fp16", 128)))
    check(prec, x, w, b, gn=_gamma_beta(cin, False), splitk=False, expect=dict(bn=64, ksplit=False))


@pytest.mark.parametrize("prec", ["fp32x3", "fp16"])
@pytest.mark.parametrize("cin", [64, 96])
def test_parity_class_form(prec, cin):
    """conv_up4_halo_kernel, 8 x 16 stored -> 16 x 32, against the conv over the nearest-2x image"""
    x, w, b = operands(("u4", cin), 2, cin, 8, 16, 128)
    check(prec, x, w, b, up4=True)


@pytest.mark.parametrize("prec", ["fp32x3", "fp16"])
@pytest.mark.parametrize("up4", [False, True])
def test_runs_are_bit_equal_and_independent_of_the_batch(prec, up4):
    x, w, b = operands(("det", up4), 3, 96, 16, 16, 128)
    gn = None if up4 else _gamma_beta(96, False)
    a, _, _ = run_conv(prec, x, w, b, gn=gn, up4=up4)
    a2, _, _ = run_conv(prec, x, w, b, gn=gn, up4=up4)
    one, _, _ = run_conv(prec, x, w, b, gn=gn, up4=up4, n=1)
    assert torch.equal(a, a2), "two runs differ"
    assert torch.equal(a[0], one[0]), "image 0 of a batch of 3 differs from batch 1"
