"""GPU: the attention kernels, each called alone through the C ABI on fresh seeded tensors and compared ROW BY ROW with the float64
references of tests/ref64.py (themselves tested on the CPU in tests/test_ref64.py): eod_attention_fwd_nat (fp16, fp32x3 plain / with
pre-split input / pre-split output, exact fp32, wide heads), eod_attention_fwd (packed q|k + vT), eod_rowdot, eod_attention_bwd,
eod_softmax_rows / eod_softmax_bwd_rows, eod_scale_f32 and the GEMM forms of the materialised attention (through engine.Program.gemm, with
the softmax-rebuild and softmax-backward epilogues).  A ledger test maps every attention launch of real inference programs and trainers
to the test_edge_* table that reaches its kernel instance and flags.  Shapes are hand-picked from the kernels' loop structure: sequence lengths around the 128-query
workgroup and the 64-key tile (1, 63 / 64 / 65, 127 / 128 / 129: a workgroup or a RAGGED tile with one valid row), every head dim
instance with a partly filled last chunk or column tile, the channel-slice boundaries of the wide kernel, the dispatch edges of the
block-per-row softmax.

Conventions of tests/test_gpu_glue_ops.py: every output lies between two guard bands and is NaN-filled before the launch; every case
runs twice and the two runs must be bit-identical (the kernels claim: no atomics, fixed summation order); fp16 operands are rounded
first and the reference is built from the rounded values; pre-split inputs are built with ref64.presplit_encode and the reference sees
decode(encode(x)).

Gates.  A whole-tensor rel-L2 lets one query row, one head or the one row a ragged tile owns be off by 10 % at T in the hundreds.  Every
gate here is PER ROW -- a query row of `out` / `lse` / dQ, a key row of dK / dV, of one (image, head) -- as the L2 norm over the row's
head channels of the error against float64, divided by the L2 norm of an ALLOWANCE built per element from the reference's own
quantities (alpha = 1 / sqrt(d), u = 2^-24, S = alpha q k^T, P = softmax(S)):
    score error     ds = u_in alpha max_s sum_j |q_j| |k_sj|     u_in = (mfma steps + 2) u of the fp32 accumulation, + 2^-22 for split pairs
    exp / softmax   Ep = 2 ds + 2^-21 + 2^-22 log2(e) max_s |S| + (T / 2 + 2) u      (v_exp_f32, the fma in its argument, the row sum)
    out             sum_s P |v| (2 Ep + u_P + u_v + (T / 16 + 2) u) + u_out |out|    u_P = 2^-11 (fp16 P) / 2^-22 (split) / 2^-24,
                    u_out = 2^-11 / 2^-24, + T 2^-25 max|v| for fp16 P below the normal range, + 2^-22 |y| + 2^-25 / s written pre-split
    lse             Ep + 2^-22 |lse|
    dV              sum_t P (2^-11 + Ep') |dO| + T 2^-33 max|dO| + 2^-11 |dV|        Ep' = Ep + the error of the lse the kernel is given
    dS              E = |dS| (2^-11 + Ep') + P ((d / 16 + 4) u (sum_j |dO| |v| + |D|) + err(D)) + 2^-25 2^-k       (k = ds_log2)
    dK, dQ          alpha sum E |q|  /  alpha sum E |k|, + the accumulation term, + 2^-11 |result|
A ratio of 1 is the derived ceiling; each gate is min(1, about 4x the worst ratio measured on an MI355X) (value in the comment next to
it in GATE; every check prints `GATE name err`).  Copies (T = 1: out = v) and pad columns are gated on bits."""
import collections
import ctypes
import math

import pytest
import torch

from tests import ref64
from tests.test_gpu_conv_programs import bound_table
from tests.test_gpu_glue_ops import DEV, F16, F32, F64, NAN, Out, Rng, _bits, _dt, _L, _lib, _ok, _p, _same_bits, _st, twice

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
LOG2E = 1.4426950408889634

GATE = {
    # error / allowance per row (module docstring); ceiling 1.  Every value is min(1, about 4x the worst ratio measured on an MI355X); the
    # measured worst is in the comment above its line.
    # eod_attention_fwd_nat, d <= 64, fp16.  Measured worst: out 0.189 (T = 65, d = 8, image 1 = 37 x image 0), lse 0.159
    "fwd_f16_out": 0.76, "fwd_f16_lse": 0.64,
    # fp32x3 with and without a bound table: out 0.0095 (the allowance is dominated by the exp terms, which the split products do not
    # reach), lse 0.182 (T = 256, d = 8, image 1 = 37 x image 0: logits in the thousands)
    "fwd_x3_out": 0.038, "fwd_x3_lse": 0.73,
    # EOD_ATTN_IN_PRESPLIT: out 0.0073, lse 0.141
    "fwd_x3_in_out": 0.03, "fwd_x3_in_lse": 0.57,
    # EOD_ATTN_OUT_PRESPLIT: out 0.0091, lse 0.182
    "fwd_x3_out_out": 0.037, "fwd_x3_out_lse": 0.73,
    # both flags: out 0.0074, lse 0.141
    "fwd_x3_inout_out": 0.03, "fwd_x3_inout_lse": 0.57,
    # EOD_ATTN_EXACT_F32: out 0.0197, lse 0.143
    "fwd_f32_out": 0.08, "fwd_f32_lse": 0.58,
    # wide heads (csrc/attn_wide.hip): fp16 out 0.135, lse 0.092; fp32x3 out 0.0047, lse 0.081
    "wide_f16_out": 0.54, "wide_f16_lse": 0.37,
    "wide_x3_out": 0.019, "wide_x3_lse": 0.33,
    # eod_attention_fwd (packed q|k + vT): out 0.285 (T = 7, d = 12), lse 0.149
    "pack_out": 1.0, "pack_lse": 0.6,
    # eod_rowdot: |err| / ((d + 1) u sum |a| |b|).  fp16 0.401, fp32 0.406 (d = 8)
    "rowdot_f16": 1.0, "rowdot_f32": 1.0,
    # eod_attention_bwd: dQ 0.384, dK 0.416, dV 0.364 (all at T = 2, where a row is a sum of two fp16-rounded terms)
    "bwd_dq": 1.0, "bwd_dk": 1.0, "bwd_dv": 1.0,
    # the attention GEMM forms (plain, bias_mode 4, bias_mode 3), per row.  fp16: 0.768 (P . v from qkvT, d = 16: the fp16 output rounding
    # fills its 2^-11 |c| bound), mode 4 0.609, mode 3 0.664; fp32: 0.055, mode 4 0.099, mode 3 0.059
    "gemm_f16": 1.0, "gemm_f32": 0.22, "gemm_mode4_f16": 1.0, "gemm_mode4_f32": 0.4, "gemm_mode3_f16": 1.0, "gemm_mode3_f32": 0.24,
    # eod_softmax_rows / eod_softmax_bwd_rows, per row.  fp16: 0.722 / 0.734 (the output rounding); fp32: 0.059 / 0.099
    "softmax_f16": 1.0, "softmax_f32": 0.24, "softmax_bwd_f16": 1.0, "softmax_bwd_f32": 0.4,
}
WORST = collections.defaultdict(float)


def _gate(name, err, what):
    gate = min(GATE[name], 1.0)
    WORST[name] = max(WORST[name], err)
    print(f"GATE {name:20s} {err:.3e} (gate {gate:.3e}, worst so far {WORST[name]:.3e})  {what}")
    assert math.isfinite(err) and err < gate, (name, err, gate, what)


def _order(heads, d, new_order):
    """(q_off, k_off, v_off, head_stride): legacy [h][q|k|v][d], new [q|k|v][h][d]"""
    C = heads * d
    return (0, C, 2 * C, d) if new_order else (0, d, 2 * d, 3 * d)


def _heads(t, heads, d):
    """[N][T][C] -> [N][heads][T][d]"""
    N, T = t.shape[:2]
    return t.reshape(N, T, heads, d).permute(0, 2, 1, 3)


def _row_ratio(err, allow):
    return float((err.norm(dim=-1) / allow.norm(dim=-1).clamp_min(1e-300)).max())


# ================================================================================================ forward: reference and allowances
def fwd_terms(xref, heads, d, lay, cls, steps=None):
    """float64 reference of the forward and the per-element allowances of the module docstring.  cls: "f16" (fp16 operands and P),
    "x3" (split pairs), "f32" (IEEE fp32 products)"""
    N, T = xref.shape[:2]
    out, lse, P = ref64.attention_forward(xref, heads, d, *lay)
    q, k, v = (ref64.head_slices(xref, heads, d, o, lay[3]) for o in lay[:3])
    a = 1.0 / math.sqrt(d)
    S = a * (q @ k.transpose(-1, -2))
    Sabs = a * (q.abs() @ k.abs().transpose(-1, -2))
    if steps is None:
        steps = d / 2 if cls == "f32" else -(-d // 16)
    u_in = (steps + 2) * U + (2.0 ** -22 if cls == "x3" else 0.0)
    ds = u_in * Sabs.amax(-1)
    Ep = 2 * ds + 2.0 ** -21 + 2.0 ** -22 * LOG2E * S.abs().amax(-1) + (T / 2 + 2) * U                    # [N][heads][T]
    u_p = {"f16": 2.0 ** -11, "x3": 2.0 ** -22, "f32": U}[cls]
    u_v = {"f16": 0.0, "x3": 2.0 ** -22, "f32": U}[cls]
    acc = ((T / 2 if cls == "f32" else T / 16) + 2) * U
    oh = _heads(out, heads, d)
    allow = (P @ v.abs()) * (2 * Ep + u_p + u_v + acc)[..., None] + (2.0 ** -11 if cls == "f16" else U) * oh.abs()
    if cls == "f16":
        allow = allow + T * 2.0 ** -25 * v.abs().amax(2, keepdim=True)
    return dict(out=out, oh=oh, lse=lse, P=P, q=q, k=k, v=v, S=S, Sabs=Sabs, Ep=Ep, allow_out=allow, allow_lse=Ep + 2.0 ** -22 * lse.abs())


def fwd_check(name, tm, g_out, g_lse, heads, d, what, s_out=None):
    """g_out [N][T][C] float64 (decoded when it was written pre-split), g_lse [N][heads][T] or None"""
    assert bool(torch.isfinite(g_out).all()), "unwritten / non-finite output element: " + what
    allow = tm["allow_out"]
    if s_out is not None:
        allow = allow + 2.0 ** -22 * tm["oh"].abs() + 2.0 ** -25 / s_out.reshape(-1, 1, 1, 1)
    _gate(name + "_out", _row_ratio(_heads(g_out, heads, d) - tm["oh"], allow), what)
    if g_lse is not None:
        assert bool(torch.isfinite(g_lse).all()), "unwritten / non-finite lse: " + what
        _gate(name + "_lse", float(((g_lse.double() - tm["lse"]).abs() / tm["allow_lse"]).max()), what)


def assert_split_pairs(p, what):
    """a tensor written pre-split holds, per 8 channels, [8 x hi | 8 x lo] with hi = fp16(s y) and lo = fp16(s y - hi): |lo| is at most half
    a unit in the last place of hi.  (hi + lo alone cannot tell the two halves apart; the conv that reads them does: it drops lo x lo)"""
    h = p.contiguous().view(F16).reshape(p.shape[:-1] + (p.shape[-1] // 8, 16)).double()
    hi, lo = h[..., :8], h[..., 8:]
    assert bool((lo.abs() <= 2.0 ** -11 * hi.abs() + 2.0 ** -25).all()), "the hi / lo halves of a pre-split group are not a split pair: " + what


def _qkv(r, N, T, C, dtype, x37, scale=0.7):
    x = r.randn((N, T, 3 * C), scale)
    if x37:   # image 1 = 37 x image 0: a key mask that leaks into the next image, or a scale from the wrong table row, is loud
        assert N >= 2
        x[1] = 37.0 * x[0]
    return x.to(dtype)


# (T, d, N, heads, new_order, lse, image 1 = 37 x image 0): every T in {1, 33, 63, 64, 65, 128, 129, 191, 256} (one workgroup / one tile /
# one valid row in a ragged tile or in a second workgroup / two full workgroups), every d % 8 == 0 up to 64 (DS / DT = 1/1, 2/1, 3/2, 4/2,
# with d = 8, 24, 40, 56 a partly filled last chunk or column tile), N and heads in {1, 3}, both channel orders
NAT_CASES = [
    (1, 8, 1, 1, False, True, False), (1, 64, 3, 3, True, True, False), (1, 40, 1, 3, False, False, False),
    (33, 16, 1, 1, False, True, False), (33, 24, 3, 1, True, False, False),
    (63, 32, 1, 3, False, True, False), (63, 8, 3, 1, True, True, False),
    (64, 40, 1, 1, True, True, False), (64, 48, 3, 3, False, False, False),
    (65, 56, 1, 1, False, True, False), (65, 8, 3, 3, True, True, True), (65, 64, 1, 3, True, False, False),
    (128, 16, 1, 1, False, True, False), (128, 40, 3, 1, False, True, False),
    (129, 24, 1, 3, True, True, False), (129, 64, 3, 1, False, True, True), (129, 8, 1, 1, False, False, False),
    (191, 32, 1, 1, True, True, False), (191, 56, 3, 1, False, False, False),
    (256, 48, 1, 3, False, True, False), (256, 8, 3, 1, True, True, True), (256, 40, 1, 1, True, True, False),
]
NAT_KINDS = {  # kind -> (class of the allowance, bound table, input pre-split, output pre-split)
    "f16": ("f16", False, False, False), "x3": ("x3", False, False, False), "x3_tab": ("x3", True, False, False),
    "x3_in": ("x3", True, True, False), "x3_out": ("x3", True, False, True), "x3_inout": ("x3", True, True, True),
    "f32": ("f32", False, False, False),
}


def _fwd_nat_case(kind, gate, T, d, N, heads, new_order, want_lse, x37, seed):
    lib = _lib()
    cls, table, in_ps, out_ps = NAT_KINDS[kind]
    C, lay = heads * d, _order(heads, d, new_order)
    dtype = F16 if cls == "f16" else F32
    x = _qkv(Rng(seed), N, T, C, dtype, x37)
    tab = bound_table(x.double().abs().amax((1, 2)), seed) if table else None
    flags = (lib.ATTN_EXACT_F32 if cls == "f32" else 0) | (lib.ATTN_IN_PRESPLIT if in_ps else 0) | (lib.ATTN_OUT_PRESPLIT if out_ps else 0)
    xin, xref = x, x.double()
    if in_ps:   # the scale the kernel derives from the same table at the attention kernels' exponent range
        s_in = ref64.presplit_scale(tab, kmin=ref64.AB_KMIN_ATTN)
        xin = ref64.presplit_encode(x, s_in)
        xref = ref64.presplit_decode(xin, s_in)
    s_out = ref64.presplit_scale(tab) if out_ps else None   # what proj_out derives from the same table at the default exponent range
    out, lse = Out((N, T, C), dtype), (Out((N, heads, T)) if want_lse else None)
    got = twice(lambda: _ok(_L().eod_attention_fwd_nat(_p(xin), out.ptr, lse.ptr if lse else 0, _dt(dtype), N, T, C, heads, d, *lay, _p(tab), flags, _st()),
                            "attention_fwd_nat"), [out] + ([lse] if lse else []))
    what = f"{kind} T={T} d={d} N={N} heads={heads} new_order={new_order} lse={want_lse} x37={x37}"
    g_out = ref64.presplit_decode(got[0], s_out) if out_ps else got[0].double()
    if out_ps:
        assert_split_pairs(got[0], what)
    tm = fwd_terms(xref, heads, d, lay, cls)
    fwd_check(gate, tm, g_out, got[1] if want_lse else None, heads, d, what, s_out=s_out)
    if T == 1:   # one key: P = 1, out = v
        v = ref64.head_slices(xref, heads, d, lay[2], lay[3]).permute(0, 2, 1, 3).reshape(N, 1, C)
        if cls == "f16":   # v (1 + delta), |delta| <= 2^-23, rounds back to v
            assert _same_bits(got[0], v.to(F16)), "T = 1: out is not v bit for bit: " + what
        elif cls == "f32":   # the rounding of one multiply
            assert bool(((g_out - v).abs() <= 2.0 ** -23 * v.abs()).all()), "T = 1: out is not v: " + what
        else:   # v as a split pair at the operand scale (and once more at the output scale): 2^-22 |v| and half an fp16 subnormal step each
            s_op = ref64.presplit_scale(tab, kmin=ref64.AB_KMIN_ATTN) if table else torch.full((N,), 16.0, dtype=F64, device=DEV)
            tol = 2.0 ** -22 * v.abs() + 2.0 ** -25 / s_op.reshape(-1, 1, 1)
            if out_ps:
                tol = tol + 2.0 ** -22 * v.abs() + 2.0 ** -25 / s_out.reshape(-1, 1, 1)
            assert bool(((g_out - v).abs() <= tol).all()), "T = 1: out is not v: " + what


@pytest.mark.parametrize("kind", list(NAT_KINDS))
def test_edge_attention_fwd_nat(kind):
    """(a) eod_attention_fwd_nat, d <= 64: attn_fwd_nat_kernel (fp16), attn_fwd_nat_x3_kernel without a table (s = 16), with a table, with
    EOD_ATTN_IN_PRESPLIT (the LDS-DMA pipeline; T = 256 is the smallest the product emits, 65 and 129 are ragged), with
    EOD_ATTN_OUT_PRESPLIT (d = 8 and 40: the lane pairing on a partly filled column tile), with both; attn_fwd_nat_f32_kernel
    (EOD_ATTN_EXACT_F32: same 128-query / 64-key structure, csrc/attn_f32.hip)"""
    gate = "fwd_x3" if kind == "x3_tab" else "fwd_" + kind
    for i, case in enumerate(NAT_CASES):
        _fwd_nat_case(kind, gate, *case, seed=100 + i)


# (T, d, N, heads, new_order, lse): 32 queries per workgroup, 32-key tiles, the head dim split over 4 waves in slices of 32 nsl channels,
# nsl = ceil(ceil(d / 4) / 32): d = 128 | 136, 256 | 264, 384 | 392 are the slice boundaries, 72 and 200 leave waves without a channel
WIDE_CASES = [
    (1, 72, 1, 1, False, True), (1, 264, 1, 2, True, True), (1, 512, 1, 1, False, False),
    (31, 128, 1, 2, False, True), (31, 384, 1, 1, True, True), (31, 256, 1, 1, False, False),
    (32, 136, 1, 1, True, True), (32, 512, 1, 1, False, True), (32, 200, 1, 2, False, False), (32, 264, 1, 1, False, True),
    (33, 200, 1, 1, False, True), (33, 392, 1, 1, True, True), (33, 128, 1, 1, True, False), (33, 384, 1, 2, False, True),
    (65, 256, 1, 1, True, True), (65, 512, 1, 1, True, True), (65, 72, 3, 2, False, True), (65, 136, 1, 1, False, False), (65, 392, 1, 1, False, True),
]


@pytest.mark.parametrize("kind", ["f16", "x3", "x3_tab"])
def test_edge_attention_fwd_wide(kind):
    """(b) eod_attention_fwd_nat, 64 < d <= 512: attn_fwd_wide_kernel<half_t | float, nsl = 1 .. 4>"""
    cls, table = ("f16", False) if kind == "f16" else ("x3", kind == "x3_tab")
    dtype = F16 if cls == "f16" else F32
    for i, (T, d, N, heads, new_order, want_lse) in enumerate(WIDE_CASES):
        C, lay = heads * d, _order(heads, d, new_order)
        x = _qkv(Rng(200 + i), N, T, C, dtype, N >= 2)
        tab = bound_table(x.double().abs().amax((1, 2)), 200 + i) if table else None
        out, lse = Out((N, T, C), dtype), (Out((N, heads, T)) if want_lse else None)
        got = twice(lambda: _ok(_L().eod_attention_fwd_nat(_p(x), out.ptr, lse.ptr if lse else 0, _dt(dtype), N, T, C, heads, d, *lay, _p(tab), 0, _st()),
                                "attention_fwd_nat"), [out] + ([lse] if lse else []))
        what = f"wide {kind} T={T} d={d} N={N} heads={heads} new_order={new_order} lse={want_lse}"
        nsl = -(-(-(-d // 4)) // 32)
        tm = fwd_terms(x.double(), heads, d, lay, cls, steps=2 * nsl + 3)   # 2 nsl mfma steps per wave, then the four partials added
        fwd_check("wide_" + cls, tm, got[0].double(), got[1] if want_lse else None, heads, d, what)
        if T == 1:
            v = ref64.head_slices(x, heads, d, lay[2], lay[3]).permute(0, 2, 1, 3).reshape(N, 1, C)
            if cls == "f16":
                assert _same_bits(got[0], v.to(F16)), "T = 1: out is not v bit for bit: " + what
            else:
                s = ref64.presplit_scale(tab, kmin=ref64.AB_KMIN_ATTN) if table else torch.full((N,), 16.0, dtype=F64, device=DEV)
                assert bool(((got[0].double() - v).abs() <= 2.0 ** -22 * v.abs() + 2.0 ** -25 / s.reshape(-1, 1, 1)).all()), "T = 1: out is not v: " + what


# (T, d, N, heads, new_order, lse): the packed kernel behind OP_ATTN (fp16, d % 8 != 0): dpad = round_up(d, 8), ldt = round_up(T, 8)
PACK_CASES = [
    (1, 4, 1, 1, False, True), (1, 60, 3, 3, True, True), (7, 12, 1, 3, False, True), (7, 36, 3, 1, True, False), (7, 52, 1, 1, False, True),
    (63, 20, 1, 1, True, True), (63, 44, 3, 1, False, True), (64, 28, 1, 3, False, True), (64, 60, 1, 1, True, False), (64, 4, 3, 1, False, True),
    (65, 12, 1, 1, False, True), (65, 36, 1, 3, True, True), (65, 52, 3, 1, False, False), (129, 20, 1, 1, False, True), (129, 28, 3, 3, True, True),
    (129, 44, 1, 1, True, False), (129, 60, 1, 3, False, True), (129, 4, 1, 1, True, True),
]


def test_edge_attention_fwd_packed():
    """(c) eod_attention_fwd through eod_attn_desc.  The caller's contract, which the test keeps: the pad channels [d, dpad) of every
    head of qk are zero (zero rows of the packed projection weight) and the columns [T, ldt) of vT are zero (the buffer is zeroed when
    the program is built)"""
    lib = _lib()
    for i, (T, d, N, heads, new_order, want_lse) in enumerate(PACK_CASES):
        C, lay = heads * d, _order(heads, d, new_order)
        dpad, ldt = -(-d // 8) * 8, -(-T // 8) * 8
        x = _qkv(Rng(300 + i), N, T, C, F16, N >= 2)
        qk, vT = ref64.attention_pack(x, heads, d, dpad, ldt, new_order)
        out, lse = Out((N, T, C), F16), (Out((N, heads, T)) if want_lse else None)
        desc = lib.AttnDesc()
        desc.qk, desc.vT, desc.out, desc.lse = _p(qk), _p(vT), out.ptr, (lse.ptr if lse else 0)
        desc.ld_qk, desc.ldt = 2 * heads * dpad, ldt
        desc.dtype, desc.N, desc.T, desc.C, desc.heads, desc.d, desc.dpad, desc.k_off = lib.EOD_F16, N, T, C, heads, d, dpad, heads * dpad
        got = twice(lambda: _ok(_L().eod_attention_fwd(ctypes.byref(desc), _st()), "attention_fwd"), [out] + ([lse] if lse else []))
        what = f"packed T={T} d={d} dpad={dpad} ldt={ldt} N={N} heads={heads} new_order={new_order} lse={want_lse}"
        tm = fwd_terms(x.double(), heads, d, lay, "f16", steps=dpad // 16 + 1)
        fwd_check("pack", tm, got[0].double(), got[1] if want_lse else None, heads, d, what)
        if T == 1:
            v = ref64.head_slices(x, heads, d, lay[2], lay[3]).permute(0, 2, 1, 3).reshape(N, 1, C)
            assert _same_bits(got[0], v.to(F16)), "T = 1: out is not v bit for bit: " + what


# ================================================================================================ rowdot
@pytest.mark.parametrize("dtype", [F16, F32], ids=["f16", "f32"])
def test_edge_rowdot(dtype):
    """(d) eod_rowdot alone: D[n][h][t] = sum_j dO O over a head's channels, as the trainer calls it, and on the q slices of a
    legacy-order qkv tensor (three different strides).  |err| <= (d + 1) u sum_j |a_j b_j|: d products and additions in fp32"""
    name = "rowdot_f16" if dtype == F16 else "rowdot_f32"
    r = Rng(400)
    for N, T, heads, d in ((1, 1, 1, 8), (3, 65, 3, 24), (1, 129, 1, 40), (2, 33, 3, 56), (1, 300, 2, 64), (1, 2, 1, 512), (2, 4100, 2, 8)):
        C = heads * d
        a, b = r.randn((N, T, C), 0.5, dtype), r.randn((N, T, C), 0.7, dtype)
        D = Out((N, heads, T))
        got, = twice(lambda: _ok(_L().eod_rowdot(_p(a), _p(b), _dt(dtype), N, heads, T, T * C, d, C, d, D.ptr, _st()), "rowdot"), [D])
        ref = ref64.rowdot(a, b, N, heads, T, T * C, d, C, d)
        den = ref64.rowdot(a.abs(), b.abs(), N, heads, T, T * C, d, C, d)
        assert bool(torch.isfinite(got).all())
        _gate(name, float(((got.double() - ref).abs() / ((d + 1) * U * den).clamp_min(1e-300)).max()), f"N={N} T={T} heads={heads} d={d}")
        x = r.randn((N, T, 3 * C), 0.7, dtype)
        D = Out((N, heads, T))
        got, = twice(lambda: _ok(_L().eod_rowdot(_p(x), _p(x), _dt(dtype), N, heads, T, T * 3 * C, 3 * d, 3 * C, d, D.ptr, _st()), "rowdot"), [D])
        ref = ref64.head_slices(x, heads, d, 0, 3 * d).square().sum(-1)
        _gate(name, float(((got.double() - ref).abs() / ((d + 1) * U * ref).clamp_min(1e-300)).max()), f"q . q, N={N} T={T} heads={heads} d={d}")


# ================================================================================================ backward
def bwd_check(x, dO, heads, d, lay, g_dqkv, what, *, lse_err=None, D_err=None):
    """x, dO fp16 (the kernel's inputs), g_dqkv fp16 [N][T][3C].  lse_err / D_err [N][heads][T]: bounds on the error of the lse / D the
    kernel was given (None: the float64 values rounded to fp32)"""
    N, T = x.shape[:2]
    tm = fwd_terms(x.double(), heads, d, lay, "f16")
    P, q, k, v = tm["P"], tm["q"], tm["k"], tm["v"]
    ref, D = ref64.attention_backward(x.double(), dO.double(), heads, d, *lay)
    g = _heads(dO.double(), heads, d)
    dP = g @ v.transpose(-1, -2)
    dS = P * (dP - D[..., None])
    klog = min(12, int(math.floor(math.log2(T))))
    cond = float(dS.abs().max()) * 2.0 ** klog
    assert cond < 2.0 ** 15, ("the case itself overflows fp16: 2^k P |dP - D|", cond, what)   # a failure below is never an fp16 overflow of the inputs
    if lse_err is None:
        lse_err = U * tm["lse"].abs()
    if D_err is None:
        D_err = U * D.abs()
    Ep = (tm["Ep"] + lse_err)[..., None]                                                               # [N][heads][T][1]
    acc = (T / 16 + 2) * U
    a = 1.0 / math.sqrt(d)
    E = dS.abs() * (2.0 ** -11 + Ep) + P * ((d / 16 + 4) * U * (g.abs() @ v.abs().transpose(-1, -2) + D.abs()[..., None]) + D_err[..., None]) \
        + 2.0 ** -25 * 2.0 ** -klog
    rq, rk, rv = (ref64.head_slices(ref, heads, d, o, lay[3]) for o in lay[:3])
    allow_v = (P * (2.0 ** -11 + Ep + acc)).transpose(-1, -2) @ g.abs() + T * 2.0 ** -33 * g.abs().amax(2, keepdim=True) + 2.0 ** -11 * rv.abs()
    allow_k = a * ((E + acc * dS.abs()).transpose(-1, -2) @ q.abs()) + 2.0 ** -11 * rk.abs()
    allow_q = a * ((E + acc * dS.abs()) @ k.abs()) + 2.0 ** -11 * rq.abs()
    assert bool(torch.isfinite(g_dqkv).all()), "an element of dqkv was not written, or is not finite: " + what
    gq, gk, gv = (ref64.head_slices(g_dqkv, heads, d, o, lay[3]) for o in lay[:3])
    _gate("bwd_dv", _row_ratio(gv - rv, allow_v), what)
    _gate("bwd_dk", _row_ratio(gk - rk, allow_k), what)
    _gate("bwd_dq", _row_ratio(gq - rq, allow_q), what)
    return cond


def _bwd_alone(T, d, N, heads, new_order, seed, *, dO_scale=0.5, neg_logits=False):
    """eod_attention_bwd with lse and D from the float64 reference, rounded to fp32: a forward error cannot hide in it"""
    C, lay = heads * d, _order(heads, d, new_order)
    r = Rng(seed)
    x = r.randn((N, T, 3 * C), 0.7)
    if neg_logits:   # every logit around -35 (tests/test_gpu_kernels.py::test_flash_attention_backward_vs_autograd): lse << 0
        off = math.sqrt(35.0 / math.sqrt(d))
        for h in range(heads):
            x[..., lay[0] + h * lay[3]: lay[0] + h * lay[3] + d] = 0.3 * x[..., lay[0] + h * lay[3]: lay[0] + h * lay[3] + d] + off
            x[..., lay[1] + h * lay[3]: lay[1] + h * lay[3] + d] = 0.3 * x[..., lay[1] + h * lay[3]: lay[1] + h * lay[3] + d] - off
    x = x.to(F16)
    dO = r.randn((N, T, C), dO_scale, F16)
    _, lse, _ = ref64.attention_forward(x.double(), heads, d, *lay)
    _, D = ref64.attention_backward(x.double(), dO.double(), heads, d, *lay)
    lse32, D32 = lse.float().contiguous(), D.float().contiguous()
    dqkv = Out((N, T, 3 * C), F16)
    got, = twice(lambda: _ok(_L().eod_attention_bwd(_p(x), _p(dO), _p(lse32), _p(D32), dqkv.ptr, _lib().EOD_F16, N, T, C, heads, d, *lay, _st()),
                             "attention_bwd"), [dqkv])
    what = f"bwd T={T} d={d} N={N} heads={heads} new_order={new_order} dO_scale={dO_scale} neg_logits={neg_logits}"
    cond = bwd_check(x, dO, heads, d, lay, got, what)
    print(f"COND 2^k P |dP - D| = {cond:.3g}  {what}")
    return cond


# (T, d, N, heads, new_order): T in {1, 2, 33, 63, 64, 65, 127, 128, 129, 193} (T = 2: ds_log2 = 1; a key / query workgroup or a ragged
# tile with one valid row), d in {8, 24, 40, 56, 64} (DS / DT = 1/1, 2/1, 3/2, 4/2 with a partly filled last chunk or column tile)
BWD_CASES = [
    (1, 8, 1, 1, False), (1, 64, 3, 3, True), (2, 24, 1, 1, False), (2, 40, 3, 1, True), (33, 56, 1, 3, False), (33, 8, 1, 1, True),
    (63, 24, 1, 1, False), (63, 64, 3, 1, True), (64, 40, 1, 1, False), (64, 56, 1, 3, True), (65, 8, 3, 3, False), (65, 24, 1, 1, True),
    (65, 64, 1, 1, False), (127, 40, 1, 1, False), (127, 56, 3, 1, True), (128, 24, 1, 3, False), (128, 64, 1, 1, True), (129, 40, 3, 1, False),
    (129, 56, 1, 1, True), (129, 8, 1, 3, False), (193, 24, 1, 1, True), (193, 64, 1, 3, False), (193, 40, 3, 1, True),
]


def test_edge_attention_bwd_alone():
    """(d) attn_bwd_kv_kernel / attn_bwd_q_kernel at their tile edges"""
    for i, case in enumerate(BWD_CASES):
        _bwd_alone(*case, seed=500 + i)


def test_edge_attention_bwd_short_sequence_with_a_large_gradient():
    """dS is carried on 2^min(12, floor(log2 T)): at T = 2 and 3 (ds_log2 = 1) an output gradient of magnitude 128 stays far inside fp16
    (the condition is asserted with the kernel's own exponent), while a fixed 2^12 would overflow"""
    for i, (T, d) in enumerate(((2, 8), (3, 24), (2, 64))):
        cond = _bwd_alone(T, d, 1, 1, False, seed=540 + i, dO_scale=128.0)
        assert cond * 2.0 ** 11 > 65504.0, "the case would not overflow on a 2^12 scale: it does not distinguish the exponents"


def test_edge_attention_bwd_long_sequence():
    """T = 4096: ds_log2 = 12, 64 key tiles, 32 workgroups"""
    _bwd_alone(4096, 8, 1, 1, False, seed=550)


@pytest.mark.parametrize("T", [65, 129])
def test_edge_attention_bwd_negative_logits_on_a_ragged_tile(T):
    """every logit around -35: exp(-lse) is huge, and a zero-filled key row of the ragged tile that holds ONE valid key has dS = -exp(-lse) 2^k D,
    inf in fp16 and NaN against the zero K row unless the tile masks the keys beyond T"""
    for i, (d, N, heads, new_order) in enumerate(((16, 1, 1, False), (40, 2, 3, True), (64, 1, 1, False))):
        _bwd_alone(T, d, N, heads, new_order, seed=560 + T + i, neg_logits=True)


def test_edge_attention_fwd_rowdot_bwd_chained():
    """forward (with lse) -> rowdot -> backward, as UNetTrainer chains them: D now comes from the fp16-rounded `out`
    (err(D) <= 2^-11 sum_j |dO| |out| + the rowdot's own) and lse from the kernel (its allowance)"""
    lib = _lib()
    for i, (T, d, N, heads, new_order) in enumerate(((129, 40, 3, 1, False), (65, 24, 1, 3, True))):
        C, lay = heads * d, _order(heads, d, new_order)
        r = Rng(570 + i)
        x, dO = r.randn((N, T, 3 * C), 0.7, F16), r.randn((N, T, C), 0.5, F16)
        out, lse, D, dqkv = Out((N, T, C), F16), Out((N, heads, T)), Out((N, heads, T)), Out((N, T, 3 * C), F16)

        def launch():
            L, st = _L(), _st()
            _ok(L.eod_attention_fwd_nat(_p(x), out.ptr, lse.ptr, lib.EOD_F16, N, T, C, heads, d, *lay, 0, 0, st), "attention_fwd_nat")
            _ok(L.eod_rowdot(_p(dO), out.ptr, lib.EOD_F16, N, heads, T, T * C, d, C, d, D.ptr, st), "rowdot")
            _ok(L.eod_attention_bwd(_p(x), _p(dO), lse.ptr, D.ptr, dqkv.ptr, lib.EOD_F16, N, T, C, heads, d, *lay, st), "attention_bwd")
        g_out, g_lse, g_D, g_dqkv = twice(launch, [out, lse, D, dqkv])
        what = f"chained T={T} d={d} N={N} heads={heads} new_order={new_order}"
        tm = fwd_terms(x.double(), heads, d, lay, "f16")
        fwd_check("fwd_f16", tm, g_out.double(), g_lse, heads, d, what)
        den = (_heads(dO.double(), heads, d).abs() * tm["oh"].abs()).sum(-1)
        _, Dref = ref64.attention_backward(x.double(), dO.double(), heads, d, *lay)
        D_err = (2.0 ** -11 + (d + 1) * U) * den + (_heads(dO.double(), heads, d).abs() * tm["allow_out"]).sum(-1)
        assert bool(((g_D.double() - Dref).abs() <= D_err).all()), "D of the chain: " + what
        bwd_check(x, dO, heads, d, lay, g_dqkv, what, lse_err=tm["allow_lse"], D_err=D_err)


# ================================================================================================ softmax rows
# (n, lds, ldp): the wave-per-row kernel (n < 1024, ldp > 16384, a pitch that is no multiple of 4) and softmax_row_block_kernel<V4> with
# need = ceil(ldp / 1024) = 1, 2, 3 (V4 = 4 with a wholly skipped register block), 5 (V4 = 8), 9 and 16 (V4 = 16); lds != ldp
SOFTMAX_CASES = [(1, 4, 4), (63, 64, 64), (65, 72, 72), (1023, 1024, 1024), (1024, 1024, 1024), (1025, 1028, 1028), (1030, 1036, 1032),
                 (2049, 2052, 2052), (4097, 4100, 4100), (8193, 8196, 8196), (16384, 16384, 16384), (16385, 16388, 16388), (1100, 1102, 1102)]


@pytest.mark.parametrize("dtype", [F16, F32], ids=["f16", "f32"])
def test_edge_softmax_rows_forward_and_backward(dtype):
    """(e) 5 rows (two blocks of the wave-per-row kernel, the second partly filled).  Input columns [n, lds) are NaN, output columns
    [n, ldp) must be exactly 0.  Row 1 is peaked (logits +-50).
    P: allowance P (2^-22 + 2^-23 max|s - m| + (n / 64 + 10) u) (+ 2^-11 P + 2^-25 in fp16; + 2^-126: a flushed subnormal).
    dS = P (dP - sum dP P) from the P handed in: |dS| 4 u + P (n / 64 + 10) u sum|dP P| (+ 2^-11 |dS| + 2^-25 in fp16)"""
    rows = 5
    tag = "f16" if dtype == F16 else "f32"
    for i, (n, lds, ldp) in enumerate(SOFTMAX_CASES):
        r = Rng(600 + i)
        s = r.randn((rows, lds), 3.0)
        s[1] = torch.where(r.randint(2, (lds,)) == 0, -50.0, 50.0) + r.randn((lds,))
        s[:, n:] = NAN
        P = Out((rows, ldp), dtype)
        got, = twice(lambda: _ok(_L().eod_softmax_rows(_p(s), lds, P.ptr, ldp, _dt(dtype), rows, n, _st()), "softmax_rows"), [P])
        what = f"{tag} n={n} lds={lds} ldp={ldp}"
        ref = ref64.softmax_rows(s, n)
        z = s[:, :n].double()
        spread = (z.amax(1, keepdim=True) - z).amax(1, keepdim=True)
        allow = ref * (2.0 ** -22 + 2.0 ** -23 * spread + (n / 64 + 10) * U) + 2.0 ** -126
        if dtype == F16:
            allow = allow + 2.0 ** -11 * ref + 2.0 ** -25
        assert bool(torch.isfinite(got[:, :n]).all()), "unwritten / non-finite output element: " + what
        assert not bool(_bits(got[:, n:]).any()), "pad columns [n, ldp) are not +0: " + what
        _gate("softmax_" + tag, _row_ratio(got[:, :n].double() - ref, allow), what)
        # backward, from the reference's P rounded to the storage type; NaN behind n in both inputs
        Pin = torch.full((rows, ldp), NAN, dtype=dtype, device=DEV)
        Pin[:, :n] = ref.to(dtype)
        dP = r.randn((rows, lds))
        dP[:, n:] = NAN
        dS = Out((rows, ldp), dtype)
        gds, = twice(lambda: _ok(_L().eod_softmax_bwd_rows(_p(Pin), ldp, _p(dP), lds, dS.ptr, _dt(dtype), rows, n, _st()), "softmax_bwd_rows"), [dS])
        rds = ref64.softmax_backward_rows(Pin, dP, n)
        pd, gd = Pin[:, :n].double(), dP[:, :n].double()
        allow = rds.abs() * 4 * U + pd * (n / 64 + 10) * U * (gd * pd).abs().sum(1, keepdim=True) + 2.0 ** -126
        if dtype == F16:
            allow = allow + 2.0 ** -11 * rds.abs() + 2.0 ** -25
        assert bool(torch.isfinite(gds[:, :n]).all()), "unwritten / non-finite dS element: " + what
        assert not bool(_bits(gds[:, n:]).any()), "pad columns [n, ldp) of dS are not +0: " + what
        _gate("softmax_bwd_" + tag, _row_ratio(gds[:, :n].double() - rds, allow), what)


# ================================================================================================ the attention GEMM forms
def _gemm_rows(name, got, ref, allow, what):
    """per row m of every batch: || got - ref || / || allow || over the N columns"""
    assert bool(torch.isfinite(got).all()), "unwritten / non-finite element: " + what
    _gate(name, _row_ratio(got.double() - ref, allow), what)


def _run_gemm(prec, outs, build, prefill=None):
    """one engine.Program holding the GEMM (and nothing else), run twice on NaN-filled outputs"""
    from eo_diffusion_amd.engine import Program
    prog = Program(DEV, prec)
    build(prog)
    assert [int(op.kind) for op in prog.ops] == [_lib().OP_GEMM]
    return twice(lambda: prog.run(), outs, prefill)


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
@pytest.mark.parametrize("T,d,new_order", [(72, 16, False), (72, 24, True), (77, 16, True), (77, 24, False)])
def test_edge_attention_gemm_forms(prec, T, d, new_order):
    """(f) the GEMM calls of the materialised attention, through engine.Program.gemm with the strides and offsets of their call sites:
    inference (AttentionBlock._emit: scores from the packed q|k with b_off = Cq into fp32, P . vT) and trainer (UNetTrainer: scores on the
    natural layout with a_off / b_off and the head stride in sa / sb, P . v from qkvT, the bias_mode 4 rebuild of P = exp(alpha q.k - lse),
    eod_scale_f32 + the bias_mode 3 epilogue dS = P (alpha' dP - D') at ds_scale 4096 and 1, dQ with c_off).  N = 2, 3 heads, T = 77 is
    padded to Tp = 80; the K pad columns of P / dS and of vT / qkvT are zero (the caller's contract), the N pad columns of every output
    must stay untouched (NaN).
    Allowances per element: alpha sum_k |a| |b| ((K / 16 + 2) u in fp16, (K + 2) u in fp32) + u_out |c|, + the exp terms of the module
    docstring for mode 4, + 2 u (|alpha' dP| + |D'|) P for mode 3, + 2^-25 for an fp16 result below the normal range"""
    lib = _lib()
    f16 = prec == "fp16"
    tdt, tag = (F16, "f16") if f16 else (F32, "f32")
    epc, u_out = (8, 2.0 ** -11) if f16 else (4, U)
    N, nh = 2, 3
    Cc, lay = nh * d, _order(nh, d, new_order)
    qo, ko, vo, hs = lay
    Tp = -(-T // epc) * epc
    alpha = 1.0 / math.sqrt(d)
    uk = (lambda K: (K / 16 + 2) * U) if f16 else (lambda K: (K + 2) * U)
    sub = 2.0 ** -25 if f16 else 0.0
    r = Rng(800 + T + d)
    x = r.randn((N, T, 3 * Cc), 0.7, tdt)
    dO = r.randn((N, T, Cc), 0.5, tdt)
    x64 = x.double()
    out_ref, lse_ref, P_ref = ref64.attention_forward(x64, nh, d, *lay)
    q, k, v = (ref64.head_slices(x64, nh, d, o, hs) for o in lay[:3])
    S_ref = alpha * (q @ k.transpose(-1, -2))                        # [N][nh][T][T]
    S_abs = alpha * (q.abs() @ k.abs().transpose(-1, -2))
    what = f"{prec} T={T} Tp={Tp} d={d} new_order={new_order}"
    bs = dict(nb0=N, nb1=nh)

    # ---- inference: scores from the packed q|k (b_off = Cq), fp32 output
    dpad = -(-d // epc) * epc
    Cq = nh * dpad
    qk, vT = ref64.attention_pack(x, nh, d, dpad, Tp, new_order)
    S = Out((N * nh, T, Tp), F32)
    got, = _run_gemm(prec, [S], lambda p: p.gemm(qk, qk, S.t, T, T, dpad, 2 * Cq, 2 * Cq, Tp, alpha=alpha, c_f32=True, sa=(T * 2 * Cq, dpad),
                                                 sb=(T * 2 * Cq, dpad), sc=(nh * T * Tp, T * Tp), b_off=Cq, **bs))
    got = got.reshape(N, nh, T, Tp)
    assert bool(torch.isnan(got[..., T:]).all()), "columns [T, Tp) of the scores were written: " + what
    _gemm_rows("gemm_" + tag, got[..., :T], S_ref, uk(dpad) * S_abs + U * S_ref.abs(), "scores, packed: " + what)

    # ---- trainer: scores on the natural layout (a_off / b_off, the head stride in sa / sb)
    S = Out((N * nh, T, Tp), F32)
    got, = _run_gemm(prec, [S], lambda p: p.gemm(x, x, S.t, T, T, d, 3 * Cc, 3 * Cc, Tp, alpha=alpha, c_f32=True, sa=(T * 3 * Cc, hs), sb=(T * 3 * Cc, hs),
                                                 sc=(nh * T * Tp, T * Tp), a_off=qo, b_off=ko, **bs))
    got = got.reshape(N, nh, T, Tp)
    assert bool(torch.isnan(got[..., T:]).all()), "columns [T, Tp) of the scores were written: " + what
    _gemm_rows("gemm_" + tag, got[..., :T], S_ref, uk(d) * S_abs + U * S_ref.abs(), "scores, natural: " + what)

    # ---- P . vT (inference) and P . v from qkvT (trainer): P = the reference's, rounded to the storage type, zero pad columns
    P = torch.zeros((N * nh, T, Tp), dtype=tdt, device=DEV)
    P.view(N, nh, T, Tp)[..., :T] = P_ref.to(tdt)
    P64 = P.view(N, nh, T, Tp)[..., :T].double()
    a_ref = P64 @ v                                                   # [N][nh][T][d]
    a_allow = uk(Tp) * (P64 @ v.abs()) + u_out * a_ref.abs() + sub
    a = Out((N * T, Cc), tdt)
    got, = _run_gemm(prec, [a], lambda p: p.gemm(P, vT, a.t, T, d, Tp, Tp, Tp, Cc, sa=(nh * T * Tp, T * Tp), sb=(Cc * Tp, d * Tp), sc=(T * Cc, d), **bs))
    _gemm_rows("gemm_" + tag, _heads(got.reshape(N, T, Cc), nh, d), a_ref, a_allow, "P . vT: " + what)
    BK = 128 // (2 if f16 else 4)
    ldT = -(-(N * Tp) // BK) * BK
    qkvT = torch.zeros((3 * Cc, ldT), dtype=tdt, device=DEV)         # [3C][n * Tp + t], zero elsewhere
    qkvT[:, :N * Tp].view(3 * Cc, N, Tp)[..., :T] = x.permute(2, 0, 1)
    a = Out((N * T, Cc), tdt)
    got, = _run_gemm(prec, [a], lambda p: p.gemm(P, qkvT, a.t, T, d, Tp, Tp, ldT, Cc, sa=(nh * T * Tp, T * Tp), sb=(Tp, hs * ldT), sc=(T * Cc, d),
                                                 b_off=vo * ldT, **bs))
    _gemm_rows("gemm_" + tag, _heads(got.reshape(N, T, Cc), nh, d), a_ref, a_allow, "P . v from qkvT: " + what)

    # ---- bias_mode 4: P = exp(alpha q.k - lse) from the natural layout and the fp32 log-sum-exp
    lse32 = lse_ref.float().contiguous()
    Pm = Out((N * nh, T, Tp), tdt)
    got, = _run_gemm(prec, [Pm], lambda p: p.gemm(x, x, Pm.t, T, T, d, 3 * Cc, 3 * Cc, Tp, alpha=alpha, bias=lse32, bias_mode=4, sa=(T * 3 * Cc, hs),
                                                  sb=(T * 3 * Cc, hs), sc=(nh * T * Tp, T * Tp), a_off=qo, b_off=ko, **bs))
    got = got.reshape(N, nh, T, Tp)
    assert bool(torch.isnan(got[..., T:]).all()), "columns [T, Tp) of P were written: " + what
    Ep = uk(d) * S_abs + 2.0 ** -22 + 2.0 ** -23 * LOG2E * (S_ref.abs() + 2 * lse_ref.abs()[..., None])
    _gemm_rows("gemm_mode4_" + tag, got[..., :T], P_ref, P_ref * (Ep + u_out) + sub, "mode 4: " + what)

    # ---- eod_scale_f32 + bias_mode 3: dS = P (ds_scale dP - ds_scale D), only where Tp == T (otherwise the trainer runs the row kernel)
    g = _heads(dO.double(), nh, d)
    dP_ref = g @ v.transpose(-1, -2)
    dP_abs = g.abs() @ v.abs().transpose(-1, -2)
    D_ref = (dP_ref * P64).sum(-1)
    if Tp == T:
        for ds_scale in (4096.0, 1.0):
            D32 = D_ref.float().contiguous()
            Dd = D32.double()
            dS = Out((N * nh, T, Tp), tdt)

            def build(p):
                p.gemm(dO, x, dS.t, T, T, d, Cc, 3 * Cc, Tp, alpha=ds_scale, bias=D32, bias_mode=3, res=P, sa=(T * Cc, d), sb=(T * 3 * Cc, hs),
                       sc=(nh * T * Tp, T * Tp), b_off=vo, **bs)

            def prefill():   # D is scaled in place before every run, as the trainer's backward does after its rowdot
                D32.copy_(D_ref.float())
                if ds_scale != 1.0:
                    _ok(_L().eod_scale_f32(_p(D32), D32.numel(), ds_scale, _st()), "scale_f32")
            got, = _run_gemm(prec, [dS], build, prefill)
            ref = ds_scale * P64 * (dP_ref - Dd[..., None])
            assert float(ref.abs().max()) < 2.0 ** 15, "the case itself overflows fp16"
            allow = ds_scale * P64 * (uk(d) * dP_abs + 2 * U * (dP_ref.abs() + Dd.abs()[..., None])) + u_out * ref.abs() + sub
            _gemm_rows("gemm_mode3_" + tag, got.reshape(N, nh, T, Tp), ref, allow, f"mode 3, ds_scale {ds_scale}: " + what)

    # ---- dQ = alpha dS k with c_off: dS = the reference's (on the 2^12 scale in fp16), rounded, zero pad columns; k^T rows from qkvT
    ds_scale = 4096.0 if f16 else 1.0
    dS_t = torch.zeros((N * nh, T, Tp), dtype=tdt, device=DEV)
    dS_t.view(N, nh, T, Tp)[..., :T] = (ds_scale * P64 * (dP_ref - D_ref[..., None])).to(tdt)
    dS64 = dS_t.view(N, nh, T, Tp)[..., :T].double()
    dqkv = Out((N, T, 3 * Cc), tdt)
    got, = _run_gemm(prec, [dqkv], lambda p: p.gemm(dS_t, qkvT, dqkv.t, T, d, Tp, Tp, ldT, 3 * Cc, alpha=alpha / ds_scale, sa=(nh * T * Tp, T * Tp),
                                                    sb=(Tp, hs * ldT), sc=(T * 3 * Cc, hs), b_off=ko * ldT, c_off=qo, **bs))
    ref = (alpha / ds_scale) * (dS64 @ k)
    allow = (alpha / ds_scale) * uk(Tp) * (dS64.abs() @ k.abs()) + u_out * ref.abs() + sub
    _gemm_rows("gemm_" + tag, ref64.head_slices(got, nh, d, qo, hs), ref, allow, "dQ with c_off: " + what)
    for o in (ko, vo):   # only the q slices are written
        assert bool(torch.isnan(ref64.head_slices(got, nh, d, o, hs)).all()), "dQ wrote outside the q slices: " + what


def test_edge_scale_f32():
    """eod_scale_f32 (x *= s in place, fp32): one IEEE multiply per element, so bit equality with torch; a second trip of the
    grid-stride loop (more than 4096 * 256 elements)"""
    r = Rng(700)
    for n in (1, 255, 257, 4096 * 256 + 3):
        for s in (4096.0, 0.37):
            x0 = r.randn((n,))
            x = Out((n,))
            got, = twice(lambda: _ok(_L().eod_scale_f32(x.ptr, n, s, _st()), "scale_f32"), [x], prefill=lambda: x.t.copy_(x0))
            assert _same_bits(got, x0 * torch.tensor(s, dtype=F32, device=DEV)), (n, s)


# ================================================================================================ coverage ledger
def _inst(d):
    """(DS, DT) of the d <= 64 kernels"""
    return (-(-d // 16), -(-d // 32))


def _nat_key(lib, dt, d, flags, table):
    """kernel instance and flags of one eod_attention_fwd_nat launch -> (test, kind)"""
    if d > 64:
        kind = "f16" if dt == lib.EOD_F16 else ("x3_tab" if table else "x3")
        return "test_edge_attention_fwd_wide", kind, -(-(-(-d // 4)) // 32)
    if dt == lib.EOD_F16:
        kind = "f16"
    elif flags & lib.ATTN_EXACT_F32:
        kind = "f32"
    else:
        ps = (bool(flags & lib.ATTN_IN_PRESPLIT), bool(flags & lib.ATTN_OUT_PRESPLIT))
        kind = {(False, False): "x3_tab" if table else "x3", (True, False): "x3_in", (False, True): "x3_out", (True, True): "x3_inout"}[ps]
        assert table or ps == (False, False), "a pre-split launch without a bound table"
    return "test_edge_attention_fwd_nat", kind, _inst(d)


def _softmax_route(n, lds, ldp):
    """the kernel eod_softmax_rows / eod_softmax_bwd_rows dispatch to (csrc/norm.hip, csrc/train.hip; pointers are 16-byte aligned)"""
    if lds % 4 or ldp % 4 or ldp > 16384 or n < 1024:
        return "wave"
    need = -(-ldp // 1024)
    return "block%d" % next(v for v in (1, 2, 4, 8, 16) if need <= v)


def _pinned():
    """what the tables of this module reach: test -> set of (kind, instance)"""
    return {
        "test_edge_attention_fwd_nat": {(kind, _inst(c[1])) for kind in NAT_KINDS for c in NAT_CASES},
        "test_edge_attention_fwd_wide": {(kind, -(-(-(-c[1] // 4)) // 32)) for kind in ("f16", "x3", "x3_tab") for c in WIDE_CASES},
        "test_edge_attention_fwd_packed": {("f16", (-(-(-(-c[1] // 8) * 8) // 16), -(-c[1] // 32))) for c in PACK_CASES},
        "test_edge_softmax_rows_forward_and_backward": {(tag, _softmax_route(*c)) for tag in ("f16", "f32") for c in SOFTMAX_CASES},
        "test_edge_attention_bwd_alone": {("f16", _inst(c[1])) for c in BWD_CASES},
        "test_edge_rowdot": {("f16", None), ("f32", None)},
        "test_edge_scale_f32": {("f32", None)},
    }


def _program_launches(lib, ops):
    """(test, kind, instance) of every OP_ATTN / OP_ATTN_NAT / OP_SOFTMAX descriptor of a program"""
    out = []
    for op in ops:
        k = int(op.kind)
        if k == lib.OP_ATTN_NAT:
            s = op.u.small
            out.append(_nat_key(lib, int(s.i[0]), int(s.i[5]), int(s.l[0]), bool(s.p[3])) + (int(s.l[0]),))
        elif k == lib.OP_ATTN:
            a = op.u.attn
            assert a.dtype == lib.EOD_F16
            out.append(("test_edge_attention_fwd_packed", "f16", (-(-a.dpad // 16), -(-a.d // 32)), 0))
        elif k == lib.OP_SOFTMAX:
            s = op.u.small
            out.append(("test_edge_softmax_rows_forward_and_backward", "f16" if int(s.i[0]) == lib.EOD_F16 else "f32",
                        _softmax_route(int(s.i[1]), int(s.l[0]), int(s.l[1])), 0))
    return out


def test_edge_every_attention_launch_of_the_real_programs_is_pinned_here():
    """(g) inference programs in the three precisions that hold a narrow head (2 x 32 channels), a wide head (1 x 128) and a head dim of 12
    (8 heads in 96 channels), and a small fp16 and a small fp32 UNetTrainer: every OP_ATTN / OP_ATTN_NAT / OP_SOFTMAX descriptor and every
    eod_rowdot / eod_attention_bwd / eod_softmax_bwd_rows / eod_scale_f32 call of UNetTrainer.bwd must be a (kernel instance, flags) that a
    test_edge_* table of this module reaches"""
    import gc
    from eo_diffusion_amd.backbones.unet_openai import UNetModel
    from eo_diffusion_amd.training import UNetTrainer
    lib = _lib()
    pinned = _pinned()
    for name in pinned:
        assert callable(globals().get(name)) and name.startswith("test_edge_"), name
    found = set()

    def need(test, kind, inst, where):
        assert (kind, inst) in pinned[test], f"{where}: launch ({kind}, {inst}) is not reached by the table of {test}"
        found.add((test, kind, inst))

    both = 0
    archs = {"narrow": dict(model_channels=32, channel_mult=[1, 2], num_head_channels=32), "wide": dict(model_channels=64, channel_mult=[1, 2], num_heads=1),
             "d12": dict(model_channels=96, channel_mult=[1, 1], num_heads=8)}
    for label, arch in archs.items():
        for prec in ("fp32", "fp16", "fp32x3"):
            u = UNetModel(32, 3, arch["model_channels"], 3, 1, [2], **{k: v for k, v in arch.items() if k != "model_channels"})
            u = u.set_precision(prec).to(DEV).eval()
            prog = u.program_for(2, 3, 0, 32, 32, torch.device(DEV), False)
            launches = _program_launches(lib, prog.ops)
            assert launches, f"{label} {prec}: the program holds no attention launch"
            for test, kind, inst, flags in launches:
                need(test, kind, inst, f"{label} {prec}")
                both += int(bool(flags & lib.ATTN_IN_PRESPLIT) and bool(flags & lib.ATTN_OUT_PRESPLIT))
            print(f"LEDGER inference {label:6s} {prec:6s}: {sorted(set(l[:3] for l in launches))}")
            del prog, u
            gc.collect()
            torch.cuda.empty_cache()
    assert both >= 1, "no harvested launch carries both pre-split flags"
    # trainers: one head of 32 channels and, one level down, one head of 128: fp16 at 16 x 16 (T = 256: flash; T = 64 = Tp: the 2^12 scale
    # and the dS epilogue), fp32 at 10 x 10 (T = 100 = Tp; T = 25, Tp = 28: the row-wise softmax backward)
    calls = collections.Counter()
    for prec, side in (("fp16", 16), ("fp32", 10)):
        u = UNetModel(side, 3, 32, 3, 1, [1, 2], channel_mult=[1, 4], num_heads=1).set_precision(prec).to(DEV).train()
        tr = UNetTrainer(u, 2, side, side, DEV, loss_scale=(1024.0 if prec == "fp16" else 1.0))
        launches = _program_launches(lib, tr.prog.ops)
        for test, kind, inst, flags in launches:
            need(test, kind, inst, f"trainer {prec} forward")
        seen = []
        for item in tr.bwd:
            if item[0] != "call":
                continue
            f, a = item[1].__name__, item[2]
            if f == "eod_rowdot":
                need("test_edge_rowdot", "f16" if a[2] == lib.EOD_F16 else "f32", None, f"trainer {prec}")
            elif f == "eod_attention_bwd":
                assert a[5] == lib.EOD_F16
                need("test_edge_attention_bwd_alone", "f16", _inst(a[10]), f"trainer {prec}")
            elif f == "eod_softmax_bwd_rows":
                need("test_edge_softmax_rows_forward_and_backward", "f16" if a[5] == lib.EOD_F16 else "f32", _softmax_route(a[7], a[3], a[1]), f"trainer {prec}")
            elif f == "eod_scale_f32":
                need("test_edge_scale_f32", "f32", None, f"trainer {prec}")
            else:
                continue
            calls[f] += 1
            seen.append(f)
        print(f"LEDGER trainer {prec}: forward {sorted(set(l[:3] for l in launches))}, backward calls {sorted(set(seen))}")
        del tr, u
        gc.collect()
        torch.cuda.empty_cache()
    for f in ("eod_rowdot", "eod_attention_bwd", "eod_softmax_bwd_rows", "eod_scale_f32"):
        assert calls[f] >= 1, f"no trainer calls {f}: the ledger does not see it"
    print("LEDGER found:", sorted(found, key=repr))
