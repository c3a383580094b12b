"""GPU: the ops that sit between the convs of the inference forward, called through the C ABI on fresh seeded tensors and compared
with the float64 references of tests/ref64.py (themselves tested on the CPU in tests/test_ref64.py): eod_resample2x, the two layout
conversions, eod_time_embed, eod_pack_rows, the bound chain (eod_act_bound, eod_weight_l1max, eod_bound_affine) and the GroupNorm chain
(eod_gn_partial -> eod_gn_finalize -> eod_gn_apply).  Shapes are hand-picked from the kernels' loop structure: the smallest that reach
each branch (tails behind a stride, second table passes, two channel blocks, empty ranges).

Every output lies between two 4 KiB guard bands (Guarded of tests/test_gpu_conv_programs.py) and is NaN-filled before the launch; every
case runs twice and the two runs must be bit-identical.  fp16 operands are rounded first and the reference is built from the rounded
values.  Copies, casts and maxima are gated on bit equality; sums on element-wise bounds derived from the arithmetic; the GroupNorm chain
and the embedding MLP on the gates below.

GroupNorm metrics.  y = x * scale + shift cancels where a group has (almost) no spread (one pixel, one channel per group: y = beta), so an
error relative to |y| says nothing about the kernel there.  Every GroupNorm error is therefore taken relative to an ALLOWANCE derived
per element from the reference's own float64 quantities (u = 2^-24, T = slot_pixels / ry + ry + 2 the length of the kernel's fp32
summation chain, kappa = 1 + mean^2 / (var + eps) of the element's group):
    statistics  A = 1/2 kappa T u           relative error of rstd from one-pass fp32 {sum, sumsq} slots (section B measures this term)
    scale       |scale| (6 u + A)
    shift       (|beta| + |mean scale|) (6 u + A) + |film shift| u + |scale| T u rms(x)
    y           6 u (|x scale| + |shift|) + (|x| + |mean|) |scale| A + |scale| T u rms(x)    (x 1.1 + 4 u terms behind a SiLU,
                + 2^-11 |y| with fp16 storage, + 2^-22 |y| + 2^-25 / s written pre-split)
and the gate is on the ratio error / allowance over a region (image, channel of an image, slab of an image), in L2.  A ratio of 1 is the
derived ceiling; each gate is at most about 4x the worst ratio measured on an MI355X (value in the comment next to it).  Where the group
is well conditioned the allowance is a few u of |y| and the ratio is a scaled rel-L2."""
import collections
import ctypes
import math
import types

import pytest
import torch

from tests import ref64
from tests.test_gpu_conv_programs import Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
INF = float("inf")
F16, F32, F64 = torch.float16, torch.float32, torch.float64
U = 2.0 ** -24
EPS = 1e-5

GATE = {
    # eod_time_embed, rel-L2 per image of h1 / emb / out against the float64 chain.  Ceiling 1e-5 (what tests/test_gpu_train_kernels.py
    # derives for the same fp32 dot products, "small").  Measured worst: h1 1.29e-7, emb 1.60e-7, out 1.97e-7
    "temb_h1": 5e-7,
    "temb_emb": 6.4e-7,
    "temb_out": 8e-7,
    # GroupNorm chain, error / allowance (module docstring): ceiling 1.  Measured worst: scale 0.235, shift 0.200
    "gn_scale": 0.9,
    "gn_shift": 0.8,
    # y per image: fp32 0.058, fp16 0.474 (the fp16 output rounding fills half of its 2^-11 |y| bound in L2), pre-split 0.060
    "gn_y_f32": 0.23, "gn_y_f16": 1.0, "gn_y_split": 0.24,
    # y, worst channel of an image: fp32 0.224, fp16 0.988 (HW = 1: the region is ONE element, and a rounding error can reach its bound),
    # pre-split 0.207
    "gn_chan_f32": 0.9, "gn_chan_f16": 1.0, "gn_chan_split": 0.83,
    # y, worst slab of an image: fp32 0.059, fp16 0.474, pre-split 0.063
    "gn_slab_f32": 0.24, "gn_slab_f16": 1.0, "gn_slab_split": 0.25,
    # section B, checks 1 and 2, as ratios to their ceilings (n_terms / ry + ry + 2) u and 4 u.  Measured worst: slots of eod_gn_partial
    # 0.186, slots of the conv epilogue 0.0133 (its ceiling takes ry = 1, any summation order), finalize from its own slots 0.655
    "cond_slots_partial": 0.75,
    "cond_slots_conv": 0.053,
    "cond_finalize": 1.0,
}
# section B, check 3: rel-L2 per (image, group) of the normalised output against ref64.group_norm_forward of the stored input, by
# (route, m / sigma): (gate, worst value measured on an MI355X over 16 x 16 and 32 x 32).  The derived ceiling is computed per group in
# the test from the group's own kappa, base + 1/2 kappa T u + (m / sigma) 2^-23 with base = 2e-6 (the fp32 gate of
# tests/test_gpu_modules.py::test_group_norm_silu), and asserted as well: 2.7e-6 at m = 0, 7e-5 at 10, 7e-3 at 100 (eod_gn_partial, T = 22).
# The error grows as (m / sigma)^2: 6.5e-8 (m / sigma)^2 through eod_gn_partial, 1.5e-7 (m / sigma)^2 through a conv epilogue whose slot
# holds a whole 16 x 16 map.
COND_GATE = {
    ("partial", 0): (3.3e-7, 8.4e-8), ("partial", 3): (2.4e-6, 5.9e-7), ("partial", 10): (2.7e-5, 6.7e-6), ("partial", 30): (2.1e-4, 5.3e-5),
    ("partial", 100): (2.5e-3, 6.4e-4),
    ("conv", 0): (4e-7, 1.0e-7), ("conv", 3): (4.8e-6, 1.2e-6), ("conv", 10): (6e-5, 1.5e-5), ("conv", 30): (4e-4, 1.0e-4),
    ("conv", 100): (6e-3, 1.5e-3),
}
COND_BASE = 2e-6
WORST = collections.defaultdict(float)


def _gate(name, err, what, gate=None, ceiling=None):
    gate = GATE[name] if gate is None else gate
    if ceiling is not None:
        gate = min(gate, ceiling)
    WORST[name] = max(WORST[name], err)
    print(f"GATE {name:22s} {err:.3e} (gate {gate:.3e}, worst so far {WORST[name]:.3e})  {what}")
    assert math.isfinite(err) and err < gate, (name, err, gate, what)


def _lib():
    from eo_diffusion_amd import _lib as m
    return m


def _L():
    return _lib().lib()


def _st():
    from eo_diffusion_amd.engine import current_stream_ptr
    return current_stream_ptr(torch.device(DEV))


def _ok(rc, what):
    _lib().check(rc, what)


def _p(t):
    return 0 if t is None else t.data_ptr()


def _dt(dtype):
    return _lib().EOD_F16 if dtype == F16 else _lib().EOD_F32


def _epc(dtype):
    return 8 if dtype == F16 else 4


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


class Rng:
    def __init__(self, seed):
        self.g = torch.Generator(device=DEV)
        self.g.manual_seed(seed)

    def randn(self, shape, scale=1.0, dtype=F32, shift=0.0):
        return (torch.randn(shape, generator=self.g, device=DEV) * scale + shift).to(dtype)

    def rand(self, shape, lo=0.0, hi=1.0):
        return torch.rand(shape, generator=self.g, device=DEV) * (hi - lo) + lo

    def randint(self, hi, shape):
        return torch.randint(0, hi, shape, generator=self.g, device=DEV)

    def unit(self, shape, dtype):
        """magnitudes in [0.5, 1.5], random signs"""
        return ((self.rand(shape) + 0.5) * (self.randint(2, shape) * 2 - 1)).to(dtype)


class Out:
    """an output tensor between two guard bands"""

    def __init__(self, shape, dtype=F32):
        nbytes = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
        self.g = Guarded(nbytes)
        self.t = self.g.view(dtype, shape)

    @property
    def ptr(self):
        return self.t.data_ptr()


def twice(launch, outs, prefill=None):
    """NaN-fill the outputs, launch, twice: the two runs must agree bit for bit and the guard bands must be intact.  Returns clones of
    the outputs"""
    runs = []
    for _ in range(2):
        for o in outs:
            o.t.fill_(NAN)
        if prefill is not None:
            prefill()
        launch()
        torch.cuda.synchronize()
        runs.append([o.t.clone() for o in outs])
    for o, a, b in zip(outs, runs[0], runs[1]):
        assert _same_bits(a, b), "two runs of the same launch differ"
        assert o.g.intact(), "write outside the output tensor"
    return runs[0]


def ulp32(v):
    """the spacing of fp32 at |v| (float64 tensor)"""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -126))
    return torch.pow(torch.tensor(2.0, dtype=F64, device=v.device), (e - 24).to(F64))


# ================================================================================================ eod_resample2x
def _resample(x, mode, pad):
    N, H, W, C = x.shape
    ref = ref64.resample2x(x, mode, pad)
    y = Out(tuple(ref.shape), x.dtype)
    got, = twice(lambda: _ok(_L().eod_resample2x(_p(x), _dt(x.dtype), N, H, W, C, mode, pad, y.ptr, _st()), "resample2x"), [y])
    assert not bool(torch.isnan(got).any()), f"unwritten output element: mode {mode} pad {pad} {tuple(x.shape)}"
    return got, ref


def _rs_in(r, shape, dtype):
    # fp16 cases: magnitudes in [0.5, 1.5], i.e. multiples of 2^-11.  A window sum is then exact in fp32 and times 0.25 either zero or at
    # least 2^-13, so no result is an fp16 subnormal, where the rounding would be 2^-25 absolute instead of the 2^-11 |ref| of the bound
    return r.unit(shape, dtype) if dtype == F16 else r.randn(shape)


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_edge_resample_pool_and_sum(dtype):
    """mode 0 (2 x 2 mean, odd maps floor) and mode 2 (2 x 2 sums behind pad_tl skipped rows / columns): |got - ref| <= 3 u sum|window| *
    factor (+ 2^-11 |ref| in fp16); mode 2 is the adjoint of mode 1: <mode1(x), g> = <x, mode2(g)>"""
    r = Rng(11)
    h16 = 2.0 ** -11 if dtype == F16 else 0.0
    for N in (1, 3):
        for C in (8, 40):
            for H, W in ((2, 2), (5, 7), (6, 4)):
                x = _rs_in(r, (N, H, W, C), dtype)
                got, ref = _resample(x, 0, 0)
                assert got.shape[1:3] == (H // 2, W // 2)
                bound = 3 * U * 0.25 * 4 * ref64.resample2x(x.abs(), 0) + h16 * ref.abs()
                assert bool(((got.double() - ref).abs() <= bound).all()), ("mode 0", N, C, H, W)
            for pad in (0, 1):
                for h, w in ((1, 1), (3, 3), (2, 2), (5, 7), (6, 4)):
                    g = _rs_in(r, (N, 2 * h + pad, 2 * w + pad, C), dtype)
                    got, ref = _resample(g, 2, pad)
                    assert got.shape[1:3] == (h, w)
                    sabs = ref64.resample2x(g.abs(), 2, pad)
                    assert bool(((got.double() - ref).abs() <= 3 * U * sabs + h16 * ref.abs()).all()), ("mode 2", N, C, h, w, pad)
                    x = _rs_in(r, (N, h, w, C), dtype)
                    y1, _ = _resample(x, 1, pad)
                    lhs, rhs = float((y1.double() * g.double()).sum()), float((x.double() * got.double()).sum())
                    tol = float((x.double().abs() * (3 * U * sabs + h16 * got.double().abs())).sum())
                    assert abs(lhs - rhs) <= tol + 1e-12 * abs(lhs), ("adjoint of mode 1", N, C, h, w, pad, lhs, rhs, tol)


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_edge_resample_copies_are_bit_exact(dtype):
    """modes 1 and 4 copy elements, mode 3 multiplies by a power of two: bit equality.  The pad rows / columns are +0.  Mode 3 is the
    adjoint of mode 0 (with pad_tl = 1 on a map odd in both axes)"""
    r = Rng(12)
    for N in (1, 3):
        for C in (8, 40):
            for H, W in ((1, 1), (3, 3), (2, 2), (5, 7), (6, 4)):
                x = _rs_in(r, (N, H, W, C), dtype)
                for pad in (0, 1):
                    got, ref = _resample(x, 1, pad)
                    assert got.shape[1:3] == (2 * H + pad, 2 * W + pad)
                    assert _same_bits(got, ref.to(dtype)), ("mode 1", N, C, H, W, pad)
                    if pad:
                        assert not bool(_bits(got[:, 0]).any()) and not bool(_bits(got[:, :, 0]).any()), "pad row / column is not +0"
                    got, ref = _resample(x, 3, pad)
                    assert _same_bits(got, ref.to(dtype)), ("mode 3", N, C, H, W, pad)
                    if pad:
                        assert not bool(_bits(got[:, -1]).any()) and not bool(_bits(got[:, :, -1]).any()), "pad row / column is not +0"
                    assert _same_bits(got[:, :2 * H:2, :2 * W:2], x * 0.25), "mode 3 is not x * 0.25"
                if H >= 2:
                    for pad in (0, 1, 2, 3):
                        got, ref = _resample(x, 4, pad)
                        assert got.shape[1:3] == (H - (pad & 1), W - (pad >> 1))
                        assert _same_bits(got, ref.to(dtype)), ("mode 4", N, C, H, W, pad)
            h16 = 2.0 ** -11 if dtype == F16 else 0.0
            for H, W in ((5, 7), (6, 4), (2, 2), (3, 3)):  # mode 3 as the adjoint of mode 0
                x = _rs_in(r, (N, H, W, C), dtype)
                g = _rs_in(r, (N, H // 2, W // 2, C), dtype)
                y0, _ = _resample(x, 0, 0)
                g3, _ = _resample(g, 3, H % 2)
                assert g3.shape[1:3] == (H, W)
                lhs, rhs = float((y0.double() * g.double()).sum()), float((x.double() * g3.double()).sum())
                tol = float((g.double().abs() * (3 * U * ref64.resample2x(x.abs(), 0) + h16 * y0.double().abs())).sum())
                assert abs(lhs - rhs) <= tol + 1e-12 * abs(lhs), ("adjoint of mode 0", N, C, H, W, lhs, rhs, tol)


def test_edge_resample_second_trip_of_the_grid_stride_loop():
    """more than 8192 * 256 output elements: the grid is capped and every thread takes further trips"""
    x = Rng(13).randn((1, 256, 256, 40), dtype=F16)
    got, ref = _resample(x, 1, 0)
    assert got.numel() > 8192 * 256
    assert _same_bits(got, ref.to(F16))


def test_edge_average_pool_backward_of_a_map_odd_in_one_axis_raises():
    """mode 3 pads both axes at once, so the backward of an average pool over a 7 x 6 map is not expressible: the trainer must say so"""
    from eo_diffusion_amd.engine import Act, Program
    from eo_diffusion_amd.training import UNetTrainer
    bp = Program(DEV, "fp32")
    tr = object.__new__(UNetTrainer)
    tr.bprog, tr.bwd = bp, []
    src, y = bp.act(1, 7, 6, 8), bp.act(1, 3, 3, 8)
    dy = Act(torch.zeros((1, 3, 3, 8), device=DEV), 1, 3, 3, 8)
    tr._take_grad = lambda a: dy
    tr._add_grad = lambda a, g: pytest.fail("a gradient of the wrong shape was accepted")
    with pytest.raises(_lib().EodError, match="resample backward shape mismatch"):
        tr._pool_bwd(types.SimpleNamespace(y=y, mode=0, pad_tl=False, src=src))


# ================================================================================================ layout conversions
@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_edge_nchw_to_nhwc(dtype):
    r = Rng(21)
    N, H, W = 3, 5, 7
    for C0, C1, cp in ((3, 0, 4), (3, 0, 8), (13, 0, 16), (5, 3, 8), (7, 9, 16)):
        s0 = r.randn((N, C0, H, W))
        s1 = r.randn((N, C1, H, W)) if C1 else None
        y = Out((N, H, W, cp), dtype)
        got, = twice(lambda: _ok(_L().eod_nchw_to_nhwc(_p(s0), C0, _p(s1), C1, y.ptr, _dt(dtype), N, H, W, cp, _st()), "nchw_to_nhwc"), [y])
        cat = s0 if s1 is None else torch.cat([s0, s1], 1)
        assert _same_bits(got[..., :C0 + C1], cat.permute(0, 2, 3, 1).to(dtype).contiguous()), (C0, C1, cp)
        assert not bool(_bits(got[..., C0 + C1:]).any()), ("pad channels are not +0", C0, C1, cp)


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_edge_nhwc_to_nchw(dtype):
    r = Rng(22)
    N = 2
    for C in (3, 32, 33, 40):
        for H, W in ((1, 1), (31, 1), (1, 32), (33, 1), (35, 3)):
            x = r.randn((N, H, W, C), dtype=dtype)
            y = Out((N, C, H, W))
            got, = twice(lambda: _ok(_L().eod_nhwc_to_nchw(_p(x), _dt(dtype), y.ptr, N, H, W, C, _st()), "nhwc_to_nchw"), [y])
            assert _same_bits(got, x.float().permute(0, 3, 1, 2).contiguous()), (C, H, W)


# ================================================================================================ eod_time_embed
def _freqs(D):
    half = D // 2
    return torch.exp(-math.log(10000.0) * torch.arange(half, dtype=F32) / max(half, 1)).to(DEV)


def _temb_params(r, D, E, J, labels):
    p = types.SimpleNamespace()
    p.w1, p.b1 = r.randn((E, D), 1.0 / math.sqrt(D)), r.randn((E,), 0.3)
    p.w2, p.b2 = r.randn((E, E), 1.0 / math.sqrt(E)), r.randn((E,), 0.3)
    p.wcat, p.bcat = (r.randn((J, E), 1.0 / math.sqrt(E)), r.randn((J,), 0.3)) if J else (None, None)
    p.lab = r.randn((4, E), 0.5) if labels else None
    p.freqs = _freqs(D)
    return p


def _temb_inputs(r, N, t_f32, labels):
    if t_f32:
        t = r.rand((N,), 0.0, 999.0)
        t[0], t[-1] = 0.5, 999.0
    else:
        t = r.randint(1000, (N,))
        t[0], t[-1] = 0, 999
    y = None
    if labels:
        y = r.randint(4, (N,))
        y[0] = y[-1] = 3          # the last class, repeated
        if N > 2:
            y[1] = y[2]
    return t.contiguous(), y


def _temb_launch(p, t, y, N, D, E, J, *, emb_in=None):
    """-> (h1, emb, out) of one eod_time_embed (None where the stage does not run)"""
    lib = _lib()
    d = lib.TembDesc()
    stage3_only = emb_in is not None
    h1 = None if stage3_only else Out((N, E))
    emb = None if stage3_only else Out((N, E))
    out = Out((N, J)) if J else None
    if stage3_only:
        d.emb = _p(emb_in)
    else:
        d.t, d.freqs, d.w1, d.b1, d.w2, d.b2 = _p(t), _p(p.freqs), _p(p.w1), _p(p.b1), _p(p.w2), _p(p.b2)
        d.label_emb, d.y = _p(p.lab) if y is not None else 0, _p(y)
        d.h1, d.emb = h1.ptr, emb.ptr
        d.t_f32 = int(t.is_floating_point())
    if J:
        d.wcat, d.bcat, d.out = _p(p.wcat), _p(p.bcat), out.ptr
    d.N, d.D, d.E, d.J = N, D, E, J
    outs = [o for o in (h1, emb, out) if o is not None]
    got = twice(lambda: _ok(_L().eod_time_embed(ctypes.byref(d), _st()), "time_embed"), outs)
    got = dict(zip([n for n, o in (("h1", h1), ("emb", emb), ("out", out)) if o is not None], got))
    return got.get("h1"), got.get("emb"), got.get("out")


def _rel_rows(got, ref):
    return float(((got.double() - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-300)).max())


def _temb_check(N, D, E, J, t_f32, labels, seed):
    r = Rng(seed)
    p = _temb_params(r, D, E, J, labels)
    t, y = _temb_inputs(r, N, t_f32, labels)
    h1, emb, out = _temb_launch(p, t, y, N, D, E, J)
    rh, re, ro = ref64.time_embed(t, p.freqs, p.w1, p.b1, p.w2, p.b2, p.wcat, p.bcat, label_emb=p.lab if labels else None, y=y)
    what = f"N={N} D={D} E={E} J={J} t_f32={t_f32} labels={labels}"
    for g in (h1, emb, out):
        assert g is None or bool(torch.isfinite(g).all()), "unwritten / non-finite output: " + what
    _gate("temb_h1", _rel_rows(h1, rh), what)
    _gate("temb_emb", _rel_rows(emb, re), what)
    if J:
        _gate("temb_out", _rel_rows(out, ro), what)


@pytest.mark.parametrize("D,E", [(32, 128), (33, 64), (128, 512), (160, 640)])
def test_edge_time_embed(D, E):
    """table passes (N = 17: two, 33: three, with nb < 16 tails), odd D, E = 512 (the last size on the table kernel) and E = 640 (stages
    2 and 3 on the fallback), J = 20 (a partial last block whose last wave leaves after some of its four columns)"""
    seed = 30
    for N in (1, 16, 17, 33):
        for J in (0, 20, 3 * E):
            for t_f32 in (0, 1):
                for labels in (False, True):
                    seed += 1
                    _temb_check(N, D, E, J, t_f32, labels, seed)


def test_edge_time_embed_stage1_on_the_fallback_kernel():
    for N, t_f32 in ((1, 0), (17, 1)):
        _temb_check(N, 520, 128, 20, t_f32, True, 29)


def test_edge_time_embed_stage3_alone():
    """w1 == NULL: `emb` is an input, only stage 3 runs (table kernel at E = 128, fallback at E = 640)"""
    for N, E, J in ((1, 128, 20), (17, 128, 3 * 128), (33, 640, 20)):
        r = Rng(28)
        p = _temb_params(r, 32, E, J, False)
        emb_in = r.randn((N, E))
        h1, emb, out = _temb_launch(p, None, None, N, 0, E, J, emb_in=emb_in)
        assert h1 is None and emb is None
        _gate("temb_out", _rel_rows(out, ref64.time_embed(None, None, None, None, None, None, p.wcat, p.bcat, emb=emb_in)[2]), f"stage 3 alone N={N} E={E} J={J}")


def test_edge_time_embed_table_and_fallback_routes_agree_bit_for_bit():
    """Both routes promise the same summation order per column (lane l adds k = l, l + 64, ...; then the same wave reduction), so a shape
    on the table route and the same weights zero-extended onto the fallback route give the same bits: a zero weight adds +-0.
    D goes 512 -> 640 and not 520: the sinusoid is [cos | sin], so growing D by 8 would move every sin column to another lane (k = half + m)
    and change the order by construction.  With half = 256 -> 320 the sin columns keep their lanes (320 = 5 * 64); the 64 new cos / sin
    columns get zero weights.  E goes 512 -> 520: the extra h1 / emb columns are SiLU(0) = 0 and meet zero weights."""
    N, D, E, J, D2, E2 = 17, 512, 512, 20, 640, 520
    r = Rng(27)
    p = _temb_params(r, D, E, J, True)
    t, y = _temb_inputs(r, N, 0, True)
    a = _temb_launch(p, t, y, N, D, E, J)
    q = types.SimpleNamespace()
    z = lambda shape: torch.zeros(shape, device=DEV)
    q.w1 = z((E2, D2))
    q.w1[:E, :256], q.w1[:E, 320:576] = p.w1[:, :256], p.w1[:, 256:]
    q.b1, q.b2 = z((E2,)), z((E2,))
    q.b1[:E], q.b2[:E] = p.b1, p.b2
    q.w2 = z((E2, E2))
    q.w2[:E, :E] = p.w2
    q.lab = z((4, E2))
    q.lab[:, :E] = p.lab
    q.wcat, q.bcat = z((J, E2)), p.bcat
    q.wcat[:, :E] = p.wcat
    q.freqs = torch.cat([p.freqs, r.rand((64,), 0.0, 1e-4)])
    b = _temb_launch(q, t, y, N, D2, E2, J)
    for name, u, v in zip(("h1", "emb"), a, b):
        assert _same_bits(u, v[:, :E].contiguous()), name + ": table and fallback route differ"
        assert not bool(_bits(v[:, E:]).any()), name + ": extension columns are not +0"
    assert _same_bits(a[2], b[2]), "out: table and fallback route differ"


# ================================================================================================ eod_pack_rows
@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_edge_pack_rows(dtype):
    r = Rng(41)
    for rows, cols in ((1, 1), (7, 40), (3 * 96, 96)):
        nsrc = rows + 2
        maps = {"identity": None, "permutation": torch.randperm(rows, generator=torch.Generator().manual_seed(rows)).int(),
                "repeated": (torch.arange(rows) * 3 % max(1, rows // 2)).int(),
                "negative": torch.where(torch.arange(rows) % 3 == 1, torch.tensor(-1), torch.arange(rows)).int()}
        maps["negative"][-1] = -7
        for ld_src, ld_dst in ((cols, cols), (cols + 3, cols + 5)):
            src = r.randn((nsrc, ld_src))
            for name, m in maps.items():
                md = None if m is None else m.to(DEV)
                dst = Out((rows, ld_dst), dtype)
                got, = twice(lambda: _ok(_L().eod_pack_rows(_p(src), ld_src, _p(md), dst.ptr, ld_dst, _dt(dtype), rows, cols, _st()), "pack_rows"), [dst])
                idx = torch.arange(rows, device=DEV) if md is None else md.long()
                ref = torch.where((idx >= 0)[:, None], src[idx.clamp_min(0), :cols], torch.zeros((), device=DEV)).to(dtype)
                what = (rows, cols, ld_src, ld_dst, name)
                assert _same_bits(got[:, :cols], ref), what
                assert bool(torch.isnan(got[:, cols:]).all()), ("gap columns of dst were written", what)
                if md is not None and name == "negative":
                    assert not bool(_bits(got[:, :cols][idx < 0]).any()), ("a negative row is not +0", what)


# ================================================================================================ the bound chain
def _act_bound_direct(x, N, per, accumulate=0, prefill=None):
    ab = Out((N, 32))
    got, = twice(lambda: _ok(_L().eod_act_bound(_p(x), _dt(x.dtype), N, per, 0, 0, 0, 0, 0, 0, ab.ptr, accumulate, _st()), "act_bound"), [ab],
                 prefill=None if prefill is None else (lambda: ab.t.copy_(prefill)))
    return got


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_edge_act_bound_direct(dtype):
    """entry j = max|x| over the j-th 1/32 of the image's 16-byte chunks, bit for bit; an empty range writes 0; NaN / inf -> +inf in its
    own entry only; accumulate keeps the entry-wise maximum"""
    epc = _epc(dtype)
    r = Rng(51)
    for N in (1, 3):
        for chunks in (1, 31, 32 * 256 + 5):
            per = chunks * epc
            x = r.randn((N, per), dtype=dtype)
            x[N - 1, per - 1] = 60.0          # the maximum in the last chunk of the last image: entry 31
            ref = ref64.act_bound_direct(x, epc)
            got = _act_bound_direct(x, N, per)
            what = (N, chunks)
            assert _same_bits(got, ref.float()), what
            assert float(got[N - 1, 31]) == 60.0 == float(got[N - 1].max())
            if chunks < 32:
                assert int((got == 0).sum()) == N * (32 - chunks), ("an empty range must write 0", what)
            xb = x.clone()
            xb[0, per // 2] = NAN
            xb[N - 1, 0] = -INF
            refb = ref64.act_bound_direct(xb, epc)
            gotb = _act_bound_direct(xb, N, per)
            assert _same_bits(gotb, refb.float()), ("NaN / inf", what)
            assert int(torch.isinf(gotb).sum()) == int(torch.isinf(refb).sum()) in (1, 2) and not bool(torch.isnan(gotb).any())
            pre = ref.float() * torch.where(torch.arange(32, device=DEV) % 2 == 0, 4.0, 0.25)[None]   # larger and smaller than what comes
            pre[0, 5] = INF
            gota = _act_bound_direct(x, N, per, accumulate=1, prefill=pre)
            assert _same_bits(gota, torch.maximum(pre, ref.float())), ("accumulate", what)
            assert float(gota[0, 5]) == INF


def _act_bound_parts(parts, N):
    ab = Out((N, 32))
    a = [(_p(t), t.shape[1], t.shape[2]) for t in parts] + [(0, 0, 0)] * (2 - len(parts))
    got, = twice(lambda: _ok(_L().eod_act_bound(0, _lib().EOD_F32, N, 0, a[0][0], a[0][1], a[0][2], a[1][0], a[1][1], a[1][2], ab.ptr, 0, _st()),
                             "act_bound"), [ab])
    return got


def test_edge_act_bound_parts():
    """entry j = sqrt(max sumsq over the j-th 1/32 of every source's {sum, sumsq} pairs), within 1 ulp; P * C no multiple of 32, one
    source shorter than the table; a NaN sum of squares -> +inf"""
    r = Rng(52)
    for N in (1, 3):
        for shapes in (((3, 40),), ((3, 40), (1, 24)), ((1, 8),)):
            parts = [r.randn((N, P, C, 2)).abs() * 10.0 ** float(k) for k, (P, C) in enumerate(shapes)]
            parts[-1][N - 1, -1, -1, 1] = 1e6   # the maximum in the last pair: entry 31
            got = _act_bound_parts(parts, N)
            ref = ref64.act_bound_parts(parts)
            assert bool(((got.double() - ref).abs() <= ulp32(ref)).all()) and not bool(torch.isnan(got).any()), (N, shapes)
            assert float(got[N - 1, 31]) == 1000.0
            parts[0][0, -1, 3, 1] = NAN
            got = _act_bound_parts(parts, N)
            ref = ref64.act_bound_parts(parts)
            assert int(torch.isinf(got).sum()) == 1 and bool((torch.isinf(got) == torch.isinf(ref)).all()), (N, shapes)


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_edge_act_bound_of_gn_partial_slots_bounds_the_tensor(dtype):
    """parts mode on the slots eod_gn_partial wrote for a real tensor: max_j ab[n][j] >= max|x_n| (1 - 2^-22)"""
    r = Rng(53)
    N, HW, C, P = 3, 35, 40, 3
    x = r.randn((N, HW, C), dtype=dtype) * torch.tensor([1e-3, 1.0, 300.0], device=DEV).to(dtype)[:, None, None]
    part = Out((N, P, C, 2))
    slots, = twice(lambda: _ok(_L().eod_gn_partial(_p(x), _dt(dtype), N, HW, C, part.ptr, P, C, 0, _st()), "gn_partial"), [part])
    got = _act_bound_parts([slots], N)
    true = x.double().abs().amax((1, 2))
    assert bool((got.double().amax(1) >= true * (1 - 2.0 ** -22)).all()), (got.amax(1), true)
    assert bool((got.double().amax(1) <= true * math.sqrt(-(-HW // P)) * (1 + 1e-5)).all()), "looser than sqrt(pixels per slot)"


def test_edge_weight_l1max_and_bound_affine():
    r = Rng(54)
    for rows, cols in ((1, 1), (5, 255), (96, 257), (1536, 512)):
        w = r.randn((rows, cols)) * torch.pow(10.0, r.rand((rows, 1), -3.0, 1.0))
        w[-1] = r.randn((cols,)).abs().clamp_min(0.1) * 1e3    # the largest row last
        b = r.randn((rows,))
        b[-1] = -7.5
        for bias in (None, b):
            coef = Out((2,))
            got, = twice(lambda: _ok(_L().eod_weight_l1max(_p(w), rows, cols, _p(bias), coef.ptr, _st()), "weight_l1max"), [coef])
            Lmax, bmax = ref64.linear_bound(w, bias)
            assert int(w.double().abs().sum(1).argmax()) == rows - 1
            assert Lmax <= float(got[0]) <= 1.0002 * Lmax, (rows, cols, float(got[0]), Lmax)
            assert _same_bits(got[1:], torch.tensor([bmax], dtype=F32, device=DEV)), (rows, cols, float(got[1]), bmax)
    for N in (1, 3):
        tab = r.rand((N, 32), 0.0, 50.0)
        tab[:, 7] = 0.0
        for c0, c1 in ((3.7, 0.0), (0.013, 2.5)):
            coef = torch.tensor([c0, c1], device=DEV)
            out = Out((N, 32))
            got, = twice(lambda: _ok(_L().eod_bound_affine(_p(tab), _p(coef), out.ptr, N, _st()), "bound_affine"), [out])
            ref = tab.double() * coef.double()[0] + coef.double()[1]
            assert bool(((got.double() - ref).abs() <= ulp32(ref)).all()), (N, c0, c1)


@pytest.mark.parametrize("N", [1, 3])
def test_edge_bound_chain_bounds_a_linear_layer(N):
    """act_bound (direct) -> weight_l1max -> bound_affine on y = W x + b: the table bounds max|y_n| and the scale presplit_scale derives
    from it keeps s max|y_n| inside the fp16 range"""
    r = Rng(55)
    K, R = 96, 40
    x = r.randn((N, K)) * torch.tensor([1e-4, 1.0, 3e4], device=DEV)[:N, None]
    w, b = r.randn((R, K)), r.randn((R,), 2.0)
    tab, coef, out = Out((N, 32)), Out((2,)), Out((N, 32))

    def launch():
        L, st = _L(), _st()
        _ok(L.eod_act_bound(_p(x), _lib().EOD_F32, N, K, 0, 0, 0, 0, 0, 0, tab.ptr, 0, st), "act_bound")
        _ok(L.eod_weight_l1max(_p(w), R, K, _p(b), coef.ptr, st), "weight_l1max")
        _ok(L.eod_bound_affine(tab.ptr, coef.ptr, out.ptr, N, st), "bound_affine")
    _, _, got = twice(launch, [tab, coef, out])
    ymax = (x.double() @ w.double().t() + b.double()).abs().amax(1)
    assert bool((ymax * (1 - 2.0 ** -20) <= got.double().amax(1)).all()), (ymax, got.amax(1))
    assert bool((ref64.presplit_scale(got) * ymax < 65504.0).all())


# ================================================================================================ GroupNorm chain
def gn_slab(N, HW, C, epc, unroll):
    """the slab decomposition of csrc/common.h"""
    cols = C // epc
    nz = (cols + 255) // 256
    cpp = (cols + nz - 1) // nz
    ry = max(1, 256 // cpp)
    q = ry * unroll
    want = (4096 + N - 1) // N
    per = (HW + want - 1) // want
    per = (per + q - 1) // q * q
    return types.SimpleNamespace(cpp=cpp, ry=ry, per=per, P=(HW + per - 1) // per, nz=nz)


def _slot_sums(x, P):
    """float64 {sum, sumsq} [N][P][C][2] over exactly the pixels of every slot of eod_gn_partial (slot p = pixels [p per, (p + 1) per),
    per = ceil(HW / P)), and the sums of |terms| the errors are relative to"""
    N, HW, C = x.shape
    per = -(-HW // P)
    seg = torch.nn.functional.pad(x.double(), (0, 0, 0, P * per - HW)).reshape(N, P, per, C)
    return torch.stack([seg.sum(2), seg.square().sum(2)], -1), torch.stack([seg.abs().sum(2), seg.square().sum(2)], -1)


def _regions(err, allow, per):
    """(image, channel, slab) maxima of ||err|| / ||allow|| over [N][HW][C]"""
    e2, a2 = err.square(), allow.square()
    ratio = lambda e, a: float((e / a.clamp_min(1e-300)).sqrt().max())
    N, HW, C = err.shape
    pad = -HW % per
    slab = lambda t: torch.nn.functional.pad(t.sum(2), (0, pad)).reshape(N, -1, per).sum(2)
    return ratio(e2.sum((1, 2)), a2.sum((1, 2))), ratio(e2.sum(1), a2.sum(1)), ratio(slab(e2), slab(a2))


def gn_chain(dtype, N, HW, srcs, groups, *, film=False, silu=True, split=False, own_table=False, seed=61, what=""):
    """eod_gn_partial (per source) -> eod_gn_finalize -> eod_gn_apply (per source, each into its own NaN-filled Ctot-wide tensor).
    srcs = [(C, P), ...]"""
    L, lib = _L(), _lib()
    r = Rng(seed)
    epc, dt = _epc(dtype), _dt(dtype)
    Ctot = sum(c for c, _ in srcs)
    cpg = Ctot // groups
    xs = [r.randn((N, HW, C), 1.0 + 0.5 * k, dtype, shift=0.25 * (k + 1)) for k, (C, _) in enumerate(srcs)]
    gam, bet = r.randn((Ctot,), 0.2, shift=1.0), r.randn((Ctot,), 0.1)
    fstride = 2 * Ctot + 8
    fl = r.randn((N, fstride), 0.3) if film else None
    parts = [Out((N, P, C, 2)) for C, P in srcs]
    ss, abr, abn = Out((N, Ctot, 2)), Out((N, 32)), Out((N, 32))
    ys = [Out((N, HW, Ctot), dtype) for _ in srcs]
    table = None
    if own_table:   # a table of the caller's whose maximum sits in entry 31 (16x the true bound: still 2^-22-grade for the large elements)
        table = torch.zeros((N, 32), device=DEV)

    def prefill():  # (entries [groups, 32) of the tables are the caller's to zero)
        abr.t[:, groups:] = 0.0
        abn.t[:, groups:] = 0.0

    def launch():
        st = _st()
        for x, o, (C, P) in zip(xs, parts, srcs):
            _ok(L.eod_gn_partial(_p(x), dt, N, HW, C, o.ptr, P, C, 0, st), "gn_partial")
        p1 = (parts[1].ptr, srcs[1][1], srcs[1][0]) if len(srcs) == 2 else (0, 0, 0)
        _ok(L.eod_gn_finalize(parts[0].ptr, srcs[0][1], srcs[0][0], p1[0], p1[1], p1[2], N, HW, groups, EPS, _p(gam), _p(bet), _p(fl), fstride,
                              ss.ptr, abr.ptr, abn.ptr, st), "gn_finalize")
        if own_table:
            torch.cuda.synchronize()
            table.zero_()
            table[:, 31] = abn.t.max(1).values * 16.0
            table[:, 3] = abn.t.max(1).values * 0.5
        coff = 0
        for x, y, (C, _) in zip(xs, ys, srcs):
            _ok(L.eod_gn_apply(_p(x), dt, N, HW, C, ss.ptr, Ctot, coff, int(silu), y.ptr, _p(table) if own_table else (abn.ptr if split else 0), st), "gn_apply")
            coff += C
    got = twice(launch, parts + [ss, abr, abn] + ys, prefill)
    g_parts, (g_ss, g_abr, g_abn), g_ys = got[:len(srcs)], got[len(srcs):len(srcs) + 3], got[len(srcs) + 3:]

    # ---- float64 reference quantities
    x = torch.cat(xs, 2).double()
    fm = (fl[:, :Ctot], fl[:, Ctot:2 * Ctot]) if film else None
    ss_ref = ref64.group_norm_scale_shift(x, gam, bet, groups, EPS, film=fm)
    y_ref = ref64.group_norm_forward(x, gam, bet, groups, EPS, silu_out=silu, film=fm)
    mean, rstd = ref64.group_norm_stats(x, groups, EPS)
    ch = lambda t: t.reshape(N, groups, 1).expand(N, groups, cpg).reshape(N, Ctot)      # per group -> per channel
    mean_c, rstd_c = ch(mean), ch(rstd)
    var_c = 1.0 / rstd_c.square() - EPS
    kappa = 1.0 + mean_c.square() / (var_c + EPS)
    rms = (var_c + mean_c.square()).sqrt()
    T = max(-(-HW // P) / gn_slab(N, HW, C, epc, 1).ry + gn_slab(N, HW, C, epc, 1).ry + 2 for C, P in srcs)
    A = 0.5 * kappa * T * U
    sc, sh = ss_ref[..., 0], ss_ref[..., 1]
    fs = (1.0 + fm[0].double()).abs() if film else 1.0
    ft = fm[1].double().abs() if film else 0.0

    # ---- slots: every {sum, sumsq} against the float64 sum over exactly its pixels, relative to the sum of |terms|
    for xk, gp, (C, P) in zip(xs, g_parts, srcs):
        per = -(-HW // P)
        ry = gn_slab(N, HW, C, epc, 1).ry
        ceil_ = (per / ry + ry + 2) * U
        assert not bool(torch.isnan(gp).any()), "unwritten slot: " + what
        ref, den = _slot_sums(xk, P)
        assert bool(((gp.double() - ref).abs() <= ceil_ * den).all()), f"slots (P = {P}): {what}"

    # ---- scale / shift per channel
    assert not bool(torch.isnan(g_ss).any()), "unwritten scale / shift entry: " + what
    _gate("gn_scale", float(((g_ss[..., 0].double() - sc).abs() / (sc.abs() * (6 * U + A))).max()), what)
    sh_allow = (bet.double().abs()[None] + (mean_c * rstd_c * gam.double()[None]).abs()) * fs * (6 * U + A) + ft * U + sc.abs() * T * U * rms
    _gate("gn_shift", float(((g_ss[..., 1].double() - sh).abs() / sh_allow).max()), what)

    # ---- y: the columns of the source, and NaN everywhere else
    cls = "split" if (split or own_table) else ("f16" if dtype == F16 else "f32")
    s_img = ref64.presplit_scale(table if own_table else g_abn) if cls == "split" else None
    coff = 0
    worst_rel = 0.0
    for gy, (C, _) in zip(g_ys, srcs):
        sl = slice(coff, coff + C)
        if cls == "split":
            inside = ref64.presplit_decode(gy[..., sl].contiguous(), s_img)
            outside = torch.cat([gy[..., :coff], gy[..., coff + C:]], 2)
        else:
            inside, outside = gy[..., sl].double(), torch.cat([gy[..., :coff], gy[..., coff + C:]], 2)
        assert bool(torch.isnan(outside).all()), "columns outside [coff, coff + C) were written: " + what
        assert bool(torch.isfinite(inside).all()), "unwritten / non-finite output: " + what
        xs_, scs, shs = x[..., sl], sc[:, None, sl], sh[:, None, sl]
        terms = (xs_ * scs).abs() + shs.abs()
        allow = 6 * U * terms + (xs_.abs() + mean_c[:, None, sl].abs()) * scs.abs() * A[:, None, sl] + scs.abs() * T * U * rms[:, None, sl]
        if silu:
            allow = 1.1 * allow + 4 * U * terms
        yr = y_ref[..., sl]
        if cls == "f16":
            allow = allow + 2.0 ** -11 * yr.abs()
        if cls == "split":
            allow = allow + 2.0 ** -22 * yr.abs() + 2.0 ** -25 / s_img[:, None, None]
        per = gn_slab(N, HW, C, epc, 4).per
        img, chan, slab = _regions(inside - yr, allow, per)
        _gate("gn_y_" + cls, img, what)
        _gate("gn_chan_" + cls, chan, what)
        _gate("gn_slab_" + cls, slab, what)
        worst_rel = max(worst_rel, float(((inside - yr).flatten(1).norm(dim=1) / yr.flatten(1).norm(dim=1).clamp_min(1e-300)).max()))
        coff += C
    print(f"GN   rel-L2 per image {worst_rel:.2e}  {what}")

    # ---- bound tables: >= the true maxima per group, never looser than the slot arithmetic allows
    xg = x.reshape(N, HW, groups, cpg)
    raw_true = xg.abs().amax((1, 3))
    z = x * sc[:, None] + sh[:, None]
    nrm_true = z.reshape(N, HW, groups, cpg).abs().amax((1, 3))
    chs = torch.cat([torch.full((C,), math.sqrt(-(-HW // P)), dtype=F64, device=DEV) for C, P in srcs])   # sqrt(slot pixels) per channel
    raw_loose = (x.abs().amax(1) * chs[None]).reshape(N, groups, cpg).amax(2)
    g_raw, g_nrm = g_abr[:, :groups].double(), g_abn[:, :groups].double()
    assert bool((g_raw >= raw_true * (1 - 2.0 ** -22)).all()) and bool((g_raw <= raw_loose * (1 + 1e-5)).all()), "ab_raw: " + what
    assert bool((g_raw <= raw_true * math.sqrt(max(-(-HW // P) for _, P in srcs) * cpg) * (1 + 1e-5)).all()), "ab_raw looser than sqrt(slot pixels * cpg): " + what
    gsc = g_ss[..., 0].double().abs().reshape(N, groups, cpg).amax(2)
    gsh = g_ss[..., 1].double().abs().reshape(N, groups, cpg).amax(2)
    assert bool((g_nrm >= nrm_true * (1 - 2.0 ** -20)).all()), "ab_norm does not bound the normalised tensor: " + what
    assert bool((g_nrm <= (gsc * raw_loose + gsh) * (1 + 1e-5)).all()), "ab_norm looser than max|scale| * sqrt(slot pixels) * max|x| + max|shift|: " + what
    if HW >= 15:   # (well-conditioned groups: the per-image looseness factors of test_bound_table_of_a_groupnorm_finalize_bounds_both_tensors)
        assert bool((g_raw.amax(1) <= 64 * raw_true.amax(1)).all()) and bool((g_nrm.amax(1) <= 256 * nrm_true.amax(1)).all()), "table looseness: " + what
    assert not bool(_bits(g_abr[:, groups:]).any()) and not bool(_bits(g_abn[:, groups:]).any()), "table entries behind the groups were written: " + what


GN_WIDTHS = [(F32, 32, 32), (F16, 32, 32), (F32, 96, 32), (F16, 96, 32), (F32, 288, 32), (F16, 288, 32), (F32, 1032, 24), (F16, 2080, 32)]


@pytest.mark.parametrize("dtype,C,groups", GN_WIDTHS, ids=[f"{'f16' if d == F16 else 'f32'}-{c}" for d, c, _ in GN_WIDTHS])
def test_edge_group_norm_slab_and_channel_block_edges(dtype, C, groups):
    """C = 32: one channel per group; 288: 72 x 3 threads, a partial last wave; 1032 fp32 / 2080 fp16: 258 / 260 chunk columns, two
    channel blocks (1032 = 24 groups of 43).  HW = 1 and 15: fewer pixels than rows of the block; P as gn_slab gives it and P = 1"""
    for HW in (1, 15, 35, 1024):
        for N in (1, 3):
            for P in sorted({gn_slab(N, HW, C, _epc(dtype), 1).P, 1}):
                gn_chain(dtype, N, HW, [(C, P)], groups, silu=(HW != 15), what=f"C={C} HW={HW} N={N} P={P} {dtype}")


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_edge_group_norm_concat_seam_and_film(dtype):
    """two sources with different slab counts whose groups straddle the seam (40 | 56 and 16 | 80 channels: 3 per group, 88 | 104: 6 per
    group; no seam is a multiple of the group width), with and without FiLM (film_stride > 2 Ctot); each apply writes its columns at coff and nothing else"""
    for HW, N in ((35, 3), (1024, 1), (15, 3)):
        for (C0, P0), (C1, P1) in (((40, min(HW, 3)), (56, 1)), ((88, 1), (104, min(HW, 5))), ((16, 1), (80, min(HW, 2)))):
            for film in (False, True):
                gn_chain(dtype, N, HW, [(C0, P0), (C1, P1)], 32, film=film, silu=film,
                         what=f"concat {C0}|{C1} P={P0}|{P1} HW={HW} N={N} film={film} {dtype}")
        gn_chain(dtype, N, HW, [(96, min(HW, 4))], 32, film=True, what=f"film C=96 HW={HW} N={N} {dtype}")


@pytest.mark.parametrize("C,groups", [(32, 32), (96, 32), (288, 32), (1032, 24)])
def test_edge_group_norm_written_presplit(C, groups):
    """split_bound: y written as [8 x fp16 hi | 8 x fp16 lo] groups scaled per image from the bound table; decoded with
    ref64.presplit_decode.  C = 1032: 129 chunk columns per block, bumped to 130 so that the DPP pair exchange stays inside a block;
    288: the partial last wave.  own_table: the image's maximum in entry 31"""
    for HW in (1, 15, 35, 1024):
        for N in (1, 3):
            gn_chain(F32, N, HW, [(C, gn_slab(N, HW, C, 4, 1).P)], groups, split=True, silu=(HW != 35), what=f"presplit C={C} HW={HW} N={N}")
    gn_chain(F32, 3, 35, [(C, 1)], groups, own_table=True, what=f"presplit, table maximum in entry 31, C={C}")
    if C == 96:
        gn_chain(F32, 3, 35, [(40, 2), (56, 1)], groups, split=True, film=True, what="presplit concat 40|56")


# ================================================================================================ coverage ledger
def _ledger():
    lib = _lib()
    return {
        lib.OP_GN_PARTIAL: "test_edge_group_norm_slab_and_channel_block_edges",
        lib.OP_GN_FINALIZE: "test_edge_group_norm_concat_seam_and_film",
        lib.OP_GN_APPLY: "test_edge_group_norm_written_presplit",
        lib.OP_TEMB: "test_edge_time_embed",
        lib.OP_TO_NHWC: "test_edge_nchw_to_nhwc",
        lib.OP_TO_NCHW: "test_edge_nhwc_to_nchw",
        lib.OP_POOL: "test_edge_resample_pool_and_sum",
        lib.OP_ACT_BOUND: "test_edge_act_bound_direct",
        lib.OP_BOUND_AFFINE: "test_edge_weight_l1max_and_bound_affine",
    }


def test_edge_every_glue_op_kind_of_a_program_is_pinned_here():
    """a new op kind in the inference program fails here until a test_edge_* of this module pins it"""
    from eo_diffusion_amd.backbones.unet_openai import UNetModel
    lib = _lib()
    elsewhere = {lib.OP_CONV, lib.OP_GEMM, lib.OP_ATTN, lib.OP_ATTN_NAT, lib.OP_SOFTMAX, lib.OP_DROPOUT, lib.OP_TRANSPOSE}
    ledger = _ledger()
    kinds = set()
    for prec in ("fp32", "fp16", "fp32x3"):
        u = UNetModel(32, 3, 32, 3, 1, [2], channel_mult=[1, 2], resblock_updown=True, use_scale_shift_norm=True, num_classes=4)
        u = u.set_precision(prec).to(DEV).eval()
        prog = u.program_for(2, 3, 0, 32, 32, torch.device(DEV), True)
        kinds |= {int(op.kind) for op in prog.ops}
        del prog, u
    assert kinds - elsewhere, "the program holds no glue op at all?"
    for k in sorted(kinds - elsewhere):
        assert k in ledger, f"op kind {k} of the inference program has no test_edge_* in tests/test_gpu_glue_ops.py"
        assert callable(globals().get(ledger[k])), ledger[k]
    for name in ledger.values():
        assert callable(globals().get(name)) and name.startswith("test_edge_"), name


# ================================================================================================ B. conditioning of the one-pass statistics
def _cond_input(r, N, HW, C, m, one_group):
    """x = m + noise per group (sigma = 1); one_group: only group 5 of image 1 carries the offset"""
    x = r.randn((N, HW, C))
    if one_group:
        x[1, :, 10:12] += m
    else:
        x += m
    return x


def _cond_checks(route, m, x, slots, slot_T, ss, y, gam, bet, what):
    """checks 2 and 3 (check 1 is the route's own): x [N][HW][C] the stored input, slots [N][P][C][2], ss [N][C][2], y [N][HW][C]"""
    N, HW, C = x.shape
    groups, cpg = 32, C // 32
    x = x.double()
    # check 2: the finalize against a float64 evaluation from ITS OWN slots: 4 u per entry, whatever kappa
    S = slots.double().sum(1).reshape(N, groups, cpg, 2).sum(2)
    cnt = HW * cpg
    mean = S[..., 0] / cnt
    var = (S[..., 1] / cnt - mean.square()).clamp_min(0.0)
    rstd = 1.0 / (var + EPS).sqrt()
    ch = lambda t: t[:, :, None].expand(N, groups, cpg).reshape(N, C)
    sc2 = ch(rstd) * gam.double()[None]
    sh2 = bet.double()[None] - ch(mean) * sc2
    e_sc = float(((ss[..., 0].double() - sc2).abs() / (4 * U * sc2.abs())).max())
    e_sh = float(((ss[..., 1].double() - sh2).abs() / (4 * U * (bet.double().abs()[None] + (ch(mean) * sc2).abs()))).max())
    _gate("cond_finalize", max(e_sc, e_sh), what)
    # check 3: end to end, rel-L2 per (image, group), against the ceiling derived from each group's own kappa
    y_ref = ref64.group_norm_forward(x, gam, bet, groups, EPS, silu_out=False)
    mu, rs = ref64.group_norm_stats(x, groups, EPS)
    mu, sig = mu.reshape(N, groups), (1.0 / rs.reshape(N, groups).square() - EPS).sqrt()
    kappa = 1.0 + (mu / sig).square()
    ceiling = COND_BASE + 0.5 * kappa * slot_T * U + (mu / sig).abs() * 2.0 ** -23
    d = (y.double() - y_ref).reshape(N, HW, groups, cpg)
    err = d.square().sum((1, 3)).sqrt() / y_ref.reshape(N, HW, groups, cpg).square().sum((1, 3)).sqrt()
    assert bool(torch.isfinite(err).all()), what
    assert bool((err < ceiling).all()), ("above the derived ceiling", what, float((err / ceiling).max()))
    gate, _measured = COND_GATE[(route, m)]
    worst = float(err.max())
    print(f"COND {route:8s} m/sigma {m:4d}  worst rel-L2 per (image, group) {worst:.3e}  gate {gate:.1e}  ceiling there {float(ceiling.flatten()[err.argmax()]):.2e}"
          f"  kappa max {float(kappa.max()):.1f}  {what}")
    WORST[f"cond_{route}_{m}"] = max(WORST[f"cond_{route}_{m}"], worst)
    assert worst < gate, (route, m, worst, gate, what)


@pytest.mark.parametrize("m", [0, 3, 10, 30, 100])
def test_edge_group_norm_conditioning_through_gn_partial(m):
    """section B, route 1: the slots of eod_gn_partial (fp32 storage) on x = m + noise, sigma = 1"""
    L, lib = _L(), _lib()
    N, C = 2, 64
    for side in (16, 32):
        for one_group in ((False, True) if m == 100 else (False,)):
            HW = side * side
            r = Rng(70 + side)
            x = _cond_input(r, N, HW, C, float(m), one_group)
            gam, bet = r.randn((C,), 0.2, shift=1.0), r.randn((C,), 0.1)
            P = max(1, min(256, HW // 64))      # (what Program.gn_stats asks for)
            per, ry = -(-HW // P), gn_slab(N, HW, C, 4, 1).ry
            T = per / ry + ry + 2
            part, ss, y = Out((N, P, C, 2)), Out((N, C, 2)), Out((N, HW, C))

            def launch():
                st = _st()
                _ok(L.eod_gn_partial(_p(x), lib.EOD_F32, N, HW, C, part.ptr, P, C, 0, st), "gn_partial")
                _ok(L.eod_gn_finalize(part.ptr, P, C, 0, 0, 0, N, HW, 32, EPS, _p(gam), _p(bet), 0, 0, ss.ptr, 0, 0, st), "gn_finalize")
                _ok(L.eod_gn_apply(_p(x), lib.EOD_F32, N, HW, C, ss.ptr, C, 0, 0, y.ptr, 0, st), "gn_apply")
            slots, g_ss, g_y = twice(launch, [part, ss, y])
            what = f"gn_partial {side}x{side} m/sigma={m} one_group={one_group}"
            ref, den = _slot_sums(x, P)   # check 1: every slot against the float64 sums over exactly its pixels
            _gate("cond_slots_partial", float(((slots.double() - ref).abs() / (T * U * den)).max()), what)
            _cond_checks("partial", m, x, slots, T, g_ss, g_y, gam, bet, what)


@pytest.mark.parametrize("m", [0, 3, 10, 30, 100])
def test_edge_group_norm_conditioning_through_conv_epilogue_statistics(m):
    """section B, route 2: a 3 x 3 conv (fp32 storage) whose epilogue emits the slots of the GroupNorm behind it; the offset sits in the
    conv's bias, so the stored y carries it"""
    from eo_diffusion_amd.engine import Act, Program
    N, C = 2, 64
    for side in (16, 32):
        for one_group in ((False, True) if m == 100 else (False,)):
            r = Rng(80 + side)
            xin = r.randn((N, side, side, C))
            w = r.randn((C, C, 3, 3), 1.0 / math.sqrt(9 * C))
            bias = torch.full((C,), 0.0 if one_group else float(m), device=DEV)
            cb = torch.zeros((N, C), device=DEV)   # (the per-sample bias carries the offset of the one group of image 1)
            cb[1, 10:12] = float(m)
            gam, bet = r.randn((C,), 0.2, shift=1.0), r.randn((C,), 0.1)
            prog = Program(DEV, "fp32")
            a = Act(prog.own(xin), N, side, side, C)
            ya, _ = prog.conv(a, prog.pack_conv(w), prog.f32(bias), C, stats=True, **(dict(cbias=prog.f32(cb), cbias_stride=C) if one_group else {}))
            assert ya.stats is not None, "the conv emits no statistics"
            ss = prog.gn_stats([ya], prog.f32(gam), prog.f32(bet), eps=EPS)
            yn = prog.gn_apply([ya], ss, silu=False)
            assert [int(op.kind) for op in prog.ops] == [_lib().OP_CONV, _lib().OP_GN_FINALIZE, _lib().OP_GN_APPLY], "a separate statistics pass ran"
            st_t, P = ya.stats
            runs = []
            for _ in range(2):
                for t in (ya.t, st_t, ss, yn.t):
                    t.fill_(NAN)
                prog.run()
                torch.cuda.synchronize()
                runs.append([t.clone() for t in (ya.t, st_t, ss, yn.t)])
            for u, v in zip(*runs):
                assert _same_bits(u, v), "two runs differ"
            y, slots, g_ss, g_y = runs[0]
            HW = side * side
            y, g_y = y.reshape(N, HW, C), g_y.reshape(N, HW, C)
            what = f"conv epilogue {side}x{side} slots={P} m/sigma={m} one_group={one_group}"
            # check 1: the slots, summed, against the float64 sums of the stored y.  A slot holds HW / P pixels; any summation order of n
            # terms is within (n - 1) u of the sum of |terms|: the ceiling with ry = 1
            T = HW / P + 3
            assert bool(torch.isfinite(slots).all()), what
            sref = ref64.stats_of(y)
            den = torch.stack([y.double().abs().sum(1), y.double().square().sum(1)], -1)
            _gate("cond_slots_conv", float(((slots.double().sum(1) - sref).abs() / (T * U * den)).max()), what)
            _cond_checks("conv", m, y, slots, T, g_ss, g_y, gam, bet, what)
