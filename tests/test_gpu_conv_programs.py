"""GPU: every conv launch of the real programs (eod_conv2d_igemm: conv3x3_halo_kernel, conv_up4_halo_kernel, conv_s2_halo_kernel,
conv_first_x3_kernel, conv_head_kernel and the generic igemm_kernel) against the float64 references of tests/ref64.py (themselves
tested against float64 F.conv2d / autograd in tests/test_ref64.py), on per-region metrics.

- harvested: the `harvest` fixture builds the inference programs of PROGRAMS and the trainers of test_gpu_train_kernels.TRAINERS one
  at a time, walks their descriptor lists (Program.ops, the ("op", ...) items of UNetTrainer.bwd: the backward-data convs) and keeps
  every distinct OP_CONV descriptor: every non-pointer field, the null / non-null state of every pointer, the alignment of x, x2, y.
  Each one is replayed through the C ABI at its harvested batch and size on fresh seeded tensors: weights packed by the library's own
  pack entry point for the form, y / statistics / workspace NaN-filled, y and statistics between two 4 KiB guard bands.  Kernel
  options that pick another kernel or schedule for the same descriptor are replayed as further arms against the same reference.
- hand-picked edges (test_edge_*): column and K tails, ragged maps, seams, uneven K slices.  Small; they also run under the electric
  fence (tests/test_gpu_efence.py).

Checks per launch: everything finite and the guard bands intact; rel-L2 of the whole tensor, of the worst output channel and of the
worst 8 x 16 pixel tile of any image; the worst element of |got - ref| / conv_abs_bound (fp16 storage: the output rounding
2^-11 |ref| is allowed on top); the statistics slots against float64 sums of the kernel's OWN stored y; two runs bit-identical.  A
whole-tensor rel-L2 dilutes a fault confined to one tile of 8192 by a factor of 90; the tile and element metrics see it at full size.

Operands: activations carry a per-channel scale and offset, GroupNorm tables scales of both signs, weights are 1 / sqrt(K) times a
power of two per output row (1/4 ... 4), the fused skip weight four times the 3x3 one.  fp16
operands are rounded first and the reference is built from the rounded values.  fp32x3: the last image of a batch is scaled by 2^10
and the second by 2^-10, every bound table's per-image maximum lies between 1x and 2x the true maximum of what the conv splits.

Gates.  One table keyed by (metric, arithmetic class): "fp32" exact products, "x3" split-fp16 products, "f16" fp16 storage, "f16gn"
fp16 storage with a fused GroupNorm (the normalised operand is rounded to fp16 inside the kernel), "ps" pre-split output.  Each gate
is at most about 4x the worst value measured on an MI355X over all harvested geometries and edges (the value in the comment next to
it) and never above its ceiling.  Ceilings come from the arithmetic: rel-L2 1e-5 for fp32 / fp32x3 (TOL), 6e-4 for fp16 storage
(twice the fp16 output rounding 2^-11 / sqrt(3)); statistics 1e-5; element metric (K + 4) 2^-24 for the fp32 accumulation of K
terms, + 3 * 2^-22 for the split product, + 2^-11 for a fused fp16 GroupNorm operand (checked per launch: elem_ceiling)."""
import collections
import contextlib
import ctypes
import gc
import math
import os

import pytest
import torch

from tests import ref64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
F64 = torch.float64

GATE = {
    # measured worst on an MI355X over the 709 harvested descriptors (1267 launches with the option arms) and the 52 edges, next to each gate
    # whole-tensor rel-L2: ceilings 1e-5 (fp32, x3, ps), 6e-4 (f16, f16gn: 4x measured would exceed it, so the gate is the ceiling)
    ("rel", "fp32"): 6.5e-6,    # 1.68e-6 (training forward, 1024 -> 512 at 32 x 32: K = 9216)
    ("rel", "x3"): 4.5e-6,      # 1.12e-6 (A0@256 b16, 512 + 512 -> 512 at 32 x 32, fused GroupNorm + skip)
    ("rel", "f16"): 6e-4,       # 2.10e-4 (the fp16 output rounding)
    ("rel", "f16gn"): 6e-4,     # 3.02e-4 (output rounding + the fp16 rounding of the normalised operand)
    ("rel", "ps"): 1e-6,        # 2.56e-7 (qkv 1x1, 512 -> 1536)
    # worst output channel
    ("chan", "fp32"): 8e-6,     # 1.98e-6
    ("chan", "x3"): 7e-6,       # 1.82e-6 (A0@64 b16, 512 + 512 -> 512 on the 8 x 8 map)
    ("chan", "f16"): 6e-4,      # 2.80e-4
    ("chan", "f16gn"): 6e-4,    # 3.49e-4
    ("chan", "ps"): 1.2e-6,     # 3.08e-7
    # worst 8 x 16 output tile of any image
    ("tile", "fp32"): 7e-6,     # 1.72e-6
    ("tile", "x3"): 4.5e-6,     # 1.15e-6
    ("tile", "f16"): 6e-4,      # 2.24e-4
    ("tile", "f16gn"): 6e-4,    # 3.14e-4
    ("tile", "ps"): 1e-6,       # 2.58e-7
    # worst element of |got - ref| / conv_abs_bound (fp16 storage: beyond 2^-11 |ref|); per-launch ceiling on top: elem_ceiling()
    ("elem", "fp32"): 3e-6,     # 7.27e-7 (A0@256 b16 fp32, 128 -> 128 at 256 x 256)
    ("elem", "x3"): 2.3e-6,     # 5.71e-7 (the same layer in fp32x3)
    ("elem", "f16"): 5.5e-7,    # 1.39e-7
    ("elem", "f16gn"): 4e-4,    # 9.86e-5 (the normalised operand is rounded to fp16 in the kernel: ceiling 2^-11 = 4.9e-4)
    ("elem", "ps"): 9e-7,       # 2.30e-7
    # statistics slots summed against float64 sums of the kernel's own stored y, worst image: ceiling 1e-5
    ("stats", "fp32"): 3.4e-7,  # 8.41e-8 (edge: the split-K reduce pass of a 1x1 conv over 288 channels; harvested 1.48e-8)
    ("stats", "x3"): 3.5e-7,    # 8.88e-8
    ("stats", "f16"): 4e-7,     # 1.06e-7
    ("stats", "f16gn"): 1e-7,   # 2.47e-8
}
WORST = collections.defaultdict(float)     # (metric, class) -> worst value seen in this session (printed with -s)
WORST_FAM = collections.defaultdict(float)  # (kernel family, metric, class)
VERBOSE = os.environ.get("EOD_TEST_CONV_VERBOSE", "0") == "1"


def elem_ceiling(K, cls):
    return (K + 4) * 2.0 ** -24 + (3 * 2.0 ** -22 if cls in ("x3", "ps") else 0.0) + (2.0 ** -11 if cls == "f16gn" else 0.0)


def _gate(metric, cls, err, what, fam, ceiling=None):
    WORST[(metric, cls)] = max(WORST[(metric, cls)], err)
    WORST_FAM[(fam, metric, cls)] = max(WORST_FAM[(fam, metric, cls)], err)
    if VERBOSE:
        print(f"GATE {metric:5s} {cls:5s} {err:.3e}  {what}")
    lim = GATE[(metric, cls)] if ceiling is None else min(GATE[(metric, cls)], ceiling)
    assert math.isfinite(err) and err < lim, (metric, cls, err, lim, what)


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


class Rng:
    def __init__(self, seed):
        self.g = torch.Generator(device=DEV)
        self.g.manual_seed(seed)

    def randn(self, shape, scale=1.0, shift=0.0):
        return torch.randn(shape, generator=self.g, device=DEV) * scale + shift

    def rand(self, shape, lo=0.0, hi=1.0):
        return torch.rand(shape, generator=self.g, device=DEV) * (hi - lo) + lo


# ================================================================================================ descriptors as plain dicts
def _fields():
    vp = ctypes.c_void_p
    f = _lib().ConvDesc._fields_
    return [n for n, t in f if t is not vp], [n for n, t in f if t is vp]


def desc_to_geom(d, kernel, src):
    """every non-pointer field, the null state of every pointer, the alignment of x / x2 / y: what a launch's behaviour can depend on"""
    vals, ptrs = _fields()
    g = {n: getattr(d, n) for n in vals}
    g["alpha"] = float(g["alpha"])
    g["nn"] = tuple(n for n in ptrs if getattr(d, n))
    g["mods"] = tuple((getattr(d, n) or 0) % 256 for n in ("x", "x2", "y"))
    g["kernel"], g["src"] = kernel, src
    return g


def geom_key(g):
    return repr(sorted((k, v) for k, v in g.items() if k not in ("src", "kernel")))


def _geom(dtype, N, H, W, C0, Cout, *, C1=0, ksize=3, stride=1, pad=1, upsample=0, pad_tl=0, alpha=1.0, w_split=0, w_tapmajor=0, bias=True,
          cbias=None, res=False, stats=False, gn=None, skip=None, a_bound=True, nchw=False, x_presplit=False, y_presplit=False, kernel="edge"):
    """a hand-picked descriptor in the same form (the statistics slot count and the workspace size are asked from the library)"""
    vals, _ = _fields()
    g = {n: 0 for n in vals}
    heff, weff = (H * (2 if upsample else 1) + pad_tl, W * (2 if upsample else 1) + pad_tl)
    Ho, Wo = (heff + 2 * pad - ksize) // stride + 1, (weff + 2 * pad - ksize) // stride + 1
    if upsample == 4:
        Ho, Wo = H // 2, W // 2
    g.update(dtype=dtype, N=N, H=H, W=W, C0=C0, C1=C1, Cout=Cout, ksize=ksize, stride=stride, pad=pad, upsample=upsample, pad_tl=pad_tl, Ho=Ho, Wo=Wo,
             out_nchw_f32=int(nchw), alpha=float(alpha), w_split=w_split, w_tapmajor=w_tapmajor, x_presplit=int(x_presplit),
             cbias_stride=0 if cbias is None else cbias, gn_silu=int(bool(gn and gn == "silu")), stats_slots=-1, workspace_bytes=-1)
    nn = ["x", "w", "y"] + (["x2"] if C1 else []) + (["bias"] if bias else []) + (["cbias"] if cbias is not None else []) + (["res"] if res else []) \
        + (["stats"] if stats else []) + (["gn_scale_shift"] if gn else []) + (["w_scale"] if w_split else []) \
        + (["a_bound"] if w_split and a_bound else []) + (["y_presplit_bound"] if y_presplit else [])
    if skip:
        g["skip_C0"], g["skip_C1"] = skip
        nn += ["skip_x", "skip_w"] + (["skip_x2"] if skip[1] else []) + (["skip_bound"] if w_split and a_bound else [])
    g["nn"], g["mods"], g["kernel"], g["src"] = tuple(nn), (0, 0, 0), kernel, "edge"
    return g


def kernel_family(d, prec):
    """the kernel name Program.op_stats() reports for this descriptor (the bench's per-op table uses the same names)"""
    from eo_diffusion_amd.engine import Program
    lib = _lib()
    prog = Program(DEV, prec)
    op = lib.Op()
    op.kind = lib.OP_CONV
    ctypes.memmove(ctypes.byref(op.u.conv), ctypes.byref(d), ctypes.sizeof(lib.ConvDesc))
    prog.ops = [op]
    return prog.op_stats()[0]["kernel"]


# ================================================================================================ buffers
GUARD = 4096
PATTERN = 0xA5


class Guarded:
    """`nbytes` of payload whose address is congruent to `mod` modulo 256, between two guard bands of at least 4 KiB of a fixed byte"""

    def __init__(self, nbytes, mod=0):
        self.buf = torch.full((GUARD + 256 + nbytes + GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
        self.off = GUARD + (mod - (self.buf.data_ptr() + GUARD)) % 256
        self.nbytes = nbytes
        assert (self.buf.data_ptr() + self.off) % 256 == mod and self.off % 4 == 0

    def view(self, dtype, shape):
        return self.buf[self.off:self.off + self.nbytes].view(dtype).reshape(shape)

    def intact(self):
        return bool((self.buf[:self.off] == PATTERN).all()) and bool((self.buf[self.off + self.nbytes:] == PATTERN).all())


def _aligned(t, mod):
    """a copy of t whose address is congruent to `mod` modulo 256"""
    if mod == 0 and t.data_ptr() % 256 == 0:
        return t.contiguous()
    g = Guarded(t.numel() * t.element_size(), mod)
    v = g.view(t.dtype, t.shape)
    v.copy_(t)
    v._keep = g
    return v


def bound_table(amax, seed):
    """[N][32] fp32 whose per-image maximum lies between 1x and 2x amax[n], smaller entries elsewhere"""
    N = amax.shape[0]
    r = Rng(seed)
    tab = r.rand((N, 32), 0.0, 0.5) * amax[:, None].float()
    f = 1.0 + ((torch.arange(N, device=DEV) * 0.37 + 0.11) % 0.99)
    tab[torch.arange(N, device=DEV), (torch.arange(N, device=DEV) * 7 + 3) % 32] = (amax.double() * f.double()).float()
    assert bool((tab.max(1).values.double() >= amax.double()).all())
    return tab.contiguous()


# ================================================================================================ metrics
def _tiles(sq):
    """[N][H][W] sums of squares -> [N][ceil(H/8)][ceil(W/16)] sums over 8 x 16 pixel blocks (ragged blocks at the edges)"""
    N, H, W = sq.shape
    sq = torch.nn.functional.pad(sq, (0, -W % 16, 0, -H % 8))
    return sq.reshape(N, sq.shape[1] // 8, 8, sq.shape[2] // 16, 16).sum((2, 4))


def metrics(got, ref, bound, f16_out):
    """got, ref, bound: NHWC float64 -> (whole rel-L2, worst channel, worst tile, worst element / bound, index of the worst tile)"""
    e = got - ref
    e2, r2 = e.square(), ref.square()
    rel = math.sqrt(float(e2.sum()) / max(float(r2.sum()), 1e-300))
    chan = float((e2.sum((0, 1, 2)) / r2.sum((0, 1, 2)).clamp_min(1e-300)).max().sqrt())
    t = _tiles(e2.sum(3)) / _tiles(r2.sum(3)).clamp_min(1e-300)
    tile = float(t.max().sqrt())
    where = tuple(int(v) for v in torch.unravel_index(t.argmax(), t.shape))
    ea = e.abs_()
    if f16_out:
        ea = (ea - ref.abs() * 2.0 ** -11).clamp_min_(0.0)
    elem = float((ea / bound.clamp_min(1e-300)).max())
    return rel, chan, tile, elem, where


# ================================================================================================ replay
OPTION_DEFAULT = {"head": 1, "first": 1, "s2_halo": 1, "halo_bn256": 1, "halo_splitk": 1, "head_tpw": 0}


@contextlib.contextmanager
def option(name, value):
    L = _L()
    if name is None:
        yield
        return
    assert L.eod_get_option(name.encode()) == OPTION_DEFAULT[name], f"option {name} is not at its default"
    prev = L.eod_set_option(name.encode(), value)
    try:
        yield
    finally:
        L.eod_set_option(name.encode(), prev)


def option_arms(g):
    """the non-default arms of the launch-time options that apply to this descriptor"""
    k = g["kernel"]
    arms = []
    if k == "conv_head_kernel":
        arms += [("head", 0), ("head_tpw", 1), ("head_tpw", 4)]
    if k == "conv_first_x3_kernel":
        arms += [("first", 0)]
    if k == "conv_s2_halo_kernel":
        arms += [("s2_halo", 0)]
    if k == "conv3x3_halo_kernel":
        if g["workspace_bytes"] > 0:
            arms += [("halo_splitk", 0)]
        else:
            if g["Cout"] >= 256 and g["Cout"] % 128 == 0:
                arms += [("halo_bn256", 0)]
    return arms


def _act(r, shape, f16, zero_from=None):
    C = shape[-1]
    x = r.randn(shape) * r.rand((C,), 0.5, 1.5) + r.rand((C,), -0.5, 0.5)
    if zero_from is not None:
        x[..., zero_from:] = 0
    return x.half() if f16 else x


def _image_scales(x, N, amount=10):
    if N >= 2:
        x[N - 1] *= 2.0 ** amount
    if N >= 3:
        x[1] *= 2.0 ** -amount


def _pack_weights(g, r, f16, td, dt):
    """-> (reference weight OIHW fp32, skip reference weight or None, dict of descriptor pointers, tensors to keep, K, extras).
    fp16 parity-class forms: the class kernels are sums of taps ROUNDED to fp16 by the pack, so extras["class_w"] carries the float64
    tap sums of the (rounded) weight, rounded to fp16 -- the operand the kernel gets; the reference is built from it like from every
    other rounded operand (ref64.conv_forward(class_w=...)), independently of eod_conv_up4_weights, which produced the packed one"""
    L, st, lib = _L(), _st(), _lib()
    C0, C1, Cout, ks, ups = g["C0"], g["C1"], g["Cout"], g["ksize"], g["upsample"]
    cin = C0 + C1
    K = (16 * C0 if ups == 4 else ks * ks * cin) + g["skip_C0"] + g["skip_C1"]
    def q(w, dim=0):
        """per output row a power of two between 1/4 and 4 (rows of different magnitude: the split weights' row exponents differ),
        then the storage rounding"""
        n = w.shape[dim]
        rs = torch.pow(2.0, ((3 * torch.arange(n, device=DEV)) % 5 - 2).float())
        w = w * rs.reshape([n if k == dim else 1 for k in range(w.dim())])
        return w.half().float() if f16 else w

    ptrs, keep = {}, []
    split = bool(g["w_split"])

    def scale_buf(rows):
        return torch.full((lib.WSCALE_ROWS + rows,), NAN, dtype=torch.float32, device=DEV)

    def pack(w, rows, cols, k):
        if split:
            dst, sc = torch.full((k * k, rows, cols), NAN, dtype=torch.float32, device=DEV), scale_buf(rows)
            _ok(L.eod_pack_conv_weight_split(_p(w), _p(dst), _p(sc), rows, cols, k, cols, st), "pack_conv_weight_split")
            ptrs["w_scale"] = sc
        else:
            dst = torch.full((k * k, rows, cols), NAN, dtype=td, device=DEV)
            _ok(L.eod_pack_conv_weight(_p(w), _p(dst), dt, rows, cols, k, cols, st), "pack_conv_weight")
        ptrs["w"] = dst

    sw = None
    if g["w_tapmajor"]:
        creal = {4: 3, 8: 7, 16: 13}.get(C0, C0 - 1)  # image channels in front of the zero padding of the 16-byte chunks
        w = q(r.randn((Cout, creal, 3, 3), 1.0 / math.sqrt(9 * creal))).contiguous()
        ldk = L.eod_conv_tapmajor_ldk(C0, dt)
        if split:
            dst, sc = torch.full((Cout, ldk), NAN, dtype=torch.float32, device=DEV), scale_buf(Cout)
            _ok(L.eod_pack_conv_weight_tapmajor_split(_p(w), _p(dst), _p(sc), Cout, creal, C0, st), "pack_conv_weight_tapmajor_split")
            ptrs["w_scale"] = sc
        else:
            dst = torch.full((Cout, ldk), NAN, dtype=td, device=DEV)
            _ok(L.eod_pack_conv_weight_tapmajor(_p(w), _p(dst), dt, Cout, creal, C0, st), "pack_conv_weight_tapmajor")
        ptrs["w"] = dst
        wref = torch.nn.functional.pad(w, (0, 0, 0, 0, 0, C0 - creal))
        keep.append(w)
        return wref, None, ptrs, keep, K, dict(creal=creal)
    if ups == 3:  # the parity-class form: the [4 Cout][Cin][3][3] class-kernel tensor, packed like any weight
        w = q(r.randn((Cout, C0, 3, 3), 1.0 / math.sqrt(9 * C0))).contiguous()
        wc = torch.full((4 * Cout, C0, 3, 3), NAN, dtype=torch.float32, device=DEV)
        _ok(L.eod_conv_up4_weights(_p(w), _p(wc), Cout, C0, st), "conv_up4_weights")
        pack(wc, 4 * Cout, C0, 3)
        keep += [w, wc]
        return w, None, ptrs, keep, K, dict(class_w=ref64.up4_class_kernels(w).half() if f16 else None)
    if ups == 4:  # backward-data of that form: w is the FORWARD weight [C0 = dY channels][Cout = dX channels][3][3]
        w = q(r.randn((C0, Cout, 3, 3), 1.0 / math.sqrt(9 * C0)), dim=1).contiguous()
        wc = torch.full((4 * C0, Cout, 3, 3), NAN, dtype=torch.float32, device=DEV)
        _ok(L.eod_conv_up4_weights(_p(w), _p(wc), C0, Cout, st), "conv_up4_weights")
        wd = wc.flip(2, 3).transpose(0, 1).contiguous()  # the conv dY -> dX over the class-kernel tensor: [Cout][4 C0][3][3]
        pack(wd, Cout, 4 * C0, 3)
        keep += [w, wc, wd]
        return w, None, ptrs, keep, K, dict(class_w=ref64.up4_class_kernels(w).half() if f16 else None)
    w = q(r.randn((Cout, cin, ks, ks), 1.0 / math.sqrt(ks * ks * cin))).contiguous()
    keep.append(w)
    if "skip_x" in g["nn"]:
        sc_ = g["skip_C0"] + g["skip_C1"]
        sw = q(r.randn((Cout, sc_, 1, 1), 4.0 / math.sqrt(ks * ks * cin))).contiguous()  # several times the 3x3 weight: the shared split scale
        keep.append(sw)
        if split:
            dst = torch.full((ks * ks, Cout, cin), NAN, dtype=torch.float32, device=DEV)
            dst2 = torch.full((1, Cout, sc_), NAN, dtype=torch.float32, device=DEV)
            sc = scale_buf(Cout)
            _ok(L.eod_pack_conv_weight_split_pair(_p(w), _p(dst), _p(sw), _p(dst2), _p(sc), Cout, cin, ks, cin, sc_, st), "pack_conv_weight_split_pair")
            ptrs.update(w=dst, skip_w=dst2, w_scale=sc)
        else:
            pack(w, Cout, cin, ks)
            dst2 = torch.full((1, Cout, sc_), NAN, dtype=td, device=DEV)
            _ok(L.eod_pack_conv_weight(_p(sw), _p(dst2), dt, Cout, sc_, 1, sc_, st), "pack_conv_weight")
            ptrs["skip_w"] = dst2
    else:
        pack(w, Cout, cin, ks)
    return w, sw, ptrs, keep, K, {}


def _reference(g, x, x2, w, ss, bias, cbias, res, sx, sx2, sw, class_w=None):
    """(ref, abs bound) NHWC float64 on the GPU, in chunks of images"""
    N, Ho, Wo, Cout = g["N"], g["Ho"], g["Wo"], g["Cout"]
    ups = g["upsample"]
    per = 8 * max(g["H"] * g["W"] * (g["C0"] + g["C1"]) * (4 if ups in (1, 2, 3) else 1), Ho * Wo * Cout, 1)
    step = max(1, min(N, (1 << 29) // per))
    ref = torch.empty((N, Ho, Wo, Cout), dtype=F64, device=DEV)
    bnd = torch.empty_like(ref)
    for n0 in range(0, N, step):
        n1 = min(N, n0 + step)
        kw = dict(ksize=g["ksize"], stride=g["stride"], pad=g["pad"], upsample=ups, pad_tl=g["pad_tl"], alpha=g["alpha"], bias=bias,
                  gn_scale_shift=None if ss is None else ss[n0:n1], gn_silu=bool(g["gn_silu"]),
                  cbias=None if cbias is None else cbias.flatten()[n0 * g["cbias_stride"]:], cbias_stride=g["cbias_stride"],
                  res=None if res is None else res[n0:n1], skip_x=None if sx is None else sx[n0:n1],
                  skip_x2=None if sx2 is None else sx2[n0:n1], skip_w=sw, class_w=class_w)
        xa, xb = x[n0:n1], (None if x2 is None else x2[n0:n1])
        ref[n0:n1] = ref64.conv_forward(xa, xb, w, **kw)
        bnd[n0:n1] = ref64.conv_abs_bound(xa, xb, w, **kw)
    return ref, bnd


def _amax_input(g, x, x2, ss):
    """per-image maximum of |A| as the conv splits it (behind the fused GroupNorm + SiLU), float64 [N]"""
    out = []
    for n in range(g["N"]):
        a = ref64.conv_input(x[n:n + 1], None if x2 is None else x2[n:n + 1], gn_scale_shift=None if ss is None else ss[n:n + 1],
                             gn_silu=bool(g["gn_silu"]))
        out.append(a.abs().max())
    return torch.stack(out)


def replay(g, seed, arms=True, harvested=True):
    """one descriptor: fresh operands, float64 reference (once), then the default arm and every applicable option arm"""
    L, st, lib = _L(), _st(), _lib()
    r = Rng(seed)
    nn = set(g["nn"])
    f16 = g["dtype"] == lib.EOD_F16
    td, dt = (torch.float16, lib.EOD_F16) if f16 else (torch.float32, lib.EOD_F32)
    split = bool(g["w_split"])
    gn = "gn_scale_shift" in nn
    ps_out = "y_presplit_bound" in nn
    cls = "ps" if ps_out else "x3" if split else ("f16gn" if gn else "f16") if f16 else "fp32"
    N, H, W, C0, C1, Cout, Ho, Wo = (g[k] for k in ("N", "H", "W", "C0", "C1", "Cout", "Ho", "Wo"))
    fam = g["kernel"]
    what = f"{fam} [{g['src']}] " + " ".join(f"{k}={g[k]}" for k in ("N", "H", "W", "C0", "C1", "Cout", "ksize", "stride", "upsample", "pad_tl")) \
        + f" {cls} nn={sorted(nn - {'x', 'w', 'y'})} ws={g['workspace_bytes']} slots={g['stats_slots']}"

    w, sw, wp, keep, K, extra = _pack_weights(g, r, f16, td, dt)
    creal = extra.get("creal")
    x = _act(r, (N, H, W, C0), f16, zero_from=creal)
    x2 = _act(r, (N, H, W, C1), f16) if C1 else None
    scaled = split and "a_bound" in nn
    if scaled:
        _image_scales(x, N)
        if x2 is not None:
            _image_scales(x2, N)
    ss = torch.stack([r.randn((N, C0 + C1), 0.8), r.randn((N, C0 + C1), 0.3)], -1).contiguous() if gn else None
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
    ab = None
    if "a_bound" in nn:
        ab = bound_table(_amax_input(g, x, x2, ss), seed + 1)
        ptr["a_bound"] = ab
    if "skip_bound" in nn:
        cat = sx if sx2 is None else torch.cat([sx, sx2], -1)
        ptr["skip_bound"] = bound_table(cat.abs().amax((1, 2, 3)).double(), seed + 2)
    xin, x2in = x, x2
    if g["x_presplit"]:  # the producer wrote [8 x hi | 8 x lo] of s_n x; the reference sees what those pairs represent
        s = ref64.presplit_scale(ab)
        xin, x = ref64.presplit_encode(x, s), ref64.presplit_decode(ref64.presplit_encode(x, s), s)
        if x2 is not None:
            x2in, x2 = ref64.presplit_encode(x2, s), ref64.presplit_decode(ref64.presplit_encode(x2, s), s)
    ref, bnd = _reference(g, x, x2, w, ss, bias, cbias, res, sx, sx2, sw, extra.get("class_w"))
    ps_scale = None
    if ps_out:
        ptr["y_presplit_bound"] = bound_table(ref.abs().amax((1, 2, 3)), seed + 3)
        ps_scale = ref64.presplit_scale(ptr["y_presplit_bound"], kmin=ref64.AB_KMIN_ATTN)
    ptr["x"], ptr["x2"] = _aligned(xin, g["mods"][0]), (None if x2in is None else _aligned(x2in, g["mods"][1]))
    ptr.update(bias=bias, cbias=cbias, res=res, gn_scale_shift=ss, skip_x=sx, skip_x2=sx2)
    nchw = bool(g["out_nchw_f32"])
    ydt = torch.float32 if (nchw or not f16) else torch.float16
    yshape = (N, Cout, Ho, Wo) if nchw else (N, Ho, Wo, Cout)
    yg = Guarded(N * Ho * Wo * Cout * (4 if ydt == torch.float32 else 2), g["mods"][2])
    y = yg.view(ydt, yshape)
    vals, ptrs_all = _fields()
    launches = 0
    for name, value in [(None, None)] + (option_arms(g) if arms else []):
        with option(name, value):
            d = lib.ConvDesc()
            for k in vals:
                setattr(d, k, g[k])
            d.workspace_bytes, d.stats_slots = 0, 0
            for k in ptrs_all:
                if k in nn and k not in ("y", "stats", "workspace"):
                    assert ptr.get(k) is not None, (k, what)
                    setattr(d, k, ptr[k].data_ptr())
            d.y = y.data_ptr()
            ws_bytes = L.eod_conv_workspace_size(ctypes.byref(d))
            slots = L.eod_conv_stats_slots(ctypes.byref(d)) if "stats" in nn else 0
            if name is None and harvested:  # the library gives today what the program was built with
                assert ws_bytes == g["workspace_bytes"], (ws_bytes, what)
                assert slots == g["stats_slots"], (slots, what)
            if name is None and "stats" in nn:
                assert slots > 0, what
            ws = torch.full((ws_bytes // 4,), NAN, dtype=torch.float32, device=DEV) if ws_bytes else None
            d.workspace, d.workspace_bytes = _p(ws), ws_bytes
            sg = stats = None
            if slots > 0:
                sg = Guarded(N * slots * Cout * 2 * 4)
                stats = sg.view(torch.float32, (N, slots, Cout, 2))
                d.stats, d.stats_slots = stats.data_ptr(), slots
            runs = []
            for _ in range(2):
                y.fill_(NAN)
                if stats is not None:
                    stats.fill_(NAN)
                if ws is not None:
                    ws.fill_(NAN)
                _ok(L.eod_conv2d_igemm(ctypes.byref(d), st), "conv2d_igemm " + what)
                torch.cuda.synchronize()
                runs.append((y.clone(), None if stats is None else stats.clone()))
        arm = what + (f" {name}={value}" if name else "")
        it = torch.int32 if ydt == torch.float32 else torch.int16
        # 8. two runs bit-identical
        assert torch.equal(runs[0][0].view(it), runs[1][0].view(it)), "y differs between two runs: " + arm
        assert stats is None or torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32)), "statistics differ between two runs: " + arm
        # 1. finite, guard bands intact
        assert yg.intact() and (sg is None or sg.intact()), "guard band overwritten: " + arm
        if ps_out:
            got = ref64.presplit_decode(y, ps_scale)
        else:
            got = (y.permute(0, 2, 3, 1) if nchw else y).to(F64)
        assert bool(torch.isfinite(got).all()), f"{int((~torch.isfinite(got)).sum())} non-finite outputs: " + arm
        # 2. - 5. (7.: the same on the decoded pre-split output)
        rel, chan, tile, elem, where = metrics(got, ref, bnd, ydt == torch.float16)
        del got
        serr = None
        if stats is not None:  # 6. the slots against the sums of the stored y
            assert bool(torch.isfinite(stats).all()), "non-finite statistics slot: " + arm
            s_ref = ref64.stats_of(y)
            s_got = stats.to(F64).sum(1)
            serr = float(((s_got - s_ref).flatten(1).norm(dim=1) / s_ref.flatten(1).norm(dim=1).clamp_min(1e-300)).max())
        print(f"CONV {cls:5s} rel {rel:.2e} chan {chan:.2e} tile {tile:.2e} elem {elem:.2e} stats {-1.0 if serr is None else serr:.2e}  {arm}")
        _gate("rel", cls, rel, arm, fam)
        _gate("chan", cls, chan, arm, fam)
        _gate("tile", cls, tile, f"{arm} worst tile (image, tile row, tile column) = {where}", fam)
        _gate("elem", cls, elem, arm, fam, ceiling=elem_ceiling(K, cls))
        if serr is not None:
            _gate("stats", cls, serr, arm, fam)
        launches += 1
        del ws, stats, sg, runs
    return launches


# ================================================================================================ harvest from the real programs
A0 = dict(model_channels=128, channel_mult=[1, 2, 3, 4], attention_resolutions=[], num_res_blocks=1, num_heads=1)
A1 = dict(model_channels=128, channel_mult=[1, 2, 3, 4], attention_resolutions=[4, 8], num_res_blocks=2, num_heads=8)
SMALL = dict(model_channels=64, channel_mult=[1, 2, 3], attention_resolutions=[], num_res_blocks=1, num_heads=1, use_scale_shift_norm=True,
             resblock_updown=True, num_classes=10)
PROGRAMS = [  # label, arch, (H, W), image channels, batch, precision, options switched off while the program is built
    ("A0@256 b16 fp32x3", A0, (256, 256), 3, 16, "fp32x3", ()),     # the headline benchmark
    ("A0@256 b16 fp16", A0, (256, 256), 3, 16, "fp16", ()),
    ("A0@256 b16 fp32", A0, (256, 256), 3, 16, "fp32", ()),
    ("A0@64 b16 fp32x3", A0, (64, 64), 3, 16, "fp32x3", ()),        # split-K and 8-wide maps
    ("A0@64 b16 fp16", A0, (64, 64), 3, 16, "fp16", ()),
    ("A1@256 b1 fp32x3", A1, (256, 256), 3, 1, "fp32x3", ()),       # qkv / proj_out 1x1 with pre-split input and output
    ("A1@256 b1 fp16", A1, (256, 256), 3, 1, "fp16", ()),
    ("A1@512x13 b1 fp16", A1, (512, 512), 13, 1, "fp16", ()),       # tap-major first conv with 16 padded channels
    ("small film+updown+classes 40x56 b3 fp32x3", SMALL, (40, 56), 3, 3, "fp32x3", ()),   # ragged maps, generic kernel with split-K
    ("small film+updown+classes 40x56 b3 fp16", SMALL, (40, 56), 3, 3, "fp16", ()),
    ("A0@64 b16 fp32x3 skip_fuse=0", A0, (64, 64), 3, 16, "fp32x3", ("skip_fuse",)),
    ("A0@64 b16 fp32x3 gn_fuse_max_cout=0", A0, (64, 64), 3, 16, "fp32x3", ("gn_fuse_max_cout",)),
    ("A0@64 b16 fp32x3 EOD_UP4=0", A0, (64, 64), 3, 16, "fp32x3", ("EOD_UP4",)),
]


def _free():
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def harvest():
    from eo_diffusion_amd.backbones.unet_openai import UNetModel
    from eo_diffusion_amd.training import UNetTrainer
    from tests.test_gpu_train_kernels import TRAINERS
    lib, L = _lib(), _L()
    pool, keys = [], set()

    def take(ops, stats, label):
        for op, s in zip(ops, stats):
            if op.kind != lib.OP_CONV:
                continue
            g = desc_to_geom(op.u.conv, s["kernel"], label)
            k = geom_key(g)
            if k not in keys:
                keys.add(k)
                pool.append(g)

    for label, arch, (H, W), ch, N, prec, off in PROGRAMS:
        prev, env = {}, os.environ.get("EOD_UP4")
        try:
            for o in off:
                if o == "EOD_UP4":
                    os.environ["EOD_UP4"] = "0"
                else:
                    prev[o] = L.eod_set_option(o.encode(), 0)
            unet = UNetModel(max(H, W), in_channels=ch, out_channels=ch, **arch).set_precision(prec).to(DEV).eval()
            prog = unet.program_for(N, ch, 0, H, W, torch.device(DEV), arch.get("num_classes") is not None)
            take(prog.ops, prog.op_stats(), label)
        finally:
            for o, v in prev.items():
                L.eod_set_option(o.encode(), v)
            if "EOD_UP4" in off:
                os.environ.pop("EOD_UP4") if env is None else os.environ.__setitem__("EOD_UP4", env)
        del prog, unet
        _free()
    for label, arch, size, ch, N, prec, extra in TRAINERS:
        unet = UNetModel(size, in_channels=ch, out_channels=ch, **arch, **extra).set_precision(prec).to(DEV).train()
        tr = UNetTrainer(unet, N, size, size, DEV, loss_scale=(1024.0 if prec == "fp16" else 1.0))
        take(tr.prog.ops, tr.prog.op_stats(), "train fwd " + label)
        bstats = {id(op): s for op, s in zip(tr.bprog.ops, tr.bprog.op_stats())}
        bops = [item[1] for item in tr.bwd if item[0] == "op" and item[1].kind == lib.OP_CONV]
        take(bops, [bstats[id(op)] for op in bops], "train bwd-data " + label)
        del tr, unet, bstats, bops
        _free()
    fams = collections.Counter(g["kernel"] for g in pool)
    for k, n in sorted(fams.items()):
        print(f"harvest: {k:28s} {n:4d} distinct descriptors")
    print(f"harvest: {len(pool)} distinct conv descriptors")
    return pool


FAMILIES = ["conv3x3_halo_kernel", "conv_up4_halo_kernel", "conv_s2_halo_kernel", "conv_first_x3_kernel", "conv_head_kernel",
            "conv3x3_halo_kernel<BN=32>", "igemm_kernel"]
STATS_FAMILIES = ["conv3x3_halo_kernel", "conv_up4_halo_kernel", "conv_s2_halo_kernel", "conv_first_x3_kernel", "igemm_kernel"]


def test_harvest_is_complete(harvest):
    """the real programs reach every kernel family and every descriptor form the replay below relies on: a program change that moves
    work to another kernel fails here instead of leaving a check that checks nothing"""
    lib = _lib()
    H = harvest

    def some(pred, what):
        assert any(pred(g) for g in H), "no harvested conv launch with: " + what

    for fam in FAMILIES:
        some(lambda g: g["kernel"] == fam, f"kernel {fam}")
    assert {g["kernel"] for g in H} <= set(FAMILIES), "a kernel name this module does not know"
    for u in (0, 2, 3, 4):
        some(lambda g: g["upsample"] == u, f"upsample {u}")
    some(lambda g: g["stride"] == 2 and g["kernel"] == "conv_s2_halo_kernel", "stride 2 on the halo form")
    some(lambda g: g["stride"] == 2 and g["kernel"] == "igemm_kernel", "stride 2 on the generic form")
    some(lambda g: g["workspace_bytes"] > 0 and g["kernel"] == "conv3x3_halo_kernel", "split-K on the halo kernel")
    some(lambda g: g["workspace_bytes"] > 0 and g["kernel"] == "igemm_kernel", "split-K on the generic kernel")
    some(lambda g: "skip_x" in g["nn"] and "skip_x2" in g["nn"], "fused skip over two sources")
    some(lambda g: "skip_x" in g["nn"] and "skip_x2" not in g["nn"], "fused skip over one source")
    some(lambda g: "x2" in g["nn"] and "gn_scale_shift" in g["nn"], "virtual concat with a fused GroupNorm")
    some(lambda g: "res" in g["nn"], "res")
    some(lambda g: "cbias" in g["nn"] and g["cbias_stride"] == 0, "cbias with stride 0")
    some(lambda g: "cbias" in g["nn"] and g["cbias_stride"] > 0, "cbias with a non-zero stride")
    for fam in STATS_FAMILIES:
        some(lambda g: g["kernel"] == fam and "stats" in g["nn"], f"statistics written by {fam}")
    some(lambda g: g["workspace_bytes"] > 0 and "stats" in g["nn"], "statistics written by the split-K reduce pass")
    some(lambda g: g["x_presplit"], "x_presplit")
    some(lambda g: "y_presplit_bound" in g["nn"], "y_presplit_bound")
    some(lambda g: g["out_nchw_f32"], "out_nchw_f32")
    some(lambda g: g["w_tapmajor"] and g["w_split"], "w_tapmajor with w_split")
    some(lambda g: g["w_tapmajor"] and not g["w_split"], "w_tapmajor without w_split")
    some(lambda g: g["w_tapmajor"] and g["C0"] == 16, "tap-major first conv with 16 padded channels")
    for c in (128, 256, 384, 512):
        some(lambda g: g["Cout"] == c, f"Cout {c}")
    some(lambda g: g["Cout"] % 128 != 0 and g["Cout"] > 64, "a wide Cout that is not a multiple of 128")
    some(lambda g: g["dtype"] == lib.EOD_F16, "fp16")
    some(lambda g: g["dtype"] == lib.EOD_F32 and g["w_split"], "fp32x3")
    some(lambda g: g["dtype"] == lib.EOD_F32 and not g["w_split"] and g["kernel"] == "conv3x3_halo_kernel", "exact fp32 on the halo kernel")
    some(lambda g: g["N"] == 16 and g["Ho"] == 256 and g["Cout"] == 128 and g["C0"] + g["C1"] == 384, "the widest 256 x 256 layer at batch 16")


def _report(fam, n, launches):
    print(f"{fam}: {n} descriptors, {launches} launches; worst " + ", ".join(
        f"{m}/{c} {v:.2e}" for (f, m, c), v in sorted(WORST_FAM.items()) if f == fam))


@pytest.mark.parametrize("fam", FAMILIES)
def test_harvested_geometries(harvest, fam):
    todo = [(i, g) for i, g in enumerate(harvest) if g["kernel"] == fam]
    assert todo, fam
    done = launches = 0
    for i, g in todo:
        launches += replay(g, seed=5000 + i)
        done += 1
        _free()
    assert done == len(todo), "a harvested launch was skipped"
    _report(fam, done, launches)
    print("worst per gate so far: " + ", ".join(f"{m}/{c} {v:.2e} (gate {GATE[(m, c)]:.1e})" for (m, c), v in sorted(WORST.items())))


# ================================================================================================ the backward-data weight packing
@pytest.mark.parametrize("f16", [True, False], ids=["f16", "f32"])
@pytest.mark.parametrize("Cout,Cin,ks,ci0,nci,cout_pad", [(24, 16, 3, 0, 16, 24), (24, 40, 3, 8, 24, 32), (40, 24, 1, 16, 8, 40), (20, 8, 3, 0, 8, 32),
                                                         (136, 264, 1, 0, 264, 136)])
def test_pack_dgrad_is_the_forward_pack_of_the_flipped_transposed_weight(f16, Cout, Cin, ks, ci0, nci, cout_pad):
    """eod_pack_conv_weight_dgrad (the weights of every backward-data conv) bit for bit: [taps-1-tap][ci - ci0][cout_pad] is
    eod_pack_conv_weight of W'[ci - ci0][co][ky][kx] = W[co][ci][ks-1-ky][ks-1-kx], zero padded to cout_pad"""
    L, st, lib = _L(), _st(), _lib()
    td, dt = (torch.float16, lib.EOD_F16) if f16 else (torch.float32, lib.EOD_F32)
    w = Rng(31).randn((Cout, Cin, ks, ks)).contiguous()
    a = torch.full((ks * ks, nci, cout_pad), NAN, dtype=td, device=DEV)
    b = torch.full_like(a, NAN)
    _ok(L.eod_pack_conv_weight_dgrad(_p(w), _p(a), dt, Cout, Cin, ks, ci0, nci, cout_pad, st), "pack_conv_weight_dgrad")
    wt = w[:, ci0:ci0 + nci].flip(2, 3).transpose(0, 1).contiguous()
    _ok(L.eod_pack_conv_weight(_p(wt), _p(b), dt, nci, Cout, ks, cout_pad, st), "pack_conv_weight")
    torch.cuda.synchronize()
    it = torch.int16 if f16 else torch.int32
    assert torch.equal(a.view(it), b.view(it))
    assert torch.equal(a[:, :, :Cout].float(), wt.to(td).float().permute(2, 3, 0, 1).reshape(ks * ks, nci, Cout))
    assert bool((a[:, :, Cout:] == 0).all())


def test_pack_dgrad_of_the_class_kernel_tensor_is_the_upsample4_weight():
    """upsample = 4: w = eod_pack_conv_weight_dgrad (cout_pad = 4 C0) of the class-kernel tensor of eod_conv_up4_weights, which is what
    the replay packs through eod_pack_conv_weight from the flipped, transposed class kernels"""
    L, st, lib = _L(), _st(), _lib()
    Cf_out, Cf_in = 72, 80  # forward conv Cf_in -> Cf_out: dY has Cf_out channels, dX Cf_in
    w = Rng(32).randn((Cf_out, Cf_in, 3, 3)).contiguous()
    wc = torch.full((4 * Cf_out, Cf_in, 3, 3), NAN, dtype=torch.float32, device=DEV)
    _ok(L.eod_conv_up4_weights(_p(w), _p(wc), Cf_out, Cf_in, st), "conv_up4_weights")
    a = torch.full((9, Cf_in, 4 * Cf_out), NAN, dtype=torch.float16, device=DEV)
    b = torch.full_like(a, NAN)
    _ok(L.eod_pack_conv_weight_dgrad(_p(wc), _p(a), lib.EOD_F16, 4 * Cf_out, Cf_in, 3, 0, Cf_in, 4 * Cf_out, st), "pack_conv_weight_dgrad")
    wd = wc.flip(2, 3).transpose(0, 1).contiguous()
    _ok(L.eod_pack_conv_weight(_p(wd), _p(b), lib.EOD_F16, Cf_in, 4 * Cf_out, 3, 4 * Cf_out, st), "pack_conv_weight")
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    # the class kernels themselves: class (p, q) sums the rows / columns of w that meet the same stored pixel
    w64 = w.double()
    rows = {0: [[0], [1, 2]], 1: [[0, 1], [2]]}
    for p in (0, 1):
        for q in (0, 1):
            blk = wc[(2 * p + q) * Cf_out:(2 * p + q + 1) * Cf_out].double()
            want = torch.zeros_like(blk)
            for a_, rs in enumerate(rows[p]):
                for b_, cs in enumerate(rows[q]):
                    want[:, :, p + a_, q + b_] = w64[:, :, rs][:, :, :, cs].sum((2, 3))
            assert float((blk - want).abs().max()) < 1e-6, (p, q)


# ================================================================================================ hand-picked edges
def _edges():
    lib = _lib()
    F32, F16 = lib.EOD_F32, lib.EOD_F16
    E = []
    for dt, sp in ((F32, 1), (F16, 0), (F32, 0)):
        # column tails on the 128- and 64-column halo instances (Cout 136 / 200), plain / fused GroupNorm / fused skip over 40 + 24
        E += [_geom(dt, 1, 32, 32, 64, 136, w_split=sp, stats=True, cbias=0),
              _geom(dt, 3, 32, 32, 64, 200, w_split=sp, gn="silu", stats=True, cbias=208),
              _geom(dt, 1, 16, 16, 64, 136, w_split=sp, gn="plain", res=True),
              _geom(dt, 3, 16, 16, 64, 200, w_split=sp, stats=True, alpha=0.75)]
        if dt == F16 or sp:
            E += [_geom(dt, 2, 32, 32, 64, 136, w_split=sp, skip=(40, 24), gn="silu", stats=True, cbias=0),
                  _geom(dt, 3, 16, 16, 64, 200, w_split=sp, skip=(40, 0), stats=True),
                  _geom(dt, 1, 16, 32, 24, 72, w_split=sp, upsample=3, stats=True),                  # parity-class form, one K chunk, Cout 72
                  _geom(dt, 1, 63, 63, 16, 136, w_split=sp, stride=2, stats=True)]                   # stride 2 on an odd map, halo form
        # K tails (C0 96 and 264: 8-channel granularity), two-source concat with a fused GroupNorm across the seam
        E += [_geom(dt, 1, 8, 16, 96, 128, w_split=sp, stats=True),                                 # one tile per image, N = 1
              _geom(dt, 3, 8, 16, 264, 128, w_split=sp, gn="silu"),                                 # one tile per image, N = 3
              _geom(dt, 2, 16, 16, 40, 72, C1=24, w_split=sp, gn="silu", stats=True),
              _geom(dt, 3, 8, 8, 96, 136, w_split=sp, stats=True, res=True),                        # 8-wide map
              # K slices that do not divide the chunk count (7 chunks in 3 slices), halo kernel + reduce pass with statistics
              _geom(dt, 3, 16, 16, 448 if dt == F16 else 224, 128, w_split=sp, stats=True, cbias=136, res=True),
              # the generic kernel: 1x1 over 9 chunks in 2 slices, stride 2 on odd maps (ragged output), the 3 x 3 -> 7 x 7 form
              _geom(dt, 3, 8, 8, 576 if dt == F16 else 288, 72, ksize=1, pad=0, w_split=sp, stats=True, alpha=-1.5),
              _geom(dt, 3, 15, 15, 96, 136, stride=2, w_split=sp, cbias=0),
              _geom(dt, 1, 31, 33, 24, 40, stride=2, w_split=sp, res=True),
              _geom(dt, 2, 3, 3, 24, 40, upsample=1, pad_tl=1, w_split=sp)]
    E += [_geom(F32, 3, 16, 32, 264, 136, ksize=1, pad=0, w_split=1, x_presplit=True),               # pre-split input with a K tail
          _geom(F32, 3, 16, 16, 96, 200, ksize=1, pad=0, w_split=1, y_presplit=True),                # pre-split output with a column tail
          _geom(F32, 2, 16, 16, 64, 136, w_split=1, a_bound=False, stats=True),                      # no bound table: the fixed operand scale
          _geom(F16, 2, 16, 16, 136, 72, upsample=2, bias=False, res=True),                          # zero insertion (four parity-class launches)
          _geom(F16, 3, 16, 32, 136, 72, upsample=4, bias=False, res=True)]                          # backward-data of the parity-class form
    return E


def _edge_id(g):
    return "dt{dtype}_x{w_split}_N{N}_{H}x{W}_c{C0}+{C1}_co{Cout}_k{ksize}s{stride}u{upsample}".format(**g) + "".join(
        "_" + n for n in ("gn_scale_shift", "skip_x", "skip_x2", "res", "stats", "cbias") if n in g["nn"]) \
        + ("_psin" if g["x_presplit"] else "") + ("_psout" if "y_presplit_bound" in g["nn"] else "") + ("_tl" if g["pad_tl"] else "") \
        + (f"_a{g['alpha']}" if g["alpha"] != 1.0 else "")


def pytest_generate_tests(metafunc):
    if "edge" in metafunc.fixturenames:
        E = _edges()
        metafunc.parametrize("edge", E, ids=[_edge_id(g) for g in E])


def test_edge_conv_launch(edge):
    lib, L = _lib(), _L()
    g = dict(edge)
    # the kernel family of the edge (for the option arms and the report), from a descriptor with the pointer states of the edge
    d = lib.ConvDesc()
    vals, _ = _fields()
    for k in vals:
        setattr(d, k, g[k])
    d.workspace_bytes = d.stats_slots = 0
    for k in g["nn"]:
        setattr(d, k, 16)
    g["workspace_bytes"] = L.eod_conv_workspace_size(ctypes.byref(d))
    d.workspace = 16 if g["workspace_bytes"] else 0
    prec = "fp16" if g["dtype"] == lib.EOD_F16 else "fp32x3" if g["w_split"] else "fp32"
    g["kernel"] = kernel_family(d, prec)
    assert replay(g, seed=77, harvested=False) >= 1
