"""GPU: the training backward kernels of csrc/train.hip against the float64 references of tests/ref64.py (themselves tested against
torch autograd in tests/test_ref64.py).

Two sources of geometries feed the same check helpers:
- harvested: the `harvest` fixture builds real UNetTrainers (the training-benchmark shape, the config-5 shape, the exact-fp32 GEMM
  path and a small FiLM / class-conditional net), reads their backward launch lists (`UNetTrainer.bwd`: ("call", fn, args) with the
  positional arguments of include/eodiff.h), groups the calls into kernel chains, dedupes them on the non-pointer arguments and frees
  the trainer.  Each distinct geometry is replayed on fresh seeded tensors: the sizes, slab and split counts, ldp / ci0 / cvalid
  offsets and loss scale of the trainer, never its pointers;
- hand-picked edges (test_edge_*): empty splits, concat seams, loop tails, odd widths.  They are small and also run under the
  electric fence (tests/test_gpu_efence.py).

Every output buffer is NaN-filled before its launch, so a tile the kernel never writes shows up.  fp16 operands are rounded first and
the reference is built from the rounded values: the gates measure the kernel, not the input rounding.

Gates (rel-L2 against float64).  The ceilings are derived from the arithmetic; each gate is at most about 4x the worst error measured
on an MI355X over the harvested geometries and the edges (value in the comment next to it), and never above its ceiling."""
import collections
import gc
import math

import pytest
import torch

from tests import ref64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")

GATE = {
    # backward-weights (fp16 operands: every product exact in fp32, only the fp32 accumulation rounds; exact-fp32 GEMM path):
    # ceiling 2e-5 per dW, 1e-4 for the worst output channel.  Measured worst: 8.8e-7 per dW (A0@256 b16, Cx = 384 at 256 x 256),
    # 1.4e-6 for one output channel (exact-fp32 GEMM path, K = 6016 per split)
    "wgrad": 3.5e-6,
    "wgrad_row": 5e-6,
    # GroupNorm backward dx: ceiling 5e-6 with fp32 storage (measured 8.3e-8), 6e-4 with fp16 storage (measured 2.1e-4: the fp16
    # output rounding, ~2.8e-4 at most; 4x the measured value would exceed the ceiling, so the gate is the ceiling)
    "gn_dx_f32": 3e-7,
    "gn_dx_f16": 6e-4,
    # dgamma, dbeta, dfilm: ceiling 2e-5, measured 2.3e-7
    "gn_params": 9e-7,
    # eod_channel_sums_finish against float64 sums of the kernel's own stored dx (or of its input slab sums): ceiling 1e-5, measured 1.6e-7
    "csum": 6e-7,
    # eod_linear_bwd_small, eod_temb_pre1, eod_embedding_bwd, eod_rowsum_segments + eod_colsum, eod_mse_loss: ceiling 1e-5,
    # measured 6.8e-7 (the mse loss of 6.8 M elements; linear_bwd_small 4.1e-7, embedding_bwd exact)
    "small": 2.5e-6,
    # eod_gemm_tn (fp16 output): ceiling 6e-4, measured 2.1e-4 (the fp16 output rounding; the gate is the ceiling)
    "gemm_tn": 6e-4,
    # eod_gemm_nt backward-weights products (fp32 C): the backward-weights ceiling 2e-5, measured 1.4e-6
    "gemm_nt": 5e-6,
}
WORST = collections.defaultdict(float)  # gate name -> worst error seen in this session (printed with -s)


def _gate(name, err, what):
    WORST[name] = max(WORST[name], err)
    print(f"GATE {name:10s} {err:.3e}  {what}")
    assert math.isfinite(err) and err < GATE[name], (name, err, GATE[name], what)


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


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def rel(got, ref):
    got, ref = got.double(), ref.double()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


def worst_row(got, ref):
    """worst rel-L2 over the output channels (dim 0)"""
    got, ref = got.double().flatten(1), ref.double().flatten(1)
    return float(((got - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-300)).max())


class Rng:
    def __init__(self, seed):
        self.g = torch.Generator(device=DEV)
        self.g.manual_seed(seed)

    def randn(self, shape, scale=1.0, dtype=torch.float32, shift=0.0):
        return (torch.randn(shape, generator=self.g, device=DEV) * scale + shift).to(dtype)

    def randint(self, hi, shape):
        return torch.randint(0, hi, shape, generator=self.g, device=DEV)


def _g(**kw):
    return dict(kw)


# ================================================================================================ check helpers (one per chain)
def check_wgrad3(g, seed=1):
    """eod_conv3x3_wgrad -> eod_wgrad_reduce (-> eod_wgrad_up4_map for ups = 2): ups 0 plain, 1 nearest-2x input, 2 parity-class
    form, 3 stride 2"""
    L, st, lib = _L(), _st(), _lib()
    r = Rng(seed)
    N, H, W, Cx, Ho, Wo, Cy, Cout, ups = (g[k] for k in ("N", "H", "W", "Cx", "Ho", "Wo", "Cy", "Cout", "ups"))
    ldp, S, nci, ci0, Cin, scale = (g[k] for k in ("ldp", "S", "nci", "ci0", "Cin", "scale"))
    x = r.randn((N, H, W, Cx), dtype=torch.float16)
    dy = r.randn((N, Ho, Wo, Cy), 0.5, dtype=torch.float16)
    taps = 16 if ups == 2 else 9
    partial = _nan((S, taps, Cout, ldp))
    _ok(L.eod_conv3x3_wgrad(_p(dy), _p(x), lib.EOD_F16, N, H, W, Cx, Ho, Wo, Cy, Cout, ups, _p(partial), ldp, S, st), "conv3x3_wgrad")
    dw = _nan((Cout, Cin, 3, 3))
    if ups == 2:
        t16 = _nan((Cout, Cin, 16))
        _ok(L.eod_wgrad_reduce(_p(partial), S, 4, Cout, nci, ldp, ci0, Cin, scale, _p(t16), st), "wgrad_reduce")
        _ok(L.eod_wgrad_up4_map(_p(t16), Cout, Cin, _p(dw), st), "wgrad_up4_map")
    else:
        _ok(L.eod_wgrad_reduce(_p(partial), S, 3, Cout, nci, ldp, ci0, Cin, scale, _p(dw), st), "wgrad_reduce")
    torch.cuda.synchronize()
    del partial
    ref = scale * ref64.conv3x3_weight_grad(dy[..., :Cout], x[..., :nci], upsample=ups in (1, 2), stride=2 if ups == 3 else 1)
    got = dw[:, ci0:ci0 + nci]
    what = f"wgrad3 {g}"
    _gate("wgrad", rel(got, ref), what)
    _gate("wgrad_row", worst_row(got, ref), what)
    if ups != 2:  # the reduce writes its own columns of the shared dW and nothing else
        assert bool(dw[:, :ci0].isnan().all()) and bool(dw[:, ci0 + nci:].isnan().all()), what


def check_wgrad1(g, seed=1):
    """eod_conv1x1_wgrad -> eod_wgrad_reduce(ksize 1)"""
    L, st, lib = _L(), _st(), _lib()
    r = Rng(seed)
    npix, Cx, Cy, Cout, ldp, S, nci, ci0, Cin, scale = (g[k] for k in ("npix", "Cx", "Cy", "Cout", "ldp", "S", "nci", "ci0", "Cin", "scale"))
    x = r.randn((npix, Cx), dtype=torch.float16)
    dy = r.randn((npix, Cy), 0.5, dtype=torch.float16)
    partial = _nan((S, 1, Cout, ldp))
    _ok(L.eod_conv1x1_wgrad(_p(dy), _p(x), lib.EOD_F16, npix, Cx, Cy, Cout, _p(partial), ldp, S, st), "conv1x1_wgrad")
    dw = _nan((Cout, Cin))
    _ok(L.eod_wgrad_reduce(_p(partial), S, 1, Cout, nci, ldp, ci0, Cin, scale, _p(dw), st), "wgrad_reduce")
    torch.cuda.synchronize()
    ref = scale * ref64.conv1x1_weight_grad(dy[:, :Cout], x[:, :nci])
    got = dw[:, ci0:ci0 + nci]
    what = f"wgrad1 {g}"
    _gate("wgrad", rel(got, ref), what)
    _gate("wgrad_row", worst_row(got, ref), what)
    assert bool(dw[:, :ci0].isnan().all()) and bool(dw[:, ci0 + nci:].isnan().all()), what


def _slab_sums(x, P):
    """forward statistics slots of one concat source x [N][HW][C]: [N][P][C][2] fp32 {sum, sum of squares} over contiguous pixel
    slabs (how the slots split the pixels does not matter to the consumer: it sums all of them)"""
    N, HW, C = x.shape
    per = (HW + P - 1) // P
    x64 = torch.nn.functional.pad(x.double(), (0, 0, 0, P * per - HW)).reshape(N, P, per, C)
    return torch.stack([x64.sum(2), x64.square().sum(2)], -1).float()


def check_gn(g, seed=1):
    """the GroupNorm(+SiLU)(+FiLM) backward chain: eod_gn_mean_rstd -> eod_gn_bwd_partial (per source) -> eod_gn_bwd_finalize
    (dfilm) -> eod_gn_bwd_params, eod_gn_bwd_apply (per source, + add, + csum) -> eod_channel_sums_finish of the csum slabs"""
    L, st, lib = _L(), _st(), _lib()
    r = Rng(seed)
    f16 = g["f16"]
    td, dt = (torch.float16, lib.EOD_F16) if f16 else (torch.float32, lib.EOD_F32)
    N, HW, Ctot, G, eps, P, silu, scale = (g[k] for k in ("N", "HW", "Ctot", "groups", "eps", "P", "silu", "scale"))
    srcs = g["srcs"]  # ((C, coff, add, csum), ...)
    assert sum(s[0] for s in srcs) == Ctot
    xs = [r.randn((N, HW, s[0]), 1.5, td, shift=0.3) for s in srcs]
    dy = r.randn((N, HW, Ctot), dtype=td)
    gam = r.randn((Ctot,), 0.2, shift=1.0)
    bet = r.randn((Ctot,), 0.1)
    film = None
    if g["film"]:
        fstride = g["film_stride"]
        fbuf = r.randn((N, max(fstride, 2 * Ctot)), 0.3)
        film = (fbuf[:, :Ctot], fbuf[:, Ctot:2 * Ctot])
    x = torch.cat(xs, -1)
    # forward statistics slots (the slot counts of the trainer's producers) -> mean / rstd
    parts = [_slab_sums(xs[0], g["P0"])] + ([_slab_sums(xs[1], g["P1"])] if len(srcs) == 2 else [])
    mr = _nan((N, G, 2))
    p1 = (_p(parts[1]), g["P1"], srcs[1][0]) if len(srcs) == 2 else (0, 0, 0)
    _ok(L.eod_gn_mean_rstd(_p(parts[0]), g["P0"], srcs[0][0], *p1, N, HW, G, eps, _p(mr), st), "gn_mean_rstd")
    ss = ref64.group_norm_scale_shift(x, gam, bet, G, eps, film=film).float().contiguous()
    part = _nan((N, P, Ctot, 2))
    for xsrc, (C, coff, _, _) in zip(xs, srcs):
        _ok(L.eod_gn_bwd_partial(_p(xsrc), _p(dy), _p(ss), dt, N, HW, C, _p(part), P, Ctot, coff, int(silu), st), "gn_bwd_partial")
    coef, gb = _nan((N, Ctot, 3)), _nan((N, Ctot, 2))
    dfilm = None
    if film is not None:
        dstride = max(g["dfilm_stride"], 2 * Ctot)
        dfilm = _nan((N, dstride))
        _ok(L.eod_gn_bwd_finalize(_p(part), P, Ctot, N, HW, G, _p(mr), _p(gam), _p(bet), _p(fbuf), fbuf.shape[1], _p(dfilm), dstride,
                                  _p(coef), _p(gb), st), "gn_bwd_finalize")
    else:
        _ok(L.eod_gn_bwd_finalize(_p(part), P, Ctot, N, HW, G, _p(mr), _p(gam), 0, 0, 0, 0, 0, _p(coef), _p(gb), st), "gn_bwd_finalize")
    dgam, dbet = _nan((Ctot,)), _nan((Ctot,))
    _ok(L.eod_gn_bwd_params(_p(gb), N, Ctot, scale, _p(dgam), _p(dbet), st), "gn_bwd_params")
    outs = []
    for xsrc, (C, coff, with_add, with_csum) in zip(xs, srcs):
        add = r.randn((N, HW, C), 0.25, td) if with_add else None
        dx = _nan((N, HW, C), td)
        cs, Ps = None, 0
        if with_csum:
            Ps = L.eod_gn_bwd_apply_slabs(dt, N, HW, C)
            cs = _nan((N, Ps, C, 2))
        _ok(L.eod_gn_bwd_apply(_p(xsrc), _p(dy), _p(ss), _p(coef), _p(add), dt, N, HW, C, Ctot, coff, int(silu), _p(dx), _p(cs), st),
            "gn_bwd_apply")
        sums = None
        if with_csum:  # the conv behind: bias and per-image embedding-projection gradients from the slab sums of the stored dx
            dbias, demb, scr = _nan((C,)), _nan((N, C + 8)), _nan((N, C))
            _ok(L.eod_channel_sums_finish(_p(cs), N, Ps, C, C, scale, _p(dbias), _p(demb), C + 8, _p(scr), st), "channel_sums_finish")
            sums = (dbias, demb, Ps)
        outs.append((dx, add, sums))
    torch.cuda.synchronize()
    dx64, dgam64, dbet64, dfilm64 = ref64.group_norm_backward(x, dy, gam, bet, G, eps, silu_out=silu, film=film)
    what = f"gn {g}"
    for (dx, add, sums), (C, coff, _, _) in zip(outs, srcs):
        ref = dx64[..., coff:coff + C]
        if add is not None:
            ref = ref + add.double()
        _gate("gn_dx_f16" if f16 else "gn_dx_f32", rel(dx, ref), what)
        if sums is not None:
            dbias, demb, Ps = sums
            rb, re = ref64.channel_sums(dx, scale)
            _gate("csum", rel(dbias, rb), f"{what} csum P={Ps} (dbias)")
            _gate("csum", rel(demb[:, :C], re), f"{what} csum P={Ps} (demb)")
            assert bool(demb[:, C:].isnan().all()), what
    del dx64
    _gate("gn_params", rel(dgam, scale * dgam64), what + " dgamma")
    _gate("gn_params", rel(dbet, scale * dbet64), what + " dbeta")
    if dfilm is not None:
        _gate("gn_params", rel(dfilm[:, :2 * Ctot], dfilm64), what + " dfilm")
        assert bool(dfilm[:, 2 * Ctot:].isnan().all()), what


def check_csum(g, seed=1):
    """eod_channel_sums_finish on per-(image, slab, channel) sums [N][P][C][2] (sum at [0]): dbias (scaled) and / or demb"""
    L, st = _L(), _st()
    r = Rng(seed)
    N, P, C, cvalid, scale, ld = (g[k] for k in ("N", "P", "C", "cvalid", "scale", "demb_ld"))
    part = r.randn((N, P, C, 2))
    dbias = _nan((cvalid,)) if g["dbias"] else None
    demb = _nan((N, ld)) if g["demb"] else None
    scr = _nan((N, cvalid)) if g["dbias"] else None
    _ok(L.eod_channel_sums_finish(_p(part), N, P, C, cvalid, scale, _p(dbias), _p(demb), ld, _p(scr), st), "channel_sums_finish")
    torch.cuda.synchronize()
    rb, re = ref64.channel_sums(part[:, :, :cvalid, 0], scale)
    what = f"csum {g}"
    if dbias is not None:
        _gate("csum", rel(dbias, rb), what + " dbias")
    if demb is not None:
        _gate("csum", rel(demb[:, :cvalid], re), what + " demb")
        assert bool(demb[:, cvalid:].isnan().all()), what


def _freqs(half):
    return torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32, device=DEV) / max(half, 1))


def check_linear(g, seed=1):
    """eod_linear_bwd_small: dW / db (scaled) and / or din (* SiLU'(pre)); act_in 0 = in, 1 = SiLU(in), 2 = sinusoid(t)"""
    L, st = _L(), _st()
    r = Rng(seed)
    ld, N, K, J, act, scale = (g[k] for k in ("ld_dout", "N", "K", "J", "act_in", "scale"))
    dbuf = r.randn((N, ld))
    t = r.randint(1000, (N,))
    freqs = _freqs(K // 2)
    inp = r.randn((N, K), 1.5)
    w = r.randn((J, K), 1.0 / math.sqrt(K))
    pre = r.randn((N, K), 1.5) if g["pre"] else None
    dW = _nan((J, K)) if g["dW"] else None
    db = _nan((J,)) if g["db"] else None
    din = _nan((N, K)) if g["din"] else None
    scr = _nan((32, N, K)) if g["scratch"] else None
    _ok(L.eod_linear_bwd_small(_p(dbuf), ld, _p(inp) if act != 2 else 0, _p(t) if act == 2 else 0, _p(freqs) if act == 2 else 0, _p(w),
                               _p(pre), N, K, J, act, scale, _p(dW), _p(db), _p(din), _p(scr), st), "linear_bwd_small")
    torch.cuda.synchronize()
    a = ref64.sinusoid(t, freqs, K) if act == 2 else inp
    rW, rb, rin = ref64.linear_backward(dbuf[:, :J], a, w, act_in=1 if act == 1 else 0, scale=scale, pre=pre)
    what = f"linear {g}"
    if dW is not None:
        _gate("small", rel(dW, rW), what + " dW")
    if db is not None:
        _gate("small", rel(db, rb), what + " db")
    if din is not None:
        _gate("small", rel(din, rin), what + " din")


def check_temb_pre1(g, seed=1):
    L, st = _L(), _st()
    r = Rng(seed)
    N, D, E = g["N"], g["D"], g["E"]
    t = r.randint(1000, (N,))
    freqs = _freqs(D // 2)
    w1, b1 = r.randn((E, D), 1.0 / math.sqrt(D)), r.randn((E,), 0.1)
    pre1 = _nan((N, E))
    _ok(L.eod_temb_pre1(_p(t), _p(freqs), _p(w1), _p(b1), N, D, E, _p(pre1), st), "temb_pre1")
    torch.cuda.synchronize()
    _gate("small", rel(pre1, ref64.temb_pre1(t, freqs, w1, b1)), f"temb_pre1 {g}")


def check_embedding(g, seed=1):
    L, st = _L(), _st()
    r = Rng(seed)
    N, E, classes, scale = g["N"], g["E"], g["classes"], g["scale"]
    y = torch.tensor(g["y"], device=DEV) if "y" in g else r.randint(classes, (N,))
    dout = r.randn((N, E))
    dW = _nan((classes, E))
    _ok(L.eod_embedding_bwd(_p(dout), _p(y), N, E, classes, scale, _p(dW), st), "embedding_bwd")
    torch.cuda.synchronize()
    ref = ref64.embedding_backward(dout, y, classes, scale)
    _gate("small", rel(dW, ref), f"embedding {g}")
    unused = [c for c in range(classes) if c not in set(y.tolist())]
    assert bool((dW[unused] == 0).all()), (g, unused)


def check_transpose_gather(g, seed=1):
    """bit-exact, zeros in the pad rows and the tail columns included"""
    L, st, lib = _L(), _st(), _lib()
    r = Rng(seed)
    td, dt = (torch.float16, lib.EOD_F16) if g["f16"] else (torch.float32, lib.EOD_F32)
    N, H, W, C, ld, Ho, Wo = (g[k] for k in ("N", "H", "W", "C", "ld_dst", "Ho", "Wo"))
    stride, pad, gy, gx, ups, rp = (g[k] for k in ("stride", "pad", "dy", "dx", "ups", "row_pad"))
    src = r.randn((N, H, W, C), dtype=td)
    dst = _nan((C, ld), td)
    _ok(L.eod_transpose_gather(_p(src), dt, N, H, W, C, _p(dst), ld, Ho, Wo, stride, pad, gy, gx, ups, rp, st), "transpose_gather")
    torch.cuda.synchronize()
    ref = ref64.transpose_gather(src, ld, Ho, Wo, stride, pad, gy, gx, ups, rp)
    iv = torch.int16 if g["f16"] else torch.int32
    assert torch.equal(dst.view(iv), ref.view(iv)), f"transpose_gather {g}: {int((dst.view(iv) != ref.view(iv)).sum())} elements differ"


def check_rowsum(g, seed=1):
    """eod_rowsum_segments (+ eod_colsum over its segments)"""
    L, st, lib = _L(), _st(), _lib()
    r = Rng(seed)
    td, dt = (torch.float16, lib.EOD_F16) if g["f16"] else (torch.float32, lib.EOD_F32)
    C, ld, nseg, seg_len, scale, seg_ld = (g[k] for k in ("C", "ld", "nseg", "seg_len", "scale", "seg_ld"))
    x = r.randn((C, ld), dtype=td)
    seg = _nan((nseg, seg_ld))
    _ok(L.eod_rowsum_segments(_p(x), dt, C, ld, nseg, seg_len, scale, _p(seg), seg_ld, st), "rowsum_segments")
    out = None
    if g["colsum"]:
        out = _nan((C,))
        _ok(L.eod_colsum(_p(seg), nseg, C, _p(out), st), "colsum")  # (seg_ld == C: the form the trainer uses)
    torch.cuda.synchronize()
    ref = ref64.rowsum_segments(x, nseg, seg_len, scale)
    what = f"rowsum {g}"
    _gate("small", rel(seg[:, :C], ref), what)
    if seg_ld > C:
        assert bool(seg[:, C:].isnan().all()), what
    if out is not None:
        _gate("small", rel(out, ref.sum(0)), what + " colsum")


def _extent(off, counts_strides):
    return off + sum((n - 1) * s for n, s in counts_strides if s > 0) + 1


def _lead(counts_strides):
    """elements in front of the first batch's origin that negative strides reach"""
    return -sum((n - 1) * s for n, s in counts_strides if s < 0)


def _aligned_off(lead, mod, step):
    """smallest offset >= lead that is congruent to `mod` modulo `step` elements (keeps the harvested pointer's alignment)"""
    return lead + (mod - lead) % step


def _gather_c(c, off, nb0, nb1, M, N, ldc, sc):
    return torch.stack([c.as_strided((nb0, M, N), (sc[0], ldc, 1), off + b1 * sc[1]) for b1 in range(nb1)], 1)


def check_gemm_tn(g, seed=1):
    """eod_gemm_tn, fp16: C = alpha * A^T B with both operands K-major, two-level batch strides (the attention backward's dK / dV)"""
    L, st, lib = _L(), _st(), _lib()
    r = Rng(seed)
    M, N, K, lda, ldb, ldc, alpha, nb0, nb1 = (g[k] for k in ("M", "N", "K", "lda", "ldb", "ldc", "alpha", "nb0", "nb1"))
    sa, sb, sc = (g["sa0"], g["sa1"]), (g["sb0"], g["sb1"]), (g["sc0"], g["sc1"])
    ao, bo, co = (_aligned_off(0, g.get(k, 0), 128) for k in ("a_mod", "b_mod", "c_mod"))
    a = r.randn((_extent(ao, [(nb0, sa[0]), (nb1, sa[1]), (K, lda), (M, 1)]),), dtype=torch.float16)
    b = r.randn((_extent(bo, [(nb0, sb[0]), (nb1, sb[1]), (K, ldb), (N, 1)]),), dtype=torch.float16)
    c = _nan((_extent(co, [(nb0, sc[0]), (nb1, sc[1]), (M, ldc), (N, 1)]),), torch.float16)
    _ok(L.eod_gemm_tn(_p(a) + 2 * ao, lda, _p(b) + 2 * bo, ldb, _p(c) + 2 * co, ldc, lib.EOD_F16, M, N, K, alpha, nb0, nb1, sa[0], sa[1], sb[0], sb[1],
                      sc[0], sc[1], st), "gemm_tn")
    torch.cuda.synchronize()
    ref = ref64.gemm_tn(a, b, M=M, N=N, K=K, lda=lda, ldb=ldb, alpha=alpha, nb0=nb0, nb1=nb1, sa=sa, sb=sb, a_off=ao, b_off=bo)
    del a, b
    got = _gather_c(c, co, nb0, nb1, M, N, ldc, sc)
    what = f"gemm_tn {g}"
    _gate("gemm_tn", rel(got, ref), what)
    assert int((~c.isnan()).sum()) == nb0 * nb1 * M * N, what  # nothing written outside C


def check_gemm_nt(g, seed=1):
    """eod_gemm_nt through engine.Program.gemm in the batched forms of the backward-weights GEMM path: nb1 = 3 column / row taps, a
    negative inner A stride (the dY shifts), element offsets into shared buffers, fp32 C"""
    from eo_diffusion_amd.engine import Program
    r = Rng(seed)
    prec = "fp16" if g["f16"] else "fp32"
    td = torch.float16 if g["f16"] else torch.float32
    es = 2 if g["f16"] else 4
    M, N, K, lda, ldb, ldc, alpha, nb0, nb1 = (g[k] for k in ("M", "N", "K", "lda", "ldb", "ldc", "alpha", "nb0", "nb1"))
    sa, sb, sc = (g["sa0"], g["sa1"]), (g["sb0"], g["sb1"]), (g["sc0"], g["sc1"])
    A = [(nb0, sa[0]), (nb1, sa[1]), (M, lda), (K, 1)]
    B = [(nb0, sb[0]), (nb1, sb[1]), (N, ldb), (K, 1)]
    Cs = [(nb0, sc[0]), (nb1, sc[1]), (M, ldc), (N, 1)]
    ao = _aligned_off(_lead(A), g.get("a_mod", 0), 256 // es)
    bo = _aligned_off(_lead(B), g.get("b_mod", 0), 256 // es)
    co = _aligned_off(_lead(Cs), g.get("c_mod", 0), 64)
    a = r.randn((_extent(ao, A),), dtype=td)
    b = r.randn((_extent(bo, B),), dtype=td)
    c = _nan((_extent(co, Cs),))
    prog = Program(DEV, prec)
    prog.gemm(a, b, c, M, N, K, lda, ldb, ldc, alpha=alpha, c_f32=True, nb0=nb0, nb1=nb1, sa=sa, sb=sb, sc=sc, a_off=ao, b_off=bo, c_off=co)
    prog.run()
    torch.cuda.synchronize()
    ref = ref64.gemm_nt(a, b, M=M, N=N, K=K, lda=lda, ldb=ldb, alpha=alpha, nb0=nb0, nb1=nb1, sa=sa, sb=sb, a_off=ao, b_off=bo)
    del a, b
    got = _gather_c(c, co, nb0, nb1, M, N, ldc, sc)
    what = f"gemm_nt {g}"
    _gate("gemm_nt", rel(got, ref), what)
    _gate("wgrad_row", worst_row(got.transpose(0, 2).reshape(M, -1), ref.transpose(0, 2).reshape(M, -1)), what)
    assert int((~c.isnan()).sum()) == nb0 * nb1 * M * N, what


def check_mse(n, seed=1):
    L, st = _L(), _st()
    r = Rng(seed)
    pred, target = r.randn((n,)), r.randn((n,), 0.5, shift=0.1)
    loss, dpred, scr = _nan((1,)), _nan((n,)), _nan((1024,))
    _ok(L.eod_mse_loss(_p(pred), _p(target), n, _p(loss), _p(dpred), _p(scr), 1024, st), "mse_loss")
    torch.cuda.synchronize()
    rl, rd = ref64.mse_loss(pred, target)
    _gate("small", abs(float(loss) - float(rl)) / float(rl), f"mse n={n} loss")
    _gate("small", rel(dpred, rd), f"mse n={n} dpred")


CHECK = {"wgrad3": check_wgrad3, "wgrad1": check_wgrad1, "gn": check_gn, "csum": check_csum, "linear": check_linear,
         "temb_pre1": check_temb_pre1, "embedding": check_embedding, "transpose_gather": check_transpose_gather, "rowsum": check_rowsum,
         "gemm_tn": check_gemm_tn, "gemm_path": check_gemm_nt}


# ================================================================================================ harvest from real trainers
# positional arguments of include/eodiff.h (the stream, appended at run time, excluded); '*' marks a pointer
SPECS = {k: tuple(v.split()) for k, v in {
    "eod_conv3x3_wgrad": "*dy *x dtype N H W Cx Ho Wo Cy Cout ups *partial ldp S",
    "eod_conv1x1_wgrad": "*dy *x dtype npix Cx Cy Cout *partial ldp S",
    "eod_wgrad_reduce": "*partial S ksize Cout nci ldp ci0 Cin scale *dw",
    "eod_wgrad_up4_map": "*t16 Cout Cin *dw",
    "eod_gn_mean_rstd": "*part0 P0 C0 *part1 P1 C1 N HW groups eps *mean_rstd",
    "eod_gn_bwd_partial": "*x *dy *ss dtype N HW C *part P Ctot coff silu",
    "eod_gn_bwd_finalize": "*part P Ctot N HW groups *mean_rstd *gamma *beta *film film_stride *dfilm dfilm_stride *coef *gb",
    "eod_gn_bwd_params": "*gb N Ctot scale *dgamma *dbeta",
    "eod_gn_bwd_apply": "*x *dy *ss *coef *add dtype N HW C Ctot coff silu *dx *csum",
    "eod_channel_sums_finish": "*part N P C cvalid scale *dbias *demb demb_ld *scratch",
    "eod_linear_bwd_small": "*dout ld_dout *in *t *freqs *w *pre N K J act_in scale *dW *db *din *scratch",
    "eod_temb_pre1": "*t *freqs *w1 *b1 N D E *pre1",
    "eod_embedding_bwd": "*dout *y N E classes scale *dW",
    "eod_transpose_gather": "*src dtype N H W C *dst ld_dst Ho Wo stride pad dy dx ups row_pad",
    "eod_rowsum_segments": "*x dtype C ld nseg seg_len scale *seg seg_ld",
    "eod_colsum": "*seg S C *out",
    "eod_gemm_tn": "*a lda *b ldb *c ldc dtype M N K alpha nb0 nb1 sa0 sa1 sb0 sb1 sc0 sc1",
}.items()}


def _named(fname, args):
    spec = SPECS[fname]
    assert len(spec) == len(args), f"{fname}: {len(args)} arguments, include/eodiff.h has {len(spec)}"
    return {n.lstrip("*"): a for n, a in zip(spec, args)}


def _after(calls, i, fname, key, val):
    for j in range(i + 1, len(calls)):
        if calls[j][0] == fname and calls[j][1][key] == val:
            return calls[j][1]
    raise AssertionError(f"{fname} consuming {key} of call {i} ({calls[i][0]}) not found")


def _harvest_trainer(tr, label):
    from eo_diffusion_amd import _lib as lib
    calls = []
    for item in tr.bwd:
        if item[0] == "call" and item[1].__name__ in SPECS:
            calls.append((item[1].__name__, _named(item[1].__name__, item[2])))
    seen = set()
    out = collections.defaultdict(list)

    def add(chain, g):
        key = (chain, repr(sorted(g.items())))
        if key not in seen:
            seen.add(key)
            out[chain].append(dict(g, src=label))

    for i, (f, a) in enumerate(calls):
        if f == "eod_conv3x3_wgrad":
            rd = _after(calls, i, "eod_wgrad_reduce", "partial", a["partial"])
            assert rd["S"] == a["S"] and rd["ksize"] == (4 if a["ups"] == 2 else 3) and rd["ldp"] == a["ldp"]
            if a["ups"] == 2:
                _after(calls, i, "eod_wgrad_up4_map", "t16", rd["dw"])
            add("wgrad3", _g(**{k: a[k] for k in ("N", "H", "W", "Cx", "Ho", "Wo", "Cy", "Cout", "ups", "ldp", "S")},
                             nci=rd["nci"], ci0=rd["ci0"], Cin=rd["Cin"], scale=rd["scale"]))
        elif f == "eod_conv1x1_wgrad":
            rd = _after(calls, i, "eod_wgrad_reduce", "partial", a["partial"])
            assert rd["S"] == a["S"] and rd["ksize"] == 1
            add("wgrad1", _g(**{k: a[k] for k in ("npix", "Cx", "Cy", "Cout", "ldp", "S")}, nci=rd["nci"], ci0=rd["ci0"], Cin=rd["Cin"],
                             scale=rd["scale"]))
        elif f == "eod_gn_bwd_finalize":
            mr = [c for j, (ff, c) in enumerate(calls[:i]) if ff == "eod_gn_mean_rstd" and c["mean_rstd"] == a["mean_rstd"]][-1]
            parts = [c for ff, c in calls[:i] if ff == "eod_gn_bwd_partial" and c["part"] == a["part"]]
            prm = _after(calls, i, "eod_gn_bwd_params", "gb", a["gb"])
            apps = [c for ff, c in calls[i + 1:] if ff == "eod_gn_bwd_apply" and c["coef"] == a["coef"]]
            apps = sorted(apps, key=lambda c: c["coff"])
            srcs = tuple((c["C"], c["coff"], bool(c["add"]), bool(c["csum"])) for c in apps)
            assert sum(s[0] for s in srcs) == a["Ctot"] and mr["C0"] == srcs[0][0] and mr["C1"] == (srcs[1][0] if len(srcs) == 2 else 0)
            assert {c["silu"] for c in parts + apps} == {apps[0]["silu"]} and parts[-1]["P"] == a["P"]
            add("gn", _g(f16=apps[0]["dtype"] == lib.EOD_F16, N=a["N"], HW=a["HW"], Ctot=a["Ctot"], groups=a["groups"], eps=mr["eps"],
                         P0=mr["P0"], P1=mr["P1"], P=a["P"], silu=bool(apps[0]["silu"]), film=bool(a["dfilm"]), film_stride=a["film_stride"],
                         dfilm_stride=a["dfilm_stride"], scale=prm["scale"], srcs=srcs))
        elif f == "eod_channel_sums_finish":
            add("csum", _g(**{k: a[k] for k in ("N", "P", "C", "cvalid", "scale", "demb_ld")}, dbias=bool(a["dbias"]), demb=bool(a["demb"])))
        elif f == "eod_linear_bwd_small":
            add("linear", _g(**{k: a[k] for k in ("ld_dout", "N", "K", "J", "act_in", "scale")},
                             **{k: bool(a[k]) for k in ("pre", "dW", "db", "din", "scratch")}))
        elif f == "eod_temb_pre1":
            add("temb_pre1", _g(N=a["N"], D=a["D"], E=a["E"]))
        elif f == "eod_embedding_bwd":
            add("embedding", _g(N=a["N"], E=a["E"], classes=a["classes"], scale=a["scale"]))
        elif f == "eod_transpose_gather":
            add("transpose_gather", _g(f16=a["dtype"] == lib.EOD_F16, **{k: a[k] for k in ("N", "H", "W", "C", "ld_dst", "Ho", "Wo", "stride",
                                                                                            "pad", "dy", "dx", "ups", "row_pad")}))
        elif f == "eod_rowsum_segments":
            cs = [c for ff, c in calls[i + 1:] if ff == "eod_colsum" and c["seg"] == a["seg"]]
            if cs:
                assert cs[0]["S"] == a["nseg"] and cs[0]["C"] == a["C"] == a["seg_ld"]
            add("rowsum", _g(f16=a["dtype"] == lib.EOD_F16, colsum=bool(cs), **{k: a[k] for k in ("C", "ld", "nseg", "seg_len", "scale", "seg_ld")}))
        elif f == "eod_gemm_tn":
            add("gemm_tn", _g(**{k: a[k] for k in ("lda", "ldb", "ldc", "M", "N", "K", "alpha", "nb0", "nb1", "sa0", "sa1", "sb0", "sb1", "sc0", "sc1")},
                              a_mod=(a["a"] % 256) // 2, b_mod=(a["b"] % 256) // 2, c_mod=(a["c"] % 256) // 2))
    for item in tr.bwd:  # the backward-weights GEMMs of the transposed-operand path (fp32 partial tiles, no epilogue)
        if item[0] == "op" and item[1].kind == lib.OP_GEMM:
            d = item[1].u.gemm
            if not (d.c_f32 and d.bias_mode == 0 and not d.res and not d.x3):
                continue
            es = 2 if d.dtype == lib.EOD_F16 else 4
            add("gemm_path", _g(f16=d.dtype == lib.EOD_F16, M=d.M, N=d.N, K=d.K, lda=d.lda, ldb=d.ldb, ldc=d.ldc, alpha=float(d.alpha), nb0=d.nb0,
                              nb1=d.nb1, sa0=d.sa0, sa1=d.sa1, sb0=d.sb0, sb1=d.sb1, sc0=d.sc0, sc1=d.sc1,
                              a_mod=(d.a % 256) // es, b_mod=(d.b % 256) // es, c_mod=(d.c % 256) // 4))
    return out


A0 = dict(model_channels=128, channel_mult=[1, 2, 3, 4], attention_resolutions=[], num_res_blocks=1, num_heads=1)
A1 = dict(model_channels=128, channel_mult=[1, 2, 3, 4], attention_resolutions=[4, 8], num_res_blocks=2, num_heads=8)
TRAINERS = [  # label, arch, image size, channels, batch, precision, extra constructor arguments
    ("A0@256 b16 fp16", A0, 256, 3, 16, "fp16", {}),                  # the training benchmark (tools/train_bench.py)
    ("A1@512x13 b2 fp16", A1, 512, 13, 2, "fp16", {}),                # BASELINE config 5 at its full per-GPU shape
    ("A0@256 b2 fp32", A0, 256, 3, 2, "fp32", {}),                    # exact fp32: the transposed-operand GEMM path
    ("A1@64 b2 fp16 film+classes", A1, 64, 3, 2, "fp16", dict(use_scale_shift_norm=True, num_classes=10)),
]


@pytest.fixture(scope="module")
def harvest():
    from eo_diffusion_amd.backbones.unet_openai import UNetModel
    from eo_diffusion_amd.training import UNetTrainer
    merged = collections.defaultdict(list)
    keys = set()
    for label, arch, size, ch, N, prec, extra in TRAINERS:
        unet = UNetModel(size, in_channels=ch, out_channels=ch, **arch, **extra).set_precision(prec).to(DEV).train()
        tr = UNetTrainer(unet, N, size, size, DEV, loss_scale=(1024.0 if prec == "fp16" else 1.0))
        got = _harvest_trainer(tr, label)
        del tr, unet
        gc.collect()
        torch.cuda.empty_cache()
        for chain, gs in got.items():
            for g in gs:
                k = (chain, repr(sorted((a, b) for a, b in g.items() if a != "src")))
                if k not in keys:
                    keys.add(k)
                    merged[chain].append(g)
    for chain, gs in sorted(merged.items()):
        print(f"harvest: {chain:16s} {len(gs):3d} distinct geometries")
    return merged


def test_harvest_is_complete(harvest):
    """every chain is reached by the real trainers, in every mode the tests below rely on: a trainer change that moves work to another
    kernel fails here instead of leaving a check that checks nothing"""
    from eo_diffusion_amd import _lib as lib
    L = lib.lib()
    for chain in CHECK:
        assert harvest[chain], f"no {chain} launch in any trainer"
    assert {g["ups"] for g in harvest["wgrad3"]} >= {0, 2, 3}, "plain, parity-class and stride-2 backward-weights"
    assert any(g["S"] >= 170 for g in harvest["wgrad3"]), "the production split count of the 128 -> 128 convs"
    assert any(g["nci"] < g["ldp"] for g in harvest["wgrad3"]), "the first conv (input channels padded to one 16-byte chunk)"
    assert any(g["ci0"] > 0 for g in harvest["wgrad1"]), "the second concat source of a skip connection"
    assert any(g["Cout"] < g["Cy"] for g in harvest["wgrad3"]), "the head conv (Cout < the padded gradient width)"
    assert {g["act_in"] for g in harvest["linear"]} == {0, 1, 2}, "the three timestep-MLP backward forms"
    assert any(g["J"] >= 512 and g["scratch"] and g["din"] for g in harvest["linear"]), "the 32-way split of linear_bwd_small"
    gn = harvest["gn"]
    assert any(g["film"] for g in gn), "the FiLM finalize (dfilm)"
    assert any(len(g["srcs"]) == 2 for g in gn) and any(s[2] for g in gn for s in g["srcs"]) and any(s[3] for g in gn for s in g["srcs"])
    assert any(not g["f16"] for g in gn) and any(g["f16"] for g in gn)
    assert max(L.eod_gn_bwd_apply_slabs(lib.EOD_F16, g["N"], g["HW"], s[0]) for g in gn if g["f16"] for s in g["srcs"] if s[3]) >= 2048
    assert any(g["P0"] * (g["Ctot"] // g["groups"]) > 768 for g in gn), "the unrolled loop of gn_mean_rstd"
    assert any(g["dbias"] and g["demb"] for g in harvest["csum"])
    assert any(g["colsum"] for g in harvest["rowsum"])
    assert any(g["nb1"] == 3 and g["sa1"] < 0 for g in harvest["gemm_path"]), "the dY-shift form of the GEMM path"


@pytest.mark.parametrize("chain", list(CHECK))
def test_harvested_geometries(harvest, chain):
    for i, g in enumerate(harvest[chain]):
        CHECK[chain](g, seed=1000 + i)
        gc.collect()
    print(f"{chain}: {len(harvest[chain])} geometries, worst " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(WORST.items())))


# ================================================================================================ hand-picked edges
def _w3(N, H, W, Cx, Cout, ups, S, Cy=None, nci=None, ci0=0, Cin=None, ldp=None, scale=1.0):
    Ho, Wo = ((H // 2, W // 2) if ups == 3 else (2 * H, 2 * W) if ups in (1, 2) else (H, W))
    return _g(N=N, H=H, W=W, Cx=Cx, Ho=Ho, Wo=Wo, Cy=Cy or Cout, Cout=Cout, ups=ups, ldp=ldp or Cx, S=S, nci=nci or Cx, ci0=ci0,
              Cin=Cin or (ci0 + (nci or Cx)), scale=scale)


EDGE_WGRAD3 = [
    _w3(1, 4, 64, 64, 64, 0, 7),                        # S larger than the strip count: empty splits write zero tiles
    _w3(2, 16, 64, 40, 24, 0, 5),                       # S not a multiple of 4, channel counts that are not tile multiples
    _w3(2, 64, 64, 128, 128, 0, 170, scale=1 / 1024),   # the production split count (170 of 128 strips: the tail splits are empty)
    _w3(1, 8, 16, 24, 40, 0, 3),                        # 16-wide strips (4 image rows per strip)
    _w3(2, 16, 32, 16, 16, 0, 6),                       # 32-wide strips
    _w3(1, 16, 64, 16, 3, 0, 4, Cy=8, nci=13, Cin=13),  # Cout < Cy (head), nci < ldp (13 input channels padded to 16)
    _w3(1, 8, 64, 128, 128, 0, 9, ci0=128, Cin=256),    # second concat source (ci0 > 0)
    _w3(1, 8, 64, 64, 64, 0, 4, ldp=72),                # partial tiles with a row pitch beyond Cx
    _w3(2, 8, 32, 24, 40, 1, 5),                        # nearest-2x input, nine-tap form
    _w3(1, 8, 32, 136, 128, 2, 64, scale=1 / 1024),     # parity-class form, production split count of 8 tile planes
    _w3(2, 4, 16, 16, 24, 2, 3),                        # parity-class form on 16-wide stored rows
    _w3(1, 16, 128, 40, 24, 3, 85),                     # stride 2, production split count of 6 tile planes
    _w3(2, 32, 32, 8, 200, 3, 5),                       # stride 2 on 16-wide output rows
]


@pytest.mark.parametrize("g", EDGE_WGRAD3, ids=lambda g: "N{N}_{H}x{W}_cx{Cx}_co{Cout}_ups{ups}_S{S}_ci0{ci0}".format(**g))
def test_edge_conv3x3_backward_weights(g):
    check_wgrad3(g, seed=7)


@pytest.mark.parametrize("g", [
    _g(npix=3 * 5 * 7, Cx=40, Cy=48, Cout=40, ldp=40, S=7, nci=40, ci0=0, Cin=40, scale=1.0),       # ragged last strip, empty splits
    _g(npix=4096, Cx=136, Cy=128, Cout=128, ldp=136, S=5, nci=136, ci0=0, Cin=136, scale=1.0),    # S not a multiple of 4
    _g(npix=2 * 64 * 64, Cx=128, Cy=384, Cout=384, ldp=128, S=128, nci=128, ci0=128, Cin=256, scale=1 / 1024),  # second source
    _g(npix=1024, Cx=264, Cy=16, Cout=8, ldp=264, S=512, nci=260, ci0=0, Cin=260, scale=1.0),     # S >> strips, Cout < Cy, nci < ldp
], ids=lambda g: "npix{npix}_cx{Cx}_co{Cout}_S{S}".format(**g))
def test_edge_conv1x1_backward_weights(g):
    check_wgrad1(g, seed=8)


def _gn(N, HW, srcs, P, P0, P1=0, f16=True, silu=True, film=False, scale=1.0):
    src = tuple((c, sum(s[0] for s in srcs[:i]), add, cs) for i, (c, add, cs) in enumerate(srcs))
    ctot = sum(s[0] for s in srcs)
    return _g(f16=f16, N=N, HW=HW, Ctot=ctot, groups=32, eps=1e-5, P0=P0, P1=P1, P=P, silu=silu, film=film, film_stride=2 * ctot + 64,
              dfilm_stride=2 * ctot + 32, scale=scale, srcs=src)


EDGE_GN = [
    _gn(2, 35, [(104, False, True), (88, True, False)], 1, 1, 1, f16=False),         # a group straddles the concat seam (fp32)
    _gn(2, 35, [(104, True, True), (88, False, True)], 5, 3, 2),                      # ... fp16, several slabs
    _gn(2, 64, [(384, False, True)], 16, 7),                                          # cpg = 12 (does not divide 256)
    _gn(1, 30, [(2560, False, False)], 3, 2),                                         # > 256 chunk columns (channel blocks along z)
    _gn(2, 9, [(1536, False, False), (1024, False, False)], 2, 1, 1, f16=False, silu=False),   # the same in fp32, two sources
    _gn(1, 1024, [(128, False, True)], 16, 191),                                      # 764 (slot, channel) pairs per group: below 768
    _gn(1, 1024, [(128, False, True)], 16, 193),                                      # 772: the unrolled loop runs
    _gn(1, 4096, [(256, True, True)], 64, 2048, scale=1 / 1024),                      # production slot count
    _gn(2, 1000, [(64, False, True)], 15, 13, film=True),                             # HW not a multiple of the slab length, FiLM
    _gn(16, 256, [(128, True, True)], 4, 4, film=True, f16=False),                    # N = 16, FiLM in fp32
    _gn(1, 64, [(64, False, False)], 1, 1, silu=False),                               # N = 1, no SiLU
]


@pytest.mark.parametrize("g", EDGE_GN, ids=lambda g: "{}_N{}_HW{}_C{}_P{}_P0{}{}".format(
    "f16" if g["f16"] else "f32", g["N"], g["HW"], "+".join(str(s[0]) for s in g["srcs"]), g["P"], g["P0"], "_film" if g["film"] else ""))
def test_edge_group_norm_backward(g):
    check_gn(g, seed=9)


@pytest.mark.parametrize("g", [
    _g(N=2, P=5, C=64, cvalid=64, scale=1.0, demb_ld=64, dbias=True, demb=True),      # P < 16: most slab segments empty
    _g(N=3, P=100, C=256, cvalid=200, scale=0.5, demb_ld=264, dbias=True, demb=True),  # 7 slabs per segment (tail loop), cvalid < C, % 64 != 0
    _g(N=1, P=2051, C=72, cvalid=3, scale=1 / 1024, demb_ld=8, dbias=True, demb=False),  # dbias only, 3 of 72 channels
    _g(N=4, P=37, C=128, cvalid=128, scale=1.0, demb_ld=1000, dbias=False, demb=True),   # demb only, row stride of the gradient concat
], ids=lambda g: "N{N}_P{P}_C{C}_cv{cvalid}_{dbias}_{demb}".format(**g))
def test_edge_channel_sums_finish(g):
    check_csum(g, seed=10)


def _lin(N, K, J, act, *, ld=None, pre=False, dW=True, db=True, din=True, scratch=False, scale=1.0):
    return _g(ld_dout=ld or J, N=N, K=K, J=J, act_in=act, scale=scale, pre=pre, dW=dW, db=db, din=din, scratch=scratch)


@pytest.mark.parametrize("g", [
    _lin(2, 512, 511, 1, pre=True, dW=False, db=False, scratch=True),   # J = 511: one J range
    _lin(2, 512, 512, 1, pre=True, dW=False, db=False, scratch=True),   # J = 512: the 32-way split
    _lin(3, 96, 520, 1, ld=600, pre=True, scratch=True),                # J not a multiple of 32 (the last split is shorter), ld > J
    _lin(2, 64, 200, 0, pre=True),                                      # act_in 0 with SiLU'(pre)
    _lin(4, 33, 64, 2, dW=True, db=True, din=False, scale=0.5),         # odd sinusoid width (the last column is zero)
    _lin(1, 128, 512, 2, din=False),                                    # N = 1
], ids=lambda g: "N{N}_K{K}_J{J}_act{act_in}_scr{scratch}".format(**g))
def test_edge_linear_backward_small(g):
    check_linear(g, seed=11)


@pytest.mark.parametrize("g", [_g(N=3, D=33, E=64), _g(N=1, D=128, E=512)], ids=lambda g: "N{N}_D{D}_E{E}".format(**g))
def test_edge_temb_pre1(g):
    check_temb_pre1(g, seed=12)


def test_edge_embedding_backward_repeated_and_unused_labels():
    check_embedding(_g(N=6, E=96, classes=8, scale=0.25, y=[3, 3, 0, 3, 5, 0]), seed=13)


def _tg(f16, N, H, W, C, Ho, Wo, stride, pad, dy, dx, ups, rp, extra):
    return _g(f16=f16, N=N, H=H, W=W, C=C, Ho=Ho, Wo=Wo, stride=stride, pad=pad, dy=dy, dx=dx, ups=ups, row_pad=rp,
              ld_dst=N * (Ho + 2 * rp) * Wo + extra)


@pytest.mark.parametrize("g", [
    _tg(True, 2, 7, 9, 72, 4, 5, 2, 1, 0, 2, 0, 0, 8),     # stride 2 with pad, border taps, C not a multiple of 64, zero tail
    _tg(False, 2, 7, 9, 20, 4, 5, 2, 1, 2, 0, 0, 0, 4),    # the same in fp32
    _tg(True, 1, 5, 6, 40, 10, 12, 1, 1, 0, 0, 1, 1, 16),  # nearest-2x source, pad rows (row_pad)
    _tg(False, 3, 8, 8, 68, 8, 8, 1, 1, 2, 2, 0, 1, 60),   # bottom-right tap, pad rows, C and K not multiples of 64
    _tg(True, 4, 1, 30, 136, 1, 32, 1, 0, 0, 0, 0, 0, 0),  # the attention transposes (one row of T positions, Tp > T)
], ids=lambda g: "f16{f16}_s{stride}_d{dy}{dx}_ups{ups}_rp{row_pad}_C{C}".format(**g))
def test_edge_transpose_gather(g):
    check_transpose_gather(g, seed=14)


@pytest.mark.parametrize("g", [
    _g(f16=True, C=40, ld=4096, nseg=64, seg_len=64, scale=0.5, seg_ld=40, colsum=True),
    _g(f16=False, C=24, ld=1000, nseg=3, seg_len=330, scale=1.0, seg_ld=32, colsum=False),   # ld > nseg * seg_len, seg_ld > C
], ids=lambda g: "f16{f16}_C{C}_nseg{nseg}".format(**g))
def test_edge_rowsum_segments_and_colsum(g):
    check_rowsum(g, seed=15)


def _attn_tn(T, N, nh, d, which):
    """the two eod_gemm_tn calls of UNetTrainer._attn_bwd (legacy qkv order): dK = alpha dS^T q and dV = P^T dO"""
    C = nh * d
    Tp = T
    if which == "dk":
        return _g(M=T, N=d, K=T, lda=Tp, ldb=3 * C, ldc=3 * C, alpha=1 / math.sqrt(d), nb0=N, nb1=nh, sa0=nh * T * Tp, sa1=T * Tp,
                  sb0=T * 3 * C, sb1=3 * d, sc0=T * 3 * C, sc1=3 * d, a_mod=0, b_mod=0, c_mod=d)
    return _g(M=T, N=d, K=T, lda=Tp, ldb=C, ldc=3 * C, alpha=1.0, nb0=N, nb1=nh, sa0=nh * T * Tp, sa1=T * Tp, sb0=T * C, sb1=d,
              sc0=T * 3 * C, sc1=3 * d, a_mod=0, b_mod=0, c_mod=2 * d)


@pytest.mark.parametrize("g", [_attn_tn(256, 2, 2, 32, "dk"), _attn_tn(256, 2, 2, 32, "dv")], ids=["T256_dk", "T256_dv"])
def test_edge_gemm_tn(g):
    check_gemm_tn(g, seed=16)


@pytest.mark.parametrize("g", [_attn_tn(4096, 1, 2, 64, "dk"), _attn_tn(4096, 1, 2, 64, "dv"), _attn_tn(16384, 1, 1, 64, "dk")],
                         ids=["T4096_dk", "T4096_dv", "T16384_dk"])
def test_large_gemm_tn(g):
    check_gemm_tn(g, seed=17)


def _nt(f16, cout, cs, Kper, S, Wo, form):
    """the three batched GEMM forms of UNetTrainer._wgrad: 'shift' (dY shifted, negative inner A stride), 'x' (three copies of X read
    at +Wo per row tap), 'taps' (nine tap planes of a stride-2 conv)"""
    ld = S * Kper
    ldp = (cs + 3) // 4 * 4
    if form == "shift":
        yper, margin = cout * ld + 2 * 16, 16
        return _g(f16=f16, M=cout, N=cs, K=Kper, lda=ld, ldb=ld, ldc=ldp, alpha=1.0, nb0=S, nb1=3, sa0=Kper, sa1=-Wo, sb0=Kper, sb1=0,
                  sc0=9 * cout * ldp, sc1=3 * cout * ldp, a_mod=(2 * yper + margin + Wo) % 64, b_mod=margin, c_mod=(2 * cout * ldp) % 64)
    if form == "x":
        return _g(f16=f16, M=cout, N=cs, K=Kper, lda=ld, ldb=ld, ldc=ldp, alpha=1.0, nb0=S, nb1=3, sa0=Kper, sa1=0, sb0=Kper, sb1=Wo,
                  sc0=9 * cout * ldp, sc1=3 * cout * ldp, a_mod=0, b_mod=(16 - Wo) % 64, c_mod=(cout * ldp) % 64)
    per = cs * ld
    return _g(f16=f16, M=cout, N=cs, K=Kper, lda=ld, ldb=ld, ldc=ldp, alpha=1.0, nb0=S, nb1=9, sa0=Kper, sa1=0, sb0=Kper, sb1=per,
              sc0=9 * cout * ldp, sc1=cout * ldp, a_mod=0, b_mod=0, c_mod=0)


@pytest.mark.parametrize("g", [_nt(False, 40, 24, 256, 3, 16, "shift"), _nt(False, 64, 72, 512, 2, 24, "x"), _nt(False, 32, 20, 128, 5, 8, "taps"),
                               _nt(True, 40, 24, 256, 3, 16, "shift"), _nt(True, 72, 128, 512, 4, 8, "x")],
                         ids=["f32_shift", "f32_x", "f32_taps", "f16_shift", "f16_x"])
def test_edge_gemm_nt_backward_weights_forms(g):
    check_gemm_nt(g, seed=18)


@pytest.mark.parametrize("n", [1, 255, 257, 256 * 1024 + 3])
def test_edge_mse_loss(n):
    check_mse(n, seed=19)


def test_large_mse_loss_config5_size():
    check_mse(13 * 512 * 512 * 2, seed=20)
