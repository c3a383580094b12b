"""float64 references of the training-path kernels (csrc/train.hip), of the conv entry point (eod_conv2d_igemm, csrc/igemm.hip) and of
the ops between the convs of the inference forward (resampling, timestep MLP, bound tables: csrc/misc.hip, csrc/norm.hip), in plain torch.

Nothing here imports the library, so the CPU suite can test every reference against torch autograd
(tests/test_ref64.py) and the GPU suite can gate the kernels on references that have themselves been tested
(tests/test_gpu_train_kernels.py, tests/test_gpu_conv_programs.py).  Every function takes tensors on any device, computes in float64 on that
device and returns float64.  Activation tensors are NHWC, as the kernels store them ([N][H][W][C], or [N][HW][C]).

The conv references are per-tap float64 matmuls over shifted, strided or upsampled views of the zero-padded
input: no F.conv2d, so a gate never depends on which convolution backend torch picks.
"""
import torch

F64 = torch.float64


def _pad1(x):
    """NHWC -> one zero pixel on every side of the map"""
    return torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))


def upsample2x(x):
    """nearest 2x of an NHWC map"""
    return x.repeat_interleave(2, 1).repeat_interleave(2, 2)


def conv3x3_weight_grad(dy, x, *, upsample=False, stride=1):
    """dW [Cout][Cin][3][3] of a 3x3 / pad-1 conv y = conv(x') with dy [N][Ho][Wo][Cout], x [N][H][W][Cin]:
    x' = x (stride 1 or 2) or its nearest-2x upsampling (upsample=True, stride 1)
       dW[co][ci][ky][kx] = sum_{n,h,w} dy[n][h][w][co] * x'[n][h*stride + ky - 1][w*stride + kx - 1][ci]"""
    dy, x = dy.to(F64), x.to(F64)
    if upsample:
        x = upsample2x(x)
    N, Ho, Wo, Co = dy.shape
    Ci = x.shape[3]
    xp = _pad1(x)
    a = dy.reshape(-1, Co).t()
    dw = torch.empty((Co, Ci, 3, 3), dtype=F64, device=dy.device)
    for ky in range(3):
        for kx in range(3):
            v = xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride, :]
            dw[:, :, ky, kx] = a @ v.reshape(-1, Ci)
    return dw


def conv1x1_weight_grad(dy, x):
    """dW [Cout][Cin] of a 1x1 conv: sum over pixels of dy[pix][co] * x[pix][ci] (any leading pixel dims)"""
    dy, x = dy.to(F64), x.to(F64)
    return dy.reshape(-1, dy.shape[-1]).t() @ x.reshape(-1, x.shape[-1])


def silu(z):
    return z * torch.sigmoid(z)


def dsilu(z):
    s = torch.sigmoid(z)
    return s * (1.0 + z * (1.0 - s))


def group_norm_stats(x, groups, eps):
    """mean, rstd [N][1][groups][1] of x [N][HW][C] (two-pass, float64)"""
    x = x.to(F64)
    N, HW, C = x.shape
    xg = x.reshape(N, HW, groups, C // groups)
    mean = xg.mean(dim=(1, 3), keepdim=True)
    var = (xg - mean).square().mean(dim=(1, 3), keepdim=True)
    return mean, 1.0 / torch.sqrt(var + eps)


def group_norm_forward(x, gamma, beta, groups, eps, *, silu_out, film=None):
    """y of GroupNorm(groups)(x) [* (1 + s) + t] [-> SiLU] for x [N][HW][C]; film = (s, t), each [N][C]"""
    N, HW, C = x.shape
    mean, rstd = group_norm_stats(x, groups, eps)
    xh = ((x.to(F64).reshape(N, HW, groups, C // groups) - mean) * rstd).reshape(N, HW, C)
    z = xh * gamma.to(F64) + beta.to(F64)
    if film is not None:
        z = z * (1.0 + film[0].to(F64)[:, None, :]) + film[1].to(F64)[:, None, :]
    return silu(z) if silu_out else z


def group_norm_scale_shift(x, gamma, beta, groups, eps, film=None):
    """the forward's folded table [N][C][2]: y_pre_silu = x * scale + shift"""
    N, HW, C = x.shape
    mean, rstd = group_norm_stats(x, groups, eps)
    cpg = C // groups
    mean_c = mean.reshape(N, groups, 1).expand(N, groups, cpg).reshape(N, C)
    rstd_c = rstd.reshape(N, groups, 1).expand(N, groups, cpg).reshape(N, C)
    g, b = gamma.to(F64)[None, :], beta.to(F64)[None, :]
    sc, sh = rstd_c * g, b - mean_c * rstd_c * g
    if film is not None:
        fs = 1.0 + film[0].to(F64)
        sc, sh = sc * fs, sh * fs + film[1].to(F64)
    return torch.stack([sc, sh], -1)


def group_norm_backward(x, dy, gamma, beta, groups, eps, *, silu_out, film=None):
    """closed-form backward of group_norm_forward: returns (dx [N][HW][C], dgamma [C], dbeta [C], dfilm [N][2C] or None),
    dfilm[n] = [d scale | d shift]"""
    x, dy = x.to(F64), dy.to(F64)
    g, b = gamma.to(F64), beta.to(F64)
    N, HW, C = x.shape
    cpg = C // groups
    mean, rstd = group_norm_stats(x, groups, eps)
    xhg = (x.reshape(N, HW, groups, cpg) - mean) * rstd
    xh = xhg.reshape(N, HW, C)
    zpre = xh * g + b
    fs = 1.0
    z = zpre
    if film is not None:
        fs = 1.0 + film[0].to(F64)[:, None, :]
        z = zpre * fs + film[1].to(F64)[:, None, :]
    dz = dy * dsilu(z) if silu_out else dy
    dfilm = torch.cat([(dz * zpre).sum(1), dz.sum(1)], 1) if film is not None else None
    dzpre = dz * fs
    dgamma = (dzpre * xh).sum((0, 1))
    dbeta = dzpre.sum((0, 1))
    dxh = (dzpre * g).reshape(N, HW, groups, cpg)
    dx = rstd * (dxh - dxh.mean((1, 3), keepdim=True) - xhg * (dxh * xhg).mean((1, 3), keepdim=True))
    return dx.reshape(N, HW, C), dgamma, dbeta, dfilm


def channel_sums(g, scale):
    """per-channel sums of a gradient g [N][HW][C] (or per-slab sums [N][P][C]): (dbias [C] = scale * sum over n and pixels,
    demb [N][C] = per-image sums, unscaled) -- what eod_channel_sums_finish returns"""
    s = g.to(F64).sum(1)
    return scale * s.sum(0), s


def sinusoid(t, freqs, K):
    """the timestep embedding [N][K] as the kernels form it: [cos(t f) | sin(t f) (| 0 if K is odd)].  The argument t * f is
    rounded to fp32 first, as every fp32 implementation forms it: that rounding is part of the input, not of the kernel"""
    half = K // 2
    arg = (t.to(torch.float32)[:, None] * freqs.to(torch.float32)[None, :half]).to(F64)
    out = [torch.cos(arg), torch.sin(arg)]
    if K % 2:
        out.append(torch.zeros((t.shape[0], 1), dtype=F64, device=t.device))
    return torch.cat(out, 1)


def linear_backward(dout, inp, w, *, act_in, scale, pre=None):
    """dense layer out = a(in) W^T + b, a = identity (act_in 0) / SiLU (1) / `inp` already the activated input (2, the sinusoid):
    returns (dW [J][K] * scale, db [J] * scale, din [N][K] (* SiLU'(pre) if pre is given))"""
    dout, w = dout.to(F64), w.to(F64)
    a = inp.to(F64)
    if act_in == 1:
        a = silu(a)
    din = dout @ w
    if pre is not None:
        din = din * dsilu(pre.to(F64))
    return scale * (dout.t() @ a), scale * dout.sum(0), din


def temb_pre1(t, freqs, w1, b1):
    """pre-activation of time_embed[0]: sinusoid(t) W1^T + b1"""
    return sinusoid(t, freqs, w1.shape[1]) @ w1.to(F64).t() + b1.to(F64)


def embedding_backward(dout, y, classes, scale):
    """nn.Embedding backward: dW[c] = scale * sum of the rows dout[n] with y[n] == c (zero rows for unused classes)"""
    dw = torch.zeros((classes, dout.shape[1]), dtype=F64, device=dout.device)
    return scale * dw.index_add_(0, y.long(), dout.to(F64))


def transpose_gather(src, ld_dst, Ho, Wo, stride, pad, dy, dx, ups, row_pad):
    """eod_transpose_gather in the source dtype, exactly: [C][ld_dst], column k = (n*(Ho + 2 row_pad) + ho + row_pad)*Wo + wo
    holds src'[n][ho*stride - pad + dy][wo*stride - pad + dx] (src' = src or its nearest-2x upsampling), +0 outside the image,
    in the pad rows and in the tail columns K .. ld_dst-1"""
    N, H, W, C = src.shape
    img = upsample2x(src) if ups else src
    He, We = img.shape[1], img.shape[2]
    dev = src.device
    hi = torch.arange(Ho, device=dev) * stride - pad + dy
    wi = torch.arange(Wo, device=dev) * stride - pad + dx
    g = img[:, hi.clamp(0, He - 1)][:, :, wi.clamp(0, We - 1)]
    ok = ((hi >= 0) & (hi < He))[:, None] & ((wi >= 0) & (wi < We))[None, :]
    g = torch.where(ok[None, :, :, None], g, torch.zeros((), dtype=src.dtype, device=dev))
    full = torch.zeros((N, Ho + 2 * row_pad, Wo, C), dtype=src.dtype, device=dev)
    full[:, row_pad:row_pad + Ho] = g
    K = N * (Ho + 2 * row_pad) * Wo
    out = torch.zeros((C, ld_dst), dtype=src.dtype, device=dev)
    out[:, :K] = full.reshape(K, C).t()
    return out


def rowsum_segments(x, nseg, seg_len, scale):
    """seg [nseg][C] = scale * sums of x [C][ld] over the segments [s*seg_len, (s+1)*seg_len)"""
    C = x.shape[0]
    return scale * x[:, :nseg * seg_len].to(F64).reshape(C, nseg, seg_len).sum(-1).t()


def gemm_tn(a, b, *, M, N, K, lda, ldb, alpha, nb0, nb1, sa, sb, a_off=0, b_off=0):
    """eod_gemm_tn on flat buffers: C[b0][b1][m][n] = alpha * sum_k A[k][m] * B[k][n], both operands K-major"""
    a64, b64 = a.to(F64), b.to(F64)
    out = []
    for b1 in range(nb1):
        A = a64.as_strided((nb0, K, M), (sa[0], lda, 1), a_off + b1 * sa[1])
        B = b64.as_strided((nb0, K, N), (sb[0], ldb, 1), b_off + b1 * sb[1])
        out.append(alpha * (A.transpose(1, 2) @ B))
    return torch.stack(out, 1)


def gemm_nt(a, b, *, M, N, K, lda, ldb, alpha, nb0, nb1, sa, sb, a_off=0, b_off=0):
    """eod_gemm_nt on flat buffers: C[b0][b1][m][n] = alpha * sum_k A[m][k] * B[n][k] (inner batch strides may be negative)"""
    a64, b64 = a.to(F64), b.to(F64)
    out = []
    for b1 in range(nb1):
        A = a64.as_strided((nb0, M, K), (sa[0], lda, 1), a_off + b1 * sa[1])
        B = b64.as_strided((nb0, N, K), (sb[0], ldb, 1), b_off + b1 * sb[1])
        out.append(alpha * (A @ B.transpose(1, 2)))
    return torch.stack(out, 1)


def mse_loss(pred, target):
    """nn.MSELoss(reduction='mean'): (loss, dLoss/dpred)"""
    d = pred.to(F64) - target.to(F64)
    return d.square().mean(), 2.0 * d / d.numel()


# ================================================================================================ eod_conv2d_igemm (include/eodiff.h)
def zero_insert2x(x):
    """upsample = 2: z[2i][2j] = x[i][j] on a (2H x 2W) map, zeros elsewhere"""
    N, H, W, C = x.shape
    z = torch.zeros((N, 2 * H, 2 * W, C), dtype=x.dtype, device=x.device)
    z[:, ::2, ::2] = x
    return z


def conv_input(x, x2=None, *, upsample=0, pad_tl=0, gn_scale_shift=None, gn_silu=False):
    """the A operand of the conv as the kernel sees it, NHWC float64: virtual concat x | x2, input GroupNorm from the {scale, shift}
    table [N][C0+C1][2] (a = x * scale + shift, optional SiLU), then the virtual upsampling (1 / 3: nearest 2x, 2: zero insertion) and
    the extra zero row / column on top / left (pad_tl)"""
    a = x.to(F64) if x2 is None else torch.cat([x.to(F64), x2.to(F64)], -1)
    if gn_scale_shift is not None:
        ss = gn_scale_shift.to(F64)
        a = a * ss[:, None, None, :, 0] + ss[:, None, None, :, 1]
        if gn_silu:
            a = silu(a)
    if upsample in (1, 3):
        a = upsample2x(a)
    elif upsample == 2:
        a = zero_insert2x(a)
    else:
        assert upsample == 0, upsample
    if pad_tl:
        a = torch.nn.functional.pad(a, (0, 0, 1, 0, 1, 0))
    return a


def _taps(a, w, ksize, stride, pad):
    """sum over taps of (shifted, strided view of the zero-padded NHWC map a) @ w[:, :, ky, kx]^T"""
    N, H, W, C = a.shape
    Ho, Wo = (H + 2 * pad - ksize) // stride + 1, (W + 2 * pad - ksize) // stride + 1
    ap = torch.nn.functional.pad(a, (0, 0, pad, pad, pad, pad)) if pad else a
    w = w.reshape(w.shape[0], C, ksize, ksize)
    y = torch.zeros((N, Ho, Wo, w.shape[0]), dtype=F64, device=a.device)
    for ky in range(ksize):
        for kx in range(ksize):
            v = ap[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride, :]
            y += v @ w[:, :, ky, kx].t()
    return y


def block_sum2x2(g):
    N, H, W, C = g.shape
    return g.reshape(N, H // 2, 2, W // 2, 2, C).sum((2, 4))


def up4_class_kernels(w_oihw):
    """the [4 Cout][Cin][3][3] class-kernel tensor of the parity-class form (include/eodiff.h, eod_conv_up4_ok): output pixel
    (2i + p, 2j + q) of the 3x3 conv over the nearest-2x image reads stored rows {i - 1 + p, i + p} only, with the taps that meet the
    same stored pixel summed (p = 0: [w0 | w1 + w2], p = 1: [w0 + w1 | w2]; columns alike).  Row block 2p + q holds class (p, q)'s
    kernel in the tap slots dy' in {p, p + 1}, dx' in {q, q + 1}, zeros elsewhere."""
    w = w_oihw.to(F64)
    Cout = w.shape[0]
    sums = {0: [[0], [1, 2]], 1: [[0, 1], [2]]}
    wc = torch.zeros((4 * Cout,) + tuple(w.shape[1:]), dtype=F64, device=w.device)
    for p in (0, 1):
        for q in (0, 1):
            for a, rows in enumerate(sums[p]):
                for b, cols in enumerate(sums[q]):
                    wc[(2 * p + q) * Cout:(2 * p + q + 1) * Cout, :, p + a, q + b] = w[:, :, rows][:, :, :, cols].sum((2, 3))
    return wc


def space_to_depth2(x):
    """[N][2H][2W][C] -> [N][H][W][4C], channel (2p + q) C + c of pixel (i, j) = x[2i + p][2j + q][c]"""
    N, H2, W2, C = x.shape
    return x.reshape(N, H2 // 2, 2, W2 // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, H2 // 2, W2 // 2, 4 * C)


def conv_forward(x, x2, w_oihw, *, ksize, stride=1, pad=1, upsample=0, pad_tl=0, gn_scale_shift=None, gn_silu=False, alpha=1.0, bias=None,
                 cbias=None, cbias_stride=0, res=None, skip_x=None, skip_x2=None, skip_w=None, absolute=False, class_w=None):
    """y [N][Ho][Wo][Cout] float64 of eod_conv2d_igemm:
        y = alpha * (sum_{tap, c} A(n, ho*stride - pad + dy, wo*stride - pad + dx, c) * w[co][c][dy][dx] + sum_c skip_w[co][c] * X(n, ho, wo, c))
            + bias[co] + cbias[n * cbias_stride + co] + res[n][ho][wo][co]
    with A = conv_input(...) and X = skip_x | skip_x2 at the output resolution (the fused 1x1 skip conv shares the accumulator).
    upsample = 4 is the backward-data of the nearest-2x conv: x = dY [N][2 Ho][2 Wo][C0], w_oihw = the FORWARD conv's weight
    [C0][Cout][3][3], y = dX = the 2 x 2 block sum of the transposed conv of dY on the fine grid.
    class_w (upsample 3 and 4 only): the class-kernel tensor [4 rows][cols][3][3] (up4_class_kernels of the forward weight) AS THE KERNEL
    GETS IT, e.g. rounded to fp16 after the tap sums: the same function computed class by class from it instead of from w_oihw -- four
    plain 3x3 convs of the stored map (upsample 3), one 3x3 conv of the 2 x 2 space-to-depth view of dY (upsample 4).
    absolute = True: every term replaced by its absolute value (conv_abs_bound)."""
    ab = (lambda t: t.abs()) if absolute else (lambda t: t)
    w = None if w_oihw is None else ab(w_oihw.to(F64))
    if class_w is not None:
        assert upsample in (3, 4) and ksize == 3 and stride == 1 and pad == 1 and not pad_tl and x2 is None and gn_scale_shift is None
        wc = ab(class_w.to(F64))
        if upsample == 3:
            N, H, W, _ = x.shape
            Cout = wc.shape[0] // 4
            y = torch.empty((N, 2 * H, 2 * W, Cout), dtype=F64, device=x.device)
            for p in (0, 1):
                for q in (0, 1):
                    y[:, p::2, q::2] = _taps(ab(x.to(F64)), wc[(2 * p + q) * Cout:(2 * p + q + 1) * Cout], 3, 1, 1)
        else:
            y = _taps(space_to_depth2(ab(x.to(F64))), wc.flip(2, 3).transpose(0, 1), 3, 1, 1)
    elif upsample == 4:
        assert ksize == 3 and stride == 1 and pad == 1 and not pad_tl and x2 is None and gn_scale_shift is None
        # dfine[i][j][ci] = sum_{ky, kx, co} dY[i + 1 - ky][j + 1 - kx][co] * w[co][ci][ky][kx]: a 3x3 conv with the flipped, transposed weight
        y = block_sum2x2(_taps(ab(x.to(F64)), w.flip(2, 3).transpose(0, 1), 3, 1, 1))
    else:
        a = conv_input(x, x2, upsample=upsample, pad_tl=pad_tl, gn_scale_shift=gn_scale_shift, gn_silu=gn_silu)
        y = _taps(ab(a), w, ksize, stride, pad)
    if skip_x is not None:
        xs = skip_x.to(F64) if skip_x2 is None else torch.cat([skip_x.to(F64), skip_x2.to(F64)], -1)
        y = y + ab(xs) @ ab(skip_w.to(F64)).reshape(y.shape[-1], -1).t()
    y = y * abs(alpha) if absolute else y * alpha
    N, Cout = y.shape[0], y.shape[-1]
    if bias is not None:
        y = y + ab(bias.to(F64))
    if cbias is not None:
        idx = torch.arange(N, device=y.device)[:, None] * cbias_stride + torch.arange(Cout, device=y.device)[None, :]
        y = y + ab(cbias.to(F64).flatten()[idx])[:, None, None, :]
    if res is not None:
        y = y + ab(res.to(F64))
    return y


def conv_abs_bound(x, x2, w_oihw, **kw):
    """the sum of conv_forward with every term replaced by its absolute value: sum |a| |w| + |bias| + |cbias| + |res| (+ the skip term
    likewise).  It scales the element-wise error metric and does not shrink where the true sum cancels."""
    return conv_forward(x, x2, w_oihw, absolute=True, **kw)


def stats_of(y):
    """[N][C][2] float64: per (image, channel) sum and sum of squares of an NHWC tensor"""
    y = y.to(F64).flatten(1, -2)
    return torch.stack([y.sum(1), y.square().sum(1)], -1)


AB_KMIN, AB_KMAX, AB_KMIN_ATTN = -113, 60, -48  # csrc/common.h


def presplit_scale(bound, kmin=AB_KMIN):
    """the power-of-two operand scale s_n a bound table [N][32] implies (csrc/common.h): B_n = the row maximum (NaN counts as inf),
    s_n = 2^k with k = 14 - floor(log2 B_n), clamped to [kmin, 60], so that B_n * s_n lies in [2^14, 2^15).  float64 [N]"""
    b = bound.float()
    b = torch.where(b == b, b, torch.full_like(b, float("inf"))).max(1).values.contiguous()
    eb = (b.view(torch.int32) >> 23) & 0xff
    k = (141 - eb).clamp(kmin, AB_KMAX)
    return torch.pow(torch.tensor(2.0, dtype=F64, device=bound.device), k.to(F64))


def presplit_encode(x, s):
    """the pre-split layout: x [N][...][C] (C % 8 == 0), s [N] -> a float32-typed tensor of the same shape whose
    every 8 channels hold [8 x fp16 hi | 8 x fp16 lo] with hi = fp16(s_n x), lo = fp16(s_n x - hi)"""
    assert x.shape[-1] % 8 == 0
    v = x.to(F64) * s.to(F64).reshape((-1,) + (1,) * (x.dim() - 1))
    hi = v.to(torch.float16)
    lo = (v - hi.to(F64)).to(torch.float16)
    shp = x.shape[:-1] + (x.shape[-1] // 8, 8)
    packed = torch.cat([hi.reshape(shp), lo.reshape(shp)], -1).contiguous()
    return packed.view(torch.float32).reshape(x.shape)


def presplit_decode(p, s):
    """inverse of presplit_encode: (hi + lo) / s_n in float64"""
    h = p.contiguous().view(torch.float16).reshape(p.shape[:-1] + (p.shape[-1] // 8, 16)).to(F64)
    v = (h[..., :8] + h[..., 8:]).reshape(p.shape)
    return v / s.to(F64).reshape((-1,) + (1,) * (p.dim() - 1))


# ================================================================================================ glue ops of the inference forward
def resample2x(x, mode, pad_tl=0):
    """eod_resample2x on an NHWC map, float64.  mode 0: 2x2 average pool (an odd map drops its last row / column); 1: nearest 2x with
    pad_tl zero rows / columns on top / left; 2: the adjoint of mode 1 (2x2 sums that skip the first pad_tl rows / columns); 3: nearest
    2x times 0.25 with pad_tl zero rows / columns at the bottom / right (the adjoint of mode 0; pad_tl = 1 for a map odd in BOTH axes);
    4: crop of the last row (pad_tl & 1) and / or column (pad_tl & 2)"""
    x = x.to(F64)
    N, H, W, C = x.shape
    if mode == 0:
        return block_sum2x2(x[:, :H // 2 * 2, :W // 2 * 2]) * 0.25
    if mode == 1:
        return torch.nn.functional.pad(upsample2x(x), (0, 0, pad_tl, 0, pad_tl, 0))
    if mode == 2:
        x = x[:, pad_tl:, pad_tl:]
        return block_sum2x2(x[:, :x.shape[1] // 2 * 2, :x.shape[2] // 2 * 2])
    if mode == 3:
        return torch.nn.functional.pad(upsample2x(x) * 0.25, (0, 0, 0, pad_tl, 0, pad_tl))
    assert mode == 4, mode
    return x[:, :H - (pad_tl & 1), :W - ((pad_tl >> 1) & 1)]


def time_embed(t, freqs, w1, b1, w2, b2, wcat, bcat, *, label_emb=None, y=None, emb=None):
    """the three stages of eod_time_embed: h1 = SiLU(sinusoid(t) W1^T + b1), emb = h1 W2^T + b2 (+ label_emb[y]),
    out = SiLU(emb) Wcat^T + bcat.  w1 = None: `emb` is the input and only stage 3 runs.  wcat = None: no stage 3.
    Returns (h1, emb, out), float64 (None for a stage that did not run)"""
    h1 = None
    if w1 is not None:
        h1 = silu(temb_pre1(t, freqs, w1, b1))
        emb = h1 @ w2.to(F64).t() + b2.to(F64)
        if label_emb is not None:
            emb = emb + label_emb.to(F64)[y.long()]
    else:
        emb = emb.to(F64)
    out = None if wcat is None else silu(emb) @ wcat.to(F64).t() + bcat.to(F64)
    return h1, emb, out


AB = 32  # entries per image of a bound table (csrc/common.h: EOD_AB)


def act_bound_ranges(L):
    """[(i0, i1)] * 32: block j of eod_act_bound covers the items [L j / 32, L (j + 1) / 32) of an image's L items (16-byte chunks in
    direct mode, {sum, sumsq} pairs in parts mode); a range may be empty"""
    return [(L * j // AB, L * (j + 1) // AB) for j in range(AB)]


def _inf_if_nonfinite(v):
    return torch.where(torch.isfinite(v), v, torch.full_like(v, float("inf")))


def act_bound_direct(x, epc):
    """[N][32] float64: entry j = max|x| over the j-th range of 16-byte chunks (epc elements each) of image n, x [N][per_image];
    0 for an empty range, +inf where the range holds a NaN or an inf"""
    x = x.to(F64).flatten(1)
    out = torch.zeros((x.shape[0], AB), dtype=F64, device=x.device)
    for j, (i0, i1) in enumerate(act_bound_ranges(x.shape[1] // epc)):
        if i1 > i0:
            out[:, j] = _inf_if_nonfinite(x[:, i0 * epc:i1 * epc].abs()).max(1).values
    return out


def act_bound_parts(parts):
    """[N][32] float64: entry j = sqrt of the largest sum of squares among the j-th range of {sum, sumsq} pairs of every source in
    `parts` (each [N][P][C][2]); a NaN sum of squares counts as +inf"""
    N = parts[0].shape[0]
    out = torch.zeros((N, AB), dtype=F64, device=parts[0].device)
    for p in parts:
        q = p.to(F64).reshape(N, -1, 2)[:, :, 1]
        q = torch.where(q == q, q, torch.full_like(q, float("inf")))
        for j, (i0, i1) in enumerate(act_bound_ranges(q.shape[1])):
            if i1 > i0:
                out[:, j] = torch.maximum(out[:, j], q[:, i0:i1].max(1).values)
    return out.sqrt()


def linear_bound(w, b=None):
    """(max row L1 norm of w [rows][cols], max|b| or 0): |W x + b| <= coef0 * max|x| + coef1 (eod_weight_l1max, without its safety
    factor)"""
    return float(w.to(F64).abs().sum(1).max()), 0.0 if b is None else float(b.to(F64).abs().max())


# ================================================================================================ attention (csrc/attn*.hip), softmax rows
def head_slices(t, heads, d, off, head_stride):
    """[N][T][*] -> [N][heads][T][d] float64: channels off + h * head_stride + (0 .. d - 1) of every head (legacy order [h][q|k|v][d]:
    off = 0 / d / 2d, head_stride = 3d; new order [q|k|v][h][d]: off = 0 / C / 2C, head_stride = d)"""
    return torch.stack([t[..., off + h * head_stride: off + h * head_stride + d] for h in range(heads)], 1).to(F64)


def attention_forward(qkv, heads, d, q_off, k_off, v_off, head_stride):
    """QKVAttention(Legacy) on the natural layout qkv [N][T][3C]: P = softmax_s(q_t . k_s / sqrt(d)), out = P v.
    -> out [N][T][C], lse [N][heads][T] (natural log), P [N][heads][T][T], all float64"""
    N, T = qkv.shape[:2]
    q, k, v = (head_slices(qkv, heads, d, o, head_stride) for o in (q_off, k_off, v_off))
    S = (q @ k.transpose(-1, -2)) / float(d) ** 0.5
    m = S.amax(-1, keepdim=True)
    E = torch.exp(S - m)
    l = E.sum(-1, keepdim=True)
    P = E / l
    lse = (m + torch.log(l)).squeeze(-1)
    out = (P @ v).permute(0, 2, 1, 3).reshape(N, T, heads * d)
    return out, lse, P


def attention_backward(qkv, dO, heads, d, q_off, k_off, v_off, head_stride):
    """the gradient of attention_forward's `out` with respect to qkv for the output gradient dO [N][T][C]:
    dV = P^T dO, dP = dO v^T, D = rowsum(dP * P) (= sum_j dO * out), dS = P * (dP - D), dQ = dS k / sqrt(d), dK = dS^T q / sqrt(d).
    -> dqkv [N][T][3C] (channels outside the q / k / v slices are zero), D [N][heads][T], float64"""
    N, T = qkv.shape[:2]
    q, k, v = (head_slices(qkv, heads, d, o, head_stride) for o in (q_off, k_off, v_off))
    _, _, P = attention_forward(qkv, heads, d, q_off, k_off, v_off, head_stride)
    g = head_slices(dO, heads, d, 0, d)
    dV = P.transpose(-1, -2) @ g
    dP = g @ v.transpose(-1, -2)
    D = (dP * P).sum(-1)
    dS = P * (dP - D[..., None])
    a = 1.0 / float(d) ** 0.5
    dQ, dK = a * (dS @ k), a * (dS.transpose(-1, -2) @ q)
    dqkv = torch.zeros(qkv.shape, dtype=F64, device=qkv.device)
    for h in range(heads):
        for off, t in ((q_off, dQ), (k_off, dK), (v_off, dV)):
            dqkv[..., off + h * head_stride: off + h * head_stride + d] = t[:, h]
    return dqkv, D


def softmax_rows(s, n):
    """eod_softmax_rows: softmax over the first n columns of every row of s [rows][lds] -> [rows][n] float64"""
    z = s[:, :n].to(F64)
    e = torch.exp(z - z.amax(1, keepdim=True))
    return e / e.sum(1, keepdim=True)


def softmax_backward_rows(P, dP, n):
    """eod_softmax_bwd_rows: dS = P * (dP - sum_k dP P) over the first n columns -> [rows][n] float64"""
    p, g = P[:, :n].to(F64), dP[:, :n].to(F64)
    return p * (g - (g * p).sum(1, keepdim=True))


def rowdot(a, b, n0, n1, n2, s0, s1, s2, d):
    """eod_rowdot: out[i0][i1][i2] = sum_{j < d} a[off + j] b[off + j], off = i0 s0 + i1 s1 + i2 s2 (elements of the flat tensors)"""
    dev = a.device
    i0, i1, i2 = (torch.arange(n, device=dev) for n in (n0, n1, n2))
    off = i0[:, None, None] * s0 + i1[None, :, None] * s1 + i2[None, None, :] * s2
    idx = off[..., None] + torch.arange(d, device=dev)
    return (a.reshape(-1).to(F64)[idx] * b.reshape(-1).to(F64)[idx]).sum(-1)


def attention_pack(qkv, heads, d, dpad, ldt, new_order):
    """the operands of eod_attention_fwd, gathered from the natural layout qkv [N][T][3C] the way AttentionBlock._row_maps gathers the
    rows of the projection weight: qk [N * T][2 * heads * dpad] = [q: heads x dpad | k: heads x dpad] with every head zero-padded from d
    to dpad channels, and vT [N][C][ldt] = v transposed (head-major channels, keys contiguous, zero beyond T).  Same dtype as qkv"""
    N, T = qkv.shape[:2]
    C = heads * d
    base = (lambda which, h: which * C + h * d) if new_order else (lambda which, h: h * 3 * d + which * d)
    qk = torch.zeros((N * T, 2 * heads * dpad), dtype=qkv.dtype, device=qkv.device)
    flat = qkv.reshape(N * T, 3 * C)
    for which in (0, 1):
        for h in range(heads):
            c0 = (which * heads + h) * dpad
            qk[:, c0: c0 + d] = flat[:, base(which, h): base(which, h) + d]
    vT = torch.zeros((N, C, ldt), dtype=qkv.dtype, device=qkv.device)
    for h in range(heads):
        vT[:, h * d: (h + 1) * d, :T] = qkv[:, :, base(2, h): base(2, h) + d].transpose(1, 2)
    return qk, vT
