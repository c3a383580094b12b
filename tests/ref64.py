"""float64 references of the training-path kernels (csrc/train.hip), in plain torch.

Nothing here imports the library, so the CPU suite can test every reference against torch autograd
(tests/test_ref64.py) and the GPU suite can gate the kernels on references that have themselves been tested
(tests/test_gpu_train_kernels.py).  Every function takes tensors on any device, computes in float64 on that
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
