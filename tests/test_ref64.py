"""CPU: the float64 references of tests/ref64.py against torch autograd in float64 (conv2d weight gradients, F.group_norm, nn.Linear,
nn.Embedding, nn.MSELoss) at small shapes, so that the GPU gates of tests/test_gpu_train_kernels.py rest on references that have been
tested themselves."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import ref64

D = torch.float64


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, seed, scale=1.0):
    return scale * torch.randn(shape, generator=_g(seed), dtype=D)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _close(a, b, tol=1e-12):
    a, b = a.to(D), b.to(D)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = float((a - b).norm() / b.norm().clamp_min(1e-300))
    assert err < tol, err


@pytest.mark.parametrize("N,Cin,H,W,Cout,mode", [(2, 5, 6, 7, 4, "plain"), (1, 3, 4, 5, 6, "up"), (2, 4, 8, 6, 3, "s2"), (3, 2, 1, 1, 2, "plain"),
                                                 (1, 2, 2, 2, 3, "up"), (1, 3, 2, 4, 2, "s2")])
def test_conv3x3_weight_grad_matches_autograd(N, Cin, H, W, Cout, mode):
    x = _randn((N, Cin, H, W), 1)
    xin = F.interpolate(x, scale_factor=2, mode="nearest") if mode == "up" else x
    stride = 2 if mode == "s2" else 1
    Ho, Wo = (xin.shape[2] - 1) // stride + 1, (xin.shape[3] - 1) // stride + 1
    dy = _randn((N, Cout, Ho, Wo), 2)
    ref = torch.nn.grad.conv2d_weight(xin, (Cout, Cin, 3, 3), dy, stride=stride, padding=1)
    got = ref64.conv3x3_weight_grad(_nhwc(dy), _nhwc(x), upsample=(mode == "up"), stride=stride)
    _close(got, ref)


def test_conv1x1_weight_grad_matches_autograd():
    x, dy = _randn((2, 6, 5, 3), 3), _randn((2, 4, 5, 3), 4)
    ref = torch.nn.grad.conv2d_weight(x, (4, 6, 1, 1), dy)[:, :, 0, 0]
    _close(ref64.conv1x1_weight_grad(_nhwc(dy), _nhwc(x)), ref)


@pytest.mark.parametrize("N,C,H,W,groups", [(2, 8, 3, 5, 4), (1, 12, 4, 4, 3), (3, 6, 1, 2, 2)])
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("film", [False, True])
def test_group_norm_backward_matches_autograd(N, C, H, W, groups, silu, film):
    eps = 1e-5
    x = (_randn((N, C, H, W), 5, 1.5) + 0.3).requires_grad_(True)
    gam = (1.0 + 0.2 * _randn((C,), 6)).requires_grad_(True)
    bet = (0.1 * _randn((C,), 7)).requires_grad_(True)
    s = (0.3 * _randn((N, C), 8)).requires_grad_(True)
    t = (0.2 * _randn((N, C), 9)).requires_grad_(True)
    dy = _randn((N, C, H, W), 10)
    y = F.group_norm(x, groups, gam, bet, eps=eps)
    if film:
        y = y * (1 + s[:, :, None, None]) + t[:, :, None, None]
    if silu:
        y = F.silu(y)
    y.backward(dy)
    flat = lambda v: v.detach().permute(0, 2, 3, 1).reshape(N, H * W, C)
    fl = (s.detach(), t.detach()) if film else None
    fwd = ref64.group_norm_forward(flat(x), gam.detach(), bet.detach(), groups, eps, silu_out=silu, film=fl)
    _close(fwd, flat(y))
    dx, dgam, dbet, dfilm = ref64.group_norm_backward(flat(x), flat(dy), gam.detach(), bet.detach(), groups, eps, silu_out=silu, film=fl)
    _close(dx, flat(x.grad), 1e-11)
    _close(dgam, gam.grad)
    _close(dbet, bet.grad)
    if film:
        _close(dfilm, torch.cat([s.grad, t.grad], 1))
    else:
        assert dfilm is None
    ss = ref64.group_norm_scale_shift(flat(x), gam.detach(), bet.detach(), groups, eps, film=fl)
    pre = flat(x) * ss[:, None, :, 0] + ss[:, None, :, 1]
    _close(ref64.silu(pre) if silu else pre, flat(y))


def test_channel_sums():
    g = _randn((3, 7, 5), 11)
    dbias, demb = ref64.channel_sums(g, 0.25)
    _close(dbias, 0.25 * g.sum((0, 1)))
    _close(demb, g.sum(1))


@pytest.mark.parametrize("act_in", [0, 1, 2])
@pytest.mark.parametrize("with_pre", [False, True])
def test_linear_backward_matches_autograd(act_in, with_pre):
    N, K, J, scale = 3, 7, 5, 0.125
    freqs = torch.exp(-math.log(10000.0) * torch.arange(K // 2, dtype=torch.float32) / (K // 2))
    t = torch.tensor([0, 17, 999])
    inp = ref64.sinusoid(t, freqs, K) if act_in == 2 else _randn((N, K), 12)
    pre = _randn((N, K), 13) if with_pre else None
    lin = torch.nn.Linear(K, J).double()
    xin = inp.clone().requires_grad_(True)
    out = lin(F.silu(xin) if act_in == 1 else xin)
    dout = _randn((N, J), 14)
    out.backward(dout)
    dW, db, din = ref64.linear_backward(dout, inp, lin.weight.detach(), act_in=act_in, scale=scale, pre=pre)
    _close(dW, scale * lin.weight.grad)
    _close(db, scale * lin.bias.grad)
    want = (dout @ lin.weight.detach()) * (ref64.dsilu(pre) if with_pre else 1.0)
    _close(din, want)
    if not with_pre and act_in == 0:
        _close(din, xin.grad)
    if with_pre:  # din * SiLU'(pre) is the gradient w.r.t. pre of a layer whose input was SiLU(pre)
        p = pre.clone().requires_grad_(True)
        (lin(F.silu(p)) * dout).sum().backward()
        _close(din, p.grad)


def test_sinusoid_odd_width_and_temb_pre1():
    t = torch.tensor([3, 500])
    freqs = torch.tensor([1.0, 0.1, 0.01], dtype=torch.float32)
    s = ref64.sinusoid(t, freqs, 7)
    assert s.shape == (2, 7) and bool((s[:, 6] == 0).all())
    arg = (t.float()[:, None] * freqs[None, :]).double()
    _close(s[:, :3], torch.cos(arg))
    _close(s[:, 3:6], torch.sin(arg))
    w1, b1 = _randn((4, 7), 15), _randn((4,), 16)
    _close(ref64.temb_pre1(t, freqs, w1, b1), torch.nn.functional.linear(s, w1, b1))


def test_embedding_backward_matches_autograd():
    emb = torch.nn.Embedding(6, 4).double()
    y = torch.tensor([2, 0, 2, 5, 2])
    dout = _randn((5, 4), 17)
    emb(y).backward(dout)
    got = ref64.embedding_backward(dout, y, 6, 0.5)
    _close(got, 0.5 * emb.weight.grad)
    assert bool((got[[1, 3, 4]] == 0).all())


@pytest.mark.parametrize("stride,pad,dy,dx,ups,row_pad,extra", [(1, 1, 0, 2, 0, 1, 8), (2, 1, 2, 0, 0, 0, 0), (1, 1, 1, 1, 1, 0, 16), (1, 0, 0, 0, 0, 0, 4)])
def test_transpose_gather_by_loops(stride, pad, dy, dx, ups, row_pad, extra):
    N, H, W, C = 2, 3, 4, 3
    src = torch.arange(1, N * H * W * C + 1, dtype=torch.float32).reshape(N, H, W, C)
    He, We = (2 * H, 2 * W) if ups else (H, W)
    Ho, Wo = (He + 2 * pad - 3) // stride + 1 if pad else He, (We + 2 * pad - 3) // stride + 1 if pad else We
    K = N * (Ho + 2 * row_pad) * Wo
    got = ref64.transpose_gather(src, K + extra, Ho, Wo, stride, pad, dy, dx, ups, row_pad)
    want = torch.zeros((C, K + extra))
    for n in range(N):
        for ho in range(Ho):
            for wo in range(Wo):
                hi, wi = ho * stride - pad + dy, wo * stride - pad + dx
                if 0 <= hi < He and 0 <= wi < We:
                    k = (n * (Ho + 2 * row_pad) + ho + row_pad) * Wo + wo
                    want[:, k] = src[n, hi // 2 if ups else hi, wi // 2 if ups else wi]
    assert torch.equal(got, want)


def test_rowsum_segments():
    x = _randn((3, 20), 18)
    got = ref64.rowsum_segments(x, 3, 6, 2.0)
    _close(got, 2.0 * torch.stack([x[:, 6 * s:6 * s + 6].sum(1) for s in range(3)]))


def test_gemm_tn_and_gemm_nt_on_strided_buffers():
    M, N, K, nb0, nb1 = 3, 4, 5, 2, 3
    a, b = _randn((400,), 19), _randn((400,), 20)
    lda, ldb, sa, sb = 8, 9, (120, 11), (130, 7)
    got = ref64.gemm_tn(a, b, M=M, N=N, K=K, lda=lda, ldb=ldb, alpha=0.5, nb0=nb0, nb1=nb1, sa=sa, sb=sb, a_off=3, b_off=1)
    for b0 in range(nb0):
        for b1 in range(nb1):
            A = torch.stack([a[3 + b0 * sa[0] + b1 * sa[1] + k * lda:][:M] for k in range(K)])   # [K][M]
            B = torch.stack([b[1 + b0 * sb[0] + b1 * sb[1] + k * ldb:][:N] for k in range(K)])
            _close(got[b0, b1], 0.5 * A.t() @ B)
    sa_neg = (120, -10)   # negative inner stride (the dY shifts of the exact-fp32 backward-weights GEMMs)
    got = ref64.gemm_nt(a, b, M=M, N=N, K=K, lda=lda, ldb=ldb, alpha=2.0, nb0=nb0, nb1=nb1, sa=sa_neg, sb=sb, a_off=40, b_off=0)
    for b0 in range(nb0):
        for b1 in range(nb1):
            A = torch.stack([a[40 + b0 * sa_neg[0] + b1 * sa_neg[1] + m * lda:][:K] for m in range(M)])   # [M][K]
            B = torch.stack([b[b0 * sb[0] + b1 * sb[1] + n * ldb:][:K] for n in range(N)])
            _close(got[b0, b1], 2.0 * A @ B.t())


def test_mse_loss_matches_autograd():
    p = _randn((5, 7), 21).requires_grad_(True)
    t = _randn((5, 7), 22)
    loss = torch.nn.MSELoss()(p, t)
    loss.backward()
    l64, d64 = ref64.mse_loss(p.detach(), t)
    _close(l64, loss.detach())
    _close(d64, p.grad)


# ================================================================================================ the conv entry point's references
def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _conv_case(seed, N, H, W, C0, C1, Cout, ksize):
    x = _randn((N, H, W, C0), seed)
    x2 = _randn((N, H, W, C1), seed + 1) if C1 else None
    w = _randn((Cout, C0 + C1, ksize, ksize), seed + 2, 0.3)
    return x, x2, w


def _torch_conv(a_nhwc, w, stride, pad):
    return _nhwc(F.conv2d(_nchw(a_nhwc), w, stride=stride, padding=pad))


@pytest.mark.parametrize("N,H,W,C0,C1,Cout,ksize,stride,pad", [
    (2, 5, 7, 3, 0, 4, 3, 1, 1), (1, 6, 4, 2, 3, 5, 3, 1, 1), (2, 5, 7, 3, 0, 4, 3, 2, 1), (1, 7, 5, 2, 2, 3, 3, 2, 1), (2, 4, 6, 3, 2, 4, 1, 1, 0),
    (1, 5, 5, 4, 0, 2, 1, 2, 0), (1, 4, 4, 2, 0, 3, 3, 1, 0), (3, 1, 1, 2, 0, 2, 3, 1, 1)])
def test_conv_forward_matches_conv2d(N, H, W, C0, C1, Cout, ksize, stride, pad):
    x, x2, w = _conv_case(20, N, H, W, C0, C1, Cout, ksize)
    a = x if x2 is None else torch.cat([x, x2], -1)
    ref = _torch_conv(a, w, stride, pad)
    _close(ref64.conv_forward(x, x2, w, ksize=ksize, stride=stride, pad=pad), ref)
    _close(ref64.conv_abs_bound(x, x2, w, ksize=ksize, stride=stride, pad=pad), _torch_conv(a.abs(), w.abs(), stride, pad))


@pytest.mark.parametrize("ups", [1, 3])
@pytest.mark.parametrize("H,W,pad_tl", [(3, 3, 1), (4, 5, 0), (3, 3, 0), (1, 2, 1)])
def test_conv_forward_nearest_upsampling_and_pad_tl(ups, H, W, pad_tl):
    x, x2, w = _conv_case(30, 2, H, W, 3, 2, 4, 3)
    a = F.interpolate(_nchw(torch.cat([x, x2], -1)), scale_factor=2, mode="nearest")
    if pad_tl:
        a = F.pad(a, (1, 0, 1, 0))
    ref = _nhwc(F.conv2d(a, w, padding=1))
    got = ref64.conv_forward(x, x2, w, ksize=3, pad=1, upsample=ups, pad_tl=pad_tl)
    assert got.shape[1:3] == (2 * H + pad_tl, 2 * W + pad_tl)  # (3 x 3 -> 7 x 7)
    _close(got, ref)


@pytest.mark.parametrize("H,W", [(3, 4), (5, 5), (8, 6), (7, 9)])
def test_conv_forward_zero_insertion_is_the_stride2_backward_data(H, W):
    """upsample = 2 with the flipped, transposed weight = the float64 autograd gradient of the stride-2 conv (even and odd maps: the
    gradient of an odd map's last row / column lies beyond the zero-inserted grid, so the comparison crops to it)"""
    Cin, Cout, N = 3, 4, 2
    xin = _randn((N, Cin, H, W), 40).requires_grad_(True)
    w = _randn((Cout, Cin, 3, 3), 41, 0.3)
    y = F.conv2d(xin, w, stride=2, padding=1)
    dy = _randn(tuple(y.shape), 42)
    (dx,) = torch.autograd.grad(y, xin, dy)
    got = ref64.conv_forward(_nhwc(dy), None, w.flip(2, 3).transpose(0, 1), ksize=3, pad=1, upsample=2)
    Ho, Wo = y.shape[2:]
    assert got.shape[1:3] == (2 * Ho, 2 * Wo)
    _close(got[:, :H, :W], _nhwc(dx)[:, :min(H, 2 * Ho), :min(W, 2 * Wo)])
    z = ref64.zero_insert2x(_nhwc(dy))
    assert float(z[:, 1::2].abs().max()) == 0 and float(z[:, :, 1::2].abs().max()) == 0 and torch.equal(z[:, ::2, ::2], _nhwc(dy))


@pytest.mark.parametrize("H,W", [(2, 3), (4, 4), (1, 1)])
def test_conv_forward_upsample4_is_the_backward_data_of_the_nearest2x_conv(H, W):
    Cin, Cout, N = 3, 5, 2
    xin = _randn((N, Cin, H, W), 50).requires_grad_(True)
    w = _randn((Cout, Cin, 3, 3), 51, 0.3)
    y = F.conv2d(F.interpolate(xin, scale_factor=2, mode="nearest"), w, padding=1)
    dy = _randn(tuple(y.shape), 52)
    (dx,) = torch.autograd.grad(y, xin, dy)
    got = ref64.conv_forward(_nhwc(dy), None, w, ksize=3, pad=1, upsample=4)
    assert got.shape == (N, H, W, Cin)
    _close(got, _nhwc(dx))
    bound = ref64.conv_abs_bound(_nhwc(dy), None, w, ksize=3, pad=1, upsample=4)
    assert bool((bound >= got.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("cbias_stride", [0, 9])
def test_conv_forward_epilogue_groupnorm_and_fused_skip(silu, cbias_stride):
    N, H, W, C0, C1, Cout = 3, 4, 5, 3, 2, 4
    x, x2, w = _conv_case(60, N, H, W, C0, C1, Cout, 3)
    ss = torch.stack([_randn((N, C0 + C1), 63, 1.3), _randn((N, C0 + C1), 64, 0.5)], -1)  # scales of both signs
    bias, cbias, res = _randn((Cout,), 65), _randn((N * 9 + Cout,), 66), _randn((N, H, W, Cout), 67)
    sx, sx2, sw = _randn((N, H, W, 4), 68), _randn((N, H, W, 2), 69), _randn((Cout, 6, 1, 1), 70, 2.0)
    alpha = -0.75
    a = torch.cat([x, x2], -1) * ss[:, None, None, :, 0] + ss[:, None, None, :, 1]
    if silu:
        a = F.silu(a)
    cb = torch.stack([cbias[n * cbias_stride:n * cbias_stride + Cout] for n in range(N)])
    ref = alpha * (_torch_conv(a, w, 1, 1) + _torch_conv(torch.cat([sx, sx2], -1), sw, 1, 0)) + bias + cb[:, None, None, :] + res
    kw = dict(ksize=3, pad=1, gn_scale_shift=ss, gn_silu=silu, alpha=alpha, bias=bias, cbias=cbias, cbias_stride=cbias_stride, res=res,
              skip_x=sx, skip_x2=sx2, skip_w=sw)
    _close(ref64.conv_forward(x, x2, w, **kw), ref)
    refb = 0.75 * (_torch_conv(a.abs(), w.abs(), 1, 1) + _torch_conv(torch.cat([sx, sx2], -1).abs(), sw.abs(), 1, 0)) + bias.abs() \
        + cb.abs()[:, None, None, :] + res.abs()
    _close(ref64.conv_abs_bound(x, x2, w, **kw), refb)
    _close(ref64.conv_forward(x, None, w[:, :C0], ksize=3, pad=1, skip_x=sx, skip_w=sw[:, :4]),
           _torch_conv(x, w[:, :C0], 1, 1) + _torch_conv(sx, sw[:, :4], 1, 0))


def test_stats_of():
    y = _randn((3, 4, 5, 6), 80)
    s = ref64.stats_of(y)
    _close(s[..., 0], y.sum((1, 2)))
    _close(s[..., 1], (y * y).sum((1, 2)))


def test_presplit_scale_follows_the_bound_table():
    tab = torch.zeros((6, 32))
    tab[0, 3], tab[1, 31], tab[2, 0], tab[3, 5], tab[4, 7] = 1.0, 3.999, 2.0 ** 14, 1e-30, float("nan")
    tab[0, 9] = 0.25  # a smaller entry elsewhere does not matter
    s = ref64.presplit_scale(tab)
    assert s.tolist() == [2.0 ** 14, 2.0 ** 13, 1.0, 2.0 ** 60, 2.0 ** -113, 2.0 ** 60]
    assert ref64.presplit_scale(tab, kmin=ref64.AB_KMIN_ATTN)[4] == 2.0 ** -48
    for b in (0.7, 1.0, 1.9, 123.4, 5e-7, 3e12):
        sb = float(ref64.presplit_scale(torch.full((1, 32), b))[0]) * b
        assert 2 ** 14 <= sb < 2 ** 15 * (1 + 1e-7), (b, sb)


def test_presplit_layout_roundtrip():
    """encode -> decode to 2^-21 relative of the image maximum's scale for every element, 2^-21 relative for elements within 2^10 of it;
    the layout is [8 x fp16 hi | 8 x fp16 lo] per 8 channels"""
    N, C = 3, 24
    x = (_randn((N, 5, 4, C), 90) * torch.tensor([1.0, 2.0 ** 10, 2.0 ** -10], dtype=D).reshape(3, 1, 1, 1)).float()
    tab = torch.zeros((N, 32))
    tab[:, 4] = 1.5 * x.abs().amax((1, 2, 3))
    s = ref64.presplit_scale(tab)
    p = ref64.presplit_encode(x, s)
    assert p.dtype == torch.float32 and p.shape == x.shape
    h = p.view(torch.float16).reshape(N, 5, 4, C // 8, 16)
    v = (x.double() * s.reshape(3, 1, 1, 1)).reshape(N, 5, 4, C // 8, 8)
    assert torch.equal(h[..., :8], v.to(torch.float16))
    assert float(h.abs().max()) < 2 ** 15
    back = ref64.presplit_decode(p, s)
    big = x.abs() > x.abs().amax((1, 2, 3), keepdim=True) * 2.0 ** -10
    assert float(((back - x.double()).abs() / x.double().abs())[big].max()) < 2.0 ** -21
    assert float(((back - x.double()).abs() / x.abs().amax((1, 2, 3), keepdim=True).double()).max()) < 2.0 ** -21


@pytest.mark.parametrize("H,W", [(2, 3), (4, 4), (1, 1)])
def test_conv_forward_from_class_kernels_is_the_same_function(H, W):
    """upsample 3 and 4 computed class by class from up4_class_kernels(w) = the nine-tap forms from w itself"""
    x, _, w = _conv_case(100, 2, H, W, 3, 0, 5, 3)
    wc = ref64.up4_class_kernels(w)
    assert wc.shape == (20, 3, 3, 3) and float(wc[:5, :, 2].abs().max()) == 0 and float(wc[15:, :, :, 0].abs().max()) == 0
    _close(wc[:5, :, 1, 1], w[:, :, 1:, 1:].sum((2, 3)))
    _close(ref64.conv_forward(x, None, None, ksize=3, pad=1, upsample=3, class_w=wc), ref64.conv_forward(x, None, w, ksize=3, pad=1, upsample=3))
    dy = _randn((2, 2 * H, 2 * W, 5), 103)
    _close(ref64.conv_forward(dy, None, None, ksize=3, pad=1, upsample=4, class_w=wc), ref64.conv_forward(dy, None, w, ksize=3, pad=1, upsample=4))
    s2d = ref64.space_to_depth2(dy)
    assert torch.equal(s2d[:, :, :, 5:10], dy[:, 0::2, 1::2])


# ================================================================================================ glue ops of the inference forward
@pytest.mark.parametrize("N,C,H,W", [(1, 3, 2, 2), (2, 5, 5, 7), (3, 4, 6, 4), (1, 2, 7, 6)])
def test_resample2x_pool_and_nearest_match_torch(N, C, H, W):
    x = _randn((N, C, H, W), 60)
    _close(ref64.resample2x(_nhwc(x), 0), _nhwc(F.avg_pool2d(x, 2)))
    up = F.interpolate(x, scale_factor=2, mode="nearest")
    _close(ref64.resample2x(_nhwc(x), 1), _nhwc(up))
    _close(ref64.resample2x(_nhwc(x), 1, 1), _nhwc(F.pad(up, (1, 0, 1, 0))))
    for pad in (0, 1, 2, 3):
        _close(ref64.resample2x(_nhwc(x), 4, pad), _nhwc(x[:, :, :H - (pad & 1), :W - (pad >> 1)]))


@pytest.mark.parametrize("N,C,H,W", [(1, 3, 1, 1), (2, 5, 3, 3), (3, 4, 6, 4)])
@pytest.mark.parametrize("pad", [0, 1])
def test_resample2x_mode2_is_the_autograd_adjoint_of_mode1(N, C, H, W, pad):
    x = _randn((N, C, H, W), 61).requires_grad_(True)
    y = F.pad(F.interpolate(x, scale_factor=2, mode="nearest"), (pad, 0, pad, 0))
    g = _randn(tuple(y.shape), 62)
    y.backward(g)
    got = ref64.resample2x(_nhwc(g), 2, pad)
    _close(got, _nhwc(x.grad))
    assert got.shape[1:3] == (H, W)


@pytest.mark.parametrize("N,C,H,W", [(1, 3, 2, 2), (2, 5, 5, 7), (3, 4, 6, 4), (2, 2, 3, 3)])
def test_resample2x_mode3_is_the_autograd_adjoint_of_mode0(N, C, H, W):
    x = _randn((N, C, H, W), 63).requires_grad_(True)
    y = F.avg_pool2d(x, 2)
    g = _randn(tuple(y.shape), 64)
    y.backward(g)
    _close(ref64.resample2x(_nhwc(g), 3, H % 2), _nhwc(x.grad))   # (H and W are both odd or both even here)


@pytest.mark.parametrize("N,Dm,E,J,labels,t_float", [(3, 32, 16, 24, False, False), (5, 33, 8, 0, True, True), (2, 6, 4, 7, True, False)])
def test_time_embed_matches_plain_torch_linears(N, Dm, E, J, labels, t_float):
    half = Dm // 2
    freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half)
    t = torch.tensor([0.0, 999.0, 12.5, 3.25, 500.0][:N]) if t_float else torch.tensor([0, 999, 17, 4, 250][:N])
    w1, b1, w2, b2 = _randn((E, Dm), 65, 0.3), _randn((E,), 66), _randn((E, E), 67, 0.3), _randn((E,), 68)
    wcat, bcat = (_randn((J, E), 69, 0.3), _randn((J,), 70)) if J else (None, None)
    lab = _randn((4, E), 71) if labels else None
    y = torch.tensor([3, 0, 3, 1, 2][:N]) if labels else None
    h1, emb, out = ref64.time_embed(t, freqs, w1, b1, w2, b2, wcat, bcat, label_emb=lab, y=y)
    arg = (t.float()[:, None] * freqs[None]).double()
    e = torch.cat([arg.cos(), arg.sin()] + ([torch.zeros(N, 1, dtype=D)] if Dm % 2 else []), 1)
    rh = F.silu(F.linear(e, w1, b1))
    re = F.linear(rh, w2, b2) + (F.embedding(y, lab) if labels else 0.0)
    _close(h1, rh)
    _close(emb, re)
    if J:
        _close(out, F.linear(F.silu(re), wcat, bcat))
        _, emb3, out3 = ref64.time_embed(None, None, None, None, None, None, wcat, bcat, emb=re)   # stage 3 alone
        assert torch.equal(emb3, re)
        _close(out3, out)
    else:
        assert out is None


@pytest.mark.parametrize("per,epc", [(4, 4), (8, 8), (31 * 4, 4), (40 * 8, 8), ((32 * 7 + 5) * 4, 4)])
def test_act_bound_direct_is_the_brute_force_maximum(per, epc):
    x = _randn((3, per), 72)
    x[2, -1] = 50.0
    got = ref64.act_bound_direct(x, epc)
    chunks = per // epc
    covered = 0
    for n in range(3):
        for j in range(32):
            idx = [i for i in range(chunks) if chunks * j // 32 <= i < chunks * (j + 1) // 32]
            covered += len(idx)
            want = max((abs(float(x[n, i * epc + e])) for i in idx for e in range(epc)), default=0.0)
            assert float(got[n, j]) == want, (n, j)
    assert covered == 3 * chunks            # the ranges partition the chunks
    assert float(got[2, 31]) == 50.0 and float(got.max(1).values[0]) == float(x[0].abs().max())
    x[1, per // 2] = float("nan")
    x[0, 0] = float("-inf")
    got = ref64.act_bound_direct(x, epc)
    assert int(torch.isinf(got[1]).sum()) == 1 and int(torch.isinf(got[0]).sum()) == 1 and float(got[0, 0] if chunks >= 32 else got[0].max()) == math.inf


def test_act_bound_parts_is_the_brute_force_maximum():
    p0, p1 = _randn((2, 3, 5, 2), 73).abs(), _randn((2, 1, 7, 2), 74).abs()   # P*C = 15 and 7 pairs: no multiple of 32
    got = ref64.act_bound_parts([p0, p1])
    for n in range(2):
        for j in range(32):
            vals = [float(p.reshape(2, -1, 2)[n, i, 1]) for p in (p0, p1) for i in range(p.shape[1] * p.shape[2])
                    if p.shape[1] * p.shape[2] * j // 32 <= i < p.shape[1] * p.shape[2] * (j + 1) // 32]
            assert float(got[n, j]) == math.sqrt(max(vals, default=0.0))
    assert float(got.max(1).values[0]) == math.sqrt(max(float(p0[0, :, :, 1].max()), float(p1[0, :, :, 1].max())))
    p0[1, 2, 4, 1] = float("nan")
    got = ref64.act_bound_parts([p0])
    assert float(got[1, 31]) == math.inf and bool(torch.isfinite(got[0]).all())


def test_linear_bound_bounds_a_linear_layer():
    w, b = _randn((6, 9), 75), _randn((6,), 76)
    c0, c1 = ref64.linear_bound(w, b)
    assert c0 == pytest.approx(max(math.fsum(abs(float(v)) for v in row) for row in w), rel=1e-14) and c1 == max(abs(float(v)) for v in b)
    assert ref64.linear_bound(w) == (c0, 0.0)
    x = _randn((50, 9), 77)
    y = F.linear(x, w, b)
    assert bool((y.abs().amax(1) <= c0 * x.abs().amax(1) + c1).all())
    xs = torch.sign(w[int(w.abs().sum(1).argmax())])[None]   # the bound is attained
    assert float(F.linear(xs, w).abs().max()) == pytest.approx(c0, rel=1e-14)


# ================================================================================================ attention, softmax rows
def _orders(heads, d):
    C = heads * d
    return {"legacy": (0, d, 2 * d, 3 * d), "new": (0, C, 2 * C, d)}


def _torch_attention(qkv, heads, d, order):
    """QKVAttentionLegacy / QKVAttention of the modelled UNet, written on [N][3C][T] as there (scale d^-1/4 on q and on k)"""
    N, T, W = qkv.shape
    x = qkv.permute(0, 2, 1)
    if order == "legacy":
        q, k, v = x.reshape(N * heads, 3 * d, T).split(d, dim=1)
    else:
        q, k, v = (t.reshape(N * heads, d, T) for t in x.chunk(3, dim=1))
    s = 1.0 / math.sqrt(math.sqrt(d))
    w = torch.einsum("bct,bcs->bts", q * s, k * s)
    P = torch.softmax(w, -1)
    a = torch.einsum("bts,bcs->bct", P, v).reshape(N, heads * d, T).permute(0, 2, 1)
    return a, torch.logsumexp(w, -1).reshape(N, heads, T), P.reshape(N, heads, T, T)


@pytest.mark.parametrize("order", ["legacy", "new"])
@pytest.mark.parametrize("N,T,heads,d", [(1, 1, 1, 8), (2, 7, 3, 4), (3, 33, 2, 12), (1, 65, 1, 24)])
def test_attention_forward_and_backward_match_autograd(order, N, T, heads, d):
    qo, ko, vo, hs = _orders(heads, d)[order]
    qkv = _randn((N, T, 3 * heads * d), 40, 0.9).requires_grad_(True)
    dO = _randn((N, T, heads * d), 41)
    a, lse, P = _torch_attention(qkv, heads, d, order)
    a.backward(dO)
    out, lse64, P64 = ref64.attention_forward(qkv.detach(), heads, d, qo, ko, vo, hs)
    _close(out, a.detach())
    _close(lse64, lse.detach())
    _close(P64, P.detach())
    assert float((P64.sum(-1) - 1).abs().max()) < 1e-14
    dqkv, Dr = ref64.attention_backward(qkv.detach(), dO, heads, d, qo, ko, vo, hs)
    _close(dqkv, qkv.grad, 1e-11)
    _close(Dr, ref64.head_slices(dO * a.detach(), heads, d, 0, d).sum(-1), 1e-11)   # D = rowsum(dP * P) = sum_j dO * out


def test_attention_forward_of_one_key_returns_v():
    heads, d = 3, 8
    for order, (qo, ko, vo, hs) in _orders(heads, d).items():
        qkv = _randn((2, 1, 3 * heads * d), 42)
        out, lse, P = ref64.attention_forward(qkv, heads, d, qo, ko, vo, hs)
        assert torch.equal(out, ref64.head_slices(qkv, heads, d, vo, hs).permute(0, 2, 1, 3).reshape(2, 1, heads * d)), order
        assert torch.equal(P, torch.ones_like(P))


def test_softmax_rows_and_backward_match_autograd():
    for rows, n, lds in ((5, 1, 4), (3, 65, 72), (2, 1030, 1036)):
        s = _randn((rows, lds), 43, 4.0)
        s[0, :n] += 50.0 * (torch.arange(n) % 7 == 0)   # a peaked row
        sn = s.clone()
        sn[:, n:] = float("nan")                        # columns behind n are never read
        z = s[:, :n].clone().requires_grad_(True)
        P = torch.softmax(z, -1)
        g = _randn((rows, lds), 44)
        P.backward(g[:, :n])
        got = ref64.softmax_rows(sn, n)
        _close(got, P.detach())
        Pp = torch.nn.functional.pad(P.detach(), (0, lds - n), value=float("nan"))
        _close(ref64.softmax_backward_rows(Pp, g, n), z.grad, 1e-11)


def test_rowdot_matches_einsum_in_both_channel_orders():
    N, T, heads, d = 2, 5, 3, 8
    C = heads * d
    a, b = _randn((N, T, C), 45), _randn((N, T, C), 46)
    ref = torch.einsum("nthj,nthj->nht", a.reshape(N, T, heads, d), b.reshape(N, T, heads, d))
    _close(ref64.rowdot(a, b, N, heads, T, T * C, d, C, d), ref)
    # a strided operand: the q slices of a legacy-order qkv tensor against themselves
    qkv = _randn((N, T, 3 * C), 47)
    q = ref64.head_slices(qkv, heads, d, 0, 3 * d)
    _close(ref64.rowdot(qkv, qkv, N, heads, T, T * 3 * C, 3 * d, 3 * C, d), (q * q).sum(-1))


@pytest.mark.parametrize("new_order", [False, True])
@pytest.mark.parametrize("T,heads,d,epc", [(7, 2, 12, 8), (5, 3, 4, 8), (9, 1, 20, 4), (8, 2, 8, 8)])
def test_attention_pack_matches_the_row_maps_of_the_attention_block(new_order, T, heads, d, epc):
    """the packed operands against the row maps written out as AttentionBlock._row_maps writes them (an index list with -1 = zero row),
    and the packed attention against the natural-layout one"""
    N, C = 2, heads * d
    dpad, ldt = -(-d // epc) * epc, -(-T // epc) * epc
    base = (lambda which, h: which * C + h * d) if new_order else (lambda which, h: h * 3 * d + which * d)
    qk_rows = [r for which in (0, 1) for h in range(heads) for r in [base(which, h) + j for j in range(d)] + [-1] * (dpad - d)]
    v_rows = [base(2, h) + j for h in range(heads) for j in range(d)]
    qkv = _randn((N, T, 3 * C), 48)
    qk, vT = ref64.attention_pack(qkv, heads, d, dpad, ldt, new_order)
    ext = torch.cat([qkv, torch.zeros((N, T, 1), dtype=D)], -1)
    assert torch.equal(qk, ext[..., qk_rows].reshape(N * T, 2 * heads * dpad))
    assert torch.equal(vT[..., :T], qkv[..., v_rows].transpose(1, 2)) and not bool(vT[..., T:].any())
    # attention on the packed operands == attention on the natural layout
    Cq = heads * dpad
    q = qk[:, :Cq].reshape(N, T, heads, dpad).permute(0, 2, 1, 3)
    k = qk[:, Cq:].reshape(N, T, heads, dpad).permute(0, 2, 1, 3)
    P = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(d), -1)
    a = torch.einsum("nhts,nhjs->nthj", P, vT[..., :T].reshape(N, heads, d, T)).reshape(N, T, C)
    qo, ko, vo, hs = _orders(heads, d)["new" if new_order else "legacy"]
    _close(a, ref64.attention_forward(qkv, heads, d, qo, ko, vo, hs)[0])


def test_presplit_round_trip_on_attention_operands():
    """decode(encode(x)) is x to 2^-22 (two fp16 mantissas) plus half an fp16 subnormal step of the scaled value, at the scale of the attention kernels' exponent range"""
    x = _randn((3, 9, 24), 49) * torch.tensor([1e-3, 1.0, 300.0], dtype=D)[:, None, None]
    tab = torch.zeros((3, 32))
    tab[:, 5] = x.abs().amax((1, 2)).float() * 1.5
    s = ref64.presplit_scale(tab, kmin=ref64.AB_KMIN_ATTN)
    assert bool((s * x.abs().amax((1, 2)) < 2.0 ** 15).all())
    back = ref64.presplit_decode(ref64.presplit_encode(x, s), s)
    assert bool(((back - x).abs() <= 2.0 ** -22 * x.abs() + 2.0 ** -25 / s[:, None, None]).all())
