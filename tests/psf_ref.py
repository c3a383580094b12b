"""CPU side of the PSF-aware observation tests (test infrastructure):

  line64, apply64, adjoint64, landweber64, tau64   A = D_f N^-1 B0 as dense 1-D matrices (the operator is separable), its exact adjoint, the
                            Landweber step p - lam * tau * A^T(mask * (A p - values)) and tau = f^2 / (cmax(H) cmax(W)), in float64;
  norm, blur, apply, residual, update, project     eod_psf_apply / eod_psf_residual / eod_psf_update and BoundPsf.project in torch fp32, one
                            separately rounded operation per line, in the order include/eodiff.h states: zero-padded tensors, taps in
                            ascending order, sequential adds, horizontal first; the block mean is tests/consistency_ref.py block_mean's;
  step32                    the fp32 step = fp32(tau / f^2) the product hands to eod_psf_update;
  psf_link                  a link of a chain as a function prediction -> prediction, for spectral_ref.ddim_step / dpm_step /
                            ddim_sampled / dpm_sampled;
  gaussian                  Gaussian taps by the formula of the issue, computed here (not the product's gaussian_psf).
"""
import math

import numpy as np
import torch

from tests import consistency_ref as CR

_f = lambda v: float(np.float32(v))


def gaussian(f, mtf=0.3, radius=None):
    sigma = f * math.sqrt(-2.0 * math.log(mtf)) / math.pi
    r = min(int(math.ceil(3.0 * sigma)), 12) if radius is None else radius
    k = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-(k * k) / (2.0 * sigma * sigma))
    h = (g / g.sum()).astype(np.float32)
    h[r + 1:] = h[:r][::-1]
    return h


def _channels(channels, C):
    return list(range(C)) if channels is None else list(channels)


# ------------------------------------------------------------------------------------------------ float64
def line64(h, L, f=1):
    """(A1 [L / f, L], n [L]): the 1-D operator D_f N^-1 B0 on a line of length L as a dense matrix; A = A1(H) (x) A1(W)"""
    h = np.asarray(h, np.float32).astype(np.float64)
    r = h.size // 2
    B0 = np.zeros((L, L))
    for i in range(L):
        for t in range(h.size):
            j = i - r + t
            if 0 <= j < L:
                B0[i, j] = h[t]
    n = B0.sum(axis=1)
    D = np.kron(np.eye(L // f), np.full((1, f), 1.0 / f))
    return D @ (B0 / n[:, None]), n


def apply64(x, h, f, channels=None):
    x = np.asarray(x, np.float64)
    cs = _channels(channels, x.shape[1])
    Ay, Ax = line64(h, x.shape[2], f)[0], line64(h, x.shape[3], f)[0]
    return np.einsum("yh,bkhw,xw->bkyx", Ay, x[:, cs], Ax)


def adjoint64(q, h, f, H, W):
    """A^T q per observed channel: [B, K, H, W]"""
    Ay, Ax = line64(h, H, f)[0], line64(h, W, f)[0]
    return np.einsum("yh,bkyx,xw->bkhw", Ay, np.asarray(q, np.float64), Ax)


def cmax64(h, L):
    """the largest column sum of N^-1 B0 on a line of length L, by two full convolutions (no dense matrix: L may be a scene's width)"""
    h = np.asarray(h, np.float32).astype(np.float64)
    r = h.size // 2
    n = np.convolve(np.ones(L), h)[r:r + L]
    return float(np.convolve(1.0 / n, h)[r:r + L].max())


def tau64(h, f, H, W):
    return float(f * f) / (cmax64(h, H) * cmax64(h, W))


def landweber64(p, values, h, f, channels=None, mask=None, lam=1.0, iters=1, tau=None):
    p = np.array(p, np.float64)
    cs = _channels(channels, p.shape[1])
    H, W = p.shape[2:]
    tau = tau64(h, f, H, W) if tau is None else tau
    m = 1.0 if mask is None else np.asarray(mask, np.float64)
    for _ in range(iters):
        res = m * (apply64(p, h, f, cs) - np.asarray(values, np.float64))
        p[:, cs] = p[:, cs] - lam * tau * adjoint64(res, h, f, H, W)
    return p


# ------------------------------------------------------------------------------------------------ the kernels, in torch fp32
def _conv(u, h, dim):
    r, L = len(h) // 2, u.shape[dim]
    shape = list(u.shape)
    shape[dim] = r
    z = torch.zeros(shape, dtype=torch.float32)
    pad = torch.cat([z, u, z], dim)
    acc = pad.narrow(dim, 0, L) * _f(h[0])
    for i in range(1, 2 * r + 1):
        pr = pad.narrow(dim, i, L) * _f(h[i])
        acc = acc + pr
    return acc


def blur(u, h):
    """conv_v(conv_h(u)) of [..., H, W]"""
    hz = _conv(u, h, u.dim() - 1)
    return _conv(hz, h, u.dim() - 2)


def norm(h, H, W):
    """n [H, W] = nv[y] * nh[x]"""
    nh = _conv(torch.ones(W), h, 0)
    nv = _conv(torch.ones(H), h, 0)
    return nv[:, None] * nh[None, :]


def apply(p, h, f, channels=None):
    """eod_psf_apply: [B, K, H / f, W / f]"""
    assert p.dtype == torch.float32 and p.dim() == 4
    cs = _channels(channels, p.shape[1])
    bl = blur(p[:, cs], h)
    b = bl / norm(h, *p.shape[2:])
    mean = CR.block_mean(b.contiguous(), (f,) * len(cs))
    return mean[:, :, ::f, ::f].contiguous()


def residual(p, values, h, f, channels=None, mask=None, lam=1.0):
    """eod_psf_residual: q on the coarse grid"""
    mean = apply(p, h, f, channels)
    lm = _f(lam) if mask is None else mask * _f(lam)
    df = mean - values
    return df * lm


def update(p, q, h, f, channels=None, step=1.0):
    """eod_psf_update"""
    cs = _channels(channels, p.shape[1])
    rep = q.repeat_interleave(f, 2).repeat_interleave(f, 3)
    ts = rep * _f(step)
    w = ts / norm(h, *p.shape[2:])
    bl = blur(w, h)
    out = p.clone()
    out[:, cs] = p[:, cs] - bl
    return out


def step32(h, f, H, W):
    return _f(tau64(h, f, H, W) / (f * f))


def project(p, values, h, f, channels=None, mask=None, lam=1.0, iters=1, step=None):
    """BoundPsf.project: iters x (residual, update)"""
    step = step32(h, f, *p.shape[2:]) if step is None else step
    for _ in range(iters):
        p = update(p, residual(p, values, h, f, channels, mask, lam), h, f, channels, step)
    return p


def psf_link(values, h, f, channels=None, mask=None, lam=1.0, iters=1, step=None):
    return lambda p: project(p, values, h, f, channels, mask, lam, iters, step)


def psf_link64(values, h, f, channels=None, mask=None, lam=1.0, iters=1):
    return lambda p: landweber64(p, values, h, f, channels, mask, lam, iters)
