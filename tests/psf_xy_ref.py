"""CPU side of the anisotropic / shifted PSF tests (test infrastructure): tests/psf_ref.py with one tap vector per axis.

  line64, apply64, adjoint64, landweber64, cmax64 / cmax_dense, tau64   A = A1(hy, H) (x) A1(hx, W) as dense 1-D matrices built straight from the
                            orientation rule (row i of B0 holds h[t] at column i - r + t), the exact adjoint, the Landweber step and
                            tau = f^2 / (cmax(hy, H) cmax(hx, W)), in float64;
  norm, blur, apply, residual, update, project     eod_psf_apply_xy / eod_psf_residual_xy / eod_psf_update_xy and BoundPsf.project in torch
                            fp32, one separately rounded operation per line, in the order include/eodiff.h states: zero-padded tensors,
                            taps in ascending order, sequential adds, horizontal first; the update blurs with the REVERSED taps and
                            divides by the n of the FORWARD ones; with `response` the band mix of section 9.10 in its order;
  step32                    the fp32 step = fp32(tau / f^2) the product hands to eod_psf_update_xy;
  psf_link                  a link of a chain as a function prediction -> prediction;
  gaussian                  Gaussian taps centred at `shift`, by the formula of the issue, computed here;
  one_sided                 the family [0, ..., 0, .6, .4]: everything the sample sees lies at and right of / below its centre.
"""
import math

import numpy as np
import torch

from tests import consistency_ref as CR
from tests import psf_ref as PR

_f = lambda v: float(np.float32(v))


def gaussian(f, mtf=0.3, radius=None, shift=0.0):
    if shift == 0.0:
        return PR.gaussian(f, mtf, radius)
    sigma = f * math.sqrt(-2.0 * math.log(mtf)) / math.pi
    r = min(int(math.ceil(3.0 * sigma + abs(shift))), 12) if radius is None else radius
    k = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-((k - shift) ** 2) / (2.0 * sigma * sigma))
    return (g / g.sum()).astype(np.float32)


def one_sided(r):
    h = np.zeros(2 * r + 1, np.float32)
    if r == 0:
        h[0] = 1.0
    else:
        h[r], h[r + 1] = 0.6, 0.4
    return h


def _channels(channels, C):
    return list(range(C)) if channels is None else list(channels)


# ------------------------------------------------------------------------------------------------ float64
def line64(h, L, f=1):
    """(A1 [L / f, L], n [L]): D_f N^-1 B0 on a line of length L, B0[i][i - r + t] = h[t]"""
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


def _mixed64(x, channels, response):
    x = np.asarray(x, np.float64)
    if response is not None:
        return np.einsum("kc,bchw->bkhw", np.asarray(response, np.float32).astype(np.float64), x)
    return x[:, _channels(channels, x.shape[1])]


def apply64(x, hy, hx, f, channels=None, response=None):
    u = _mixed64(x, channels, response)
    Ay, Ax = line64(hy, u.shape[2], f)[0], line64(hx, u.shape[3], f)[0]
    return np.einsum("yh,bkhw,xw->bkyx", Ay, u, Ax)


def adjoint64(q, hy, hx, f, H, W):
    """A_s^T q per coarse plane: [B, K, H, W]"""
    Ay, Ax = line64(hy, H, f)[0], line64(hx, W, f)[0]
    return np.einsum("yh,bkyx,xw->bkhw", Ay, np.asarray(q, np.float64), Ax)


def cmax_dense(h, L):
    """the largest column sum of N^-1 B0, from the dense matrix"""
    return float(line64(h, L, 1)[0].sum(axis=0).max())


def cmax64(h, L):
    """the same by two full convolutions (no dense matrix: L may be a scene's width): n[y] = sum_t h[t] [0 <= y - r + t < L] is the
    convolution of ones with the REVERSED taps, column j of N^-1 B0 sums h[t] / n[j + r - t], a convolution of 1 / n with the taps"""
    h = np.asarray(h, np.float32).astype(np.float64)
    r = h.size // 2
    n = np.convolve(np.ones(L), h[::-1])[r:r + L]
    return float(np.convolve(1.0 / n, h)[r:r + L].max())


def tau64(hy, hx, f, H, W):
    return float(f * f) / (cmax64(hy, H) * cmax64(hx, W))


def landweber64(p, values, hy, hx, f, channels=None, mask=None, lam=1.0, iters=1, tau=None):
    p = np.array(p, np.float64)
    cs = _channels(channels, p.shape[1])
    H, W = p.shape[2:]
    tau = tau64(hy, hx, f, H, W) if tau is None else tau
    m = 1.0 if mask is None else np.asarray(mask, np.float64)
    for _ in range(iters):
        res = m * (apply64(p, hy, hx, f, cs) - np.asarray(values, np.float64))
        p[:, cs] = p[:, cs] - lam * tau * adjoint64(res, hy, hx, f, H, W)
    return p


# ------------------------------------------------------------------------------------------------ the kernels, in torch fp32
_conv = PR._conv            # taps in ascending order over the zero-padded line: already free of any symmetry


def blur(u, hy, hx):
    """conv_y(conv_x(u; hx); hy) of [..., H, W]"""
    hz = _conv(u, hx, u.dim() - 1)
    return _conv(hz, hy, u.dim() - 2)


def norm(hy, hx, H, W):
    """n [H, W] = nv[y] * nh[x], FORWARD taps"""
    nh = _conv(torch.ones(W), hx, 0)
    nv = _conv(torch.ones(H), hy, 0)
    return nv[:, None] * nh[None, :]


def _mix(planes, M):
    """sum_j M[i][j] * planes[:, j], products and adds in index order: [B, rows, ...]"""
    out = []
    for row in np.asarray(M, np.float32):
        acc = planes[:, 0] * _f(row[0])
        for j in range(1, len(row)):
            pr = planes[:, j] * _f(row[j])
            acc = acc + pr
        out.append(acc)
    return torch.stack(out, 1)


def apply(p, hy, hx, f, channels=None, response=None):
    """eod_psf_apply_xy: [B, K, H / f, W / f]"""
    assert p.dtype == torch.float32 and p.dim() == 4
    u = _mix(p, response) if response is not None else p[:, _channels(channels, p.shape[1])]
    bl = blur(u, hy, hx)
    b = bl / norm(hy, hx, *p.shape[2:])
    mean = CR.block_mean(b.contiguous(), (f,) * u.shape[1])
    return mean[:, :, ::f, ::f].contiguous()


def residual(p, values, hy, hx, f, channels=None, mask=None, lam=1.0, response=None):
    """eod_psf_residual_xy: q on the coarse grid"""
    mean = apply(p, hy, hx, f, channels, response)
    lm = _f(lam) if mask is None else mask * _f(lam)
    df = mean - values
    return df * lm


def update(p, q, hy, hx, f, channels=None, step=1.0, G=None):
    """eod_psf_update_xy: n from the forward taps, the blur with the reversed ones"""
    s = _mix(q, G) if G is not None else q
    rep = s.repeat_interleave(f, 2).repeat_interleave(f, 3)
    ts = rep * _f(step)
    w = ts / norm(hy, hx, *p.shape[2:])
    bl = blur(w, np.ascontiguousarray(np.asarray(hy)[::-1]), np.ascontiguousarray(np.asarray(hx)[::-1]))
    if G is not None:
        return p - bl
    cs = _channels(channels, p.shape[1])
    out = p.clone()
    out[:, cs] = p[:, cs] - bl
    return out


def step32(hy, hx, f, H, W, response=None):
    tau = tau64(hy, hx, f, H, W)
    if response is not None:
        tau /= float(np.linalg.svd(np.asarray(response, np.float32).astype(np.float64), compute_uv=False)[0]) ** 2
    return _f(tau / (f * f))


def project(p, values, hy, hx, f, channels=None, mask=None, lam=1.0, iters=1, step=None, response=None):
    """BoundPsf.project (solver="landweber"): iters x (residual, update); with a response the adjoint mixes by R^T"""
    step = step32(hy, hx, f, *p.shape[2:], response=response) if step is None else step
    G = None if response is None else np.ascontiguousarray(np.asarray(response, np.float32).T)
    for _ in range(iters):
        p = update(p, residual(p, values, hy, hx, f, channels, mask, lam, response), hy, hx, f, channels, step, G)
    return p


def psf_link(values, hy, hx, f, channels=None, mask=None, lam=1.0, iters=1, step=None, response=None):
    return lambda p: project(p, values, hy, hx, f, channels, mask, lam, iters, step, response)


# ------------------------------------------------------------------------------------------------ the cases the tests share
# (f, ry, rx, (H, W)): the smallest shapes at which each mechanism can break
CASES = [(1, 0, 12, (6, 7)),        # lines shorter than the radius; the scalar form
         (1, 12, 0, (40, 72)),      # 2 x 3 tiles of 32, ragged in y
         (2, 3, 7, (12, 28)),
         (3, 5, 2, (48, 30)),       # tiles of 24; W / f = 10 takes the scalar coarse form
         (4, 1, 12, (32, 64)),
         (5, 7, 4, (35, 70)),       # tiles of 20
         (6, 12, 9, (24, 30)),
         (8, 12, 3, (24, 168))]
FAMILIES = ("sym", "shift", "one")


def family(name, f, ry, rx):
    """(hy, hx): two different symmetric Gaussians; Gaussians shifted by +0.37 f along y and -0.37 f along x; the one-sided taps"""
    if name == "sym":
        return gaussian(f, 0.3, radius=ry), gaussian(f, 0.5, radius=rx)
    if name == "shift":
        return gaussian(f, 0.3, radius=ry, shift=0.37 * f), gaussian(f, 0.5, radius=rx, shift=-0.37 * f)
    return one_sided(ry), one_sided(rx)
