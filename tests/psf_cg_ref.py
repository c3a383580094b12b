"""CPU side of the exact PSF data-consistency tests (test infrastructure):

  gram64, bands_of          the 1-D Gram matrix G_L = A1 A1^T of psf_ref.line64's A1 as a dense float64 matrix, and its band [L / f, 2b + 1];
  dense_of                  a band table (fp32 or float64) back as a dense float64 matrix;
  cg64                      conjugate gradients for (M G M + mu I) z = c per plane in float64, G = Gy (x) Gx dense, with the guard of the issue;
  dense64                   the same system by np.linalg.lstsq on kron(Gy, Gx) restricted by the mask (small planes);
  gram32                    eod_psf_gram in torch fp32, one separately rounded operation per line, in the order include/eodiff.h states;
  cg32                      eod_psf_cg: the whole solve in torch fp32 with float64 dots, alpha and beta rounded to fp32 once;
  project32, cg_link        BoundPsf.project with solver="cg": psf_ref.residual (weight 1) -> cg32 -> psf_ref.update (step fp32(1 / f^2)); a
                            link of a chain as a function prediction -> prediction;
  project64, cg_link64      the same in float64 with the dense operators (the toy loop).
"""
import numpy as np
import torch

from tests import psf_ref as PR

_f = lambda v: float(np.float32(v))


def half_width(r, f):
    return -((-2 * r) // f)


# ------------------------------------------------------------------------------------------------ float64
def gram64(h, L, f):
    A1 = PR.line64(h, L, f)[0]
    return A1 @ A1.T


def bands_of(G, b):
    """[n, 2b + 1] with [i][j] = G[i][i - b + j], zero outside the matrix"""
    n = G.shape[0]
    out = np.zeros((n, 2 * b + 1), G.dtype)
    for i in range(n):
        for j in range(2 * b + 1):
            col = i - b + j
            if 0 <= col < n:
                out[i, j] = G[i, col]
    return out


def dense_of(bands):
    bands = np.asarray(bands, np.float64)
    n, b = bands.shape[0], bands.shape[1] // 2
    G = np.zeros((n, n))
    for i in range(n):
        for j in range(2 * b + 1):
            col = i - b + j
            if 0 <= col < n:
                G[i, col] = bands[i, j]
    return G


def _planes(c, mask):
    c = np.asarray(c, np.float64)
    m = np.ones_like(c) if mask is None else np.broadcast_to(np.asarray(mask, np.float64), c.shape)
    return c, m


def cg64(c, Gy, Gx, mask=None, mu=0.0, iters=1):
    """z [B, K, Hc, Wc] after `iters` iterations from z = 0, every plane on its own"""
    c, m = _planes(c, mask)
    S = lambda d: m * (Gy @ (m * d) @ Gx.T) + mu * d
    dot = lambda a, b: (a * b).sum(axis=(2, 3), keepdims=True)
    z, r, d = np.zeros_like(c), c.copy(), c.copy()
    rho = dot(r, r)
    for _ in range(iters):
        q = S(d)
        sigma = dot(d, q)
        ok = np.isfinite(rho) & np.isfinite(sigma) & (rho != 0.0) & (sigma > 0.0)
        alpha = np.where(ok, rho / np.where(ok, sigma, 1.0), 0.0)
        z = z + alpha * d
        r = r - alpha * q
        rho2 = dot(r, r)
        beta = np.where(ok & np.isfinite(rho2), rho2 / np.where(ok, rho, 1.0), 0.0)
        d = r + beta * d
        rho = rho2
    return z


def dense64(c, Gy, Gx, mask=None, mu=0.0):
    """the minimum-norm solution of (M G M + mu I) z = c per plane, G = kron(Gy, Gx); z = 0 where the mask is 0"""
    c, m = _planes(c, mask)
    G = np.kron(Gy, Gx)
    z = np.zeros_like(c)
    for bi in range(c.shape[0]):
        for k in range(c.shape[1]):
            idx = np.flatnonzero(m[bi, k].ravel() != 0.0)
            if idx.size:
                mi = m[bi, k].ravel()[idx]
                S = mi[:, None] * G[np.ix_(idx, idx)] * mi[None, :] + mu * np.eye(idx.size)
                z[bi, k].reshape(-1)[idx] = np.linalg.lstsq(S, c[bi, k].ravel()[idx], rcond=None)[0]
    return z


def project64(p, values, h, f, channels=None, mask=None, lam=1.0, mu=0.0, iters=1):
    """p - lam A^T (m z), (M G M + mu I) z = m (A p - values) by `iters` float64 CG iterations"""
    p = np.array(p, np.float64)
    cs = list(range(p.shape[1])) if channels is None else list(channels)
    H, W = p.shape[2:]
    m = 1.0 if mask is None else np.asarray(mask, np.float64)
    c = m * (PR.apply64(p, h, f, cs) - np.asarray(values, np.float64))
    z = cg64(c, gram64(h, H, f), gram64(h, W, f), mask, mu, iters)
    p[:, cs] = p[:, cs] - lam * PR.adjoint64(m * z, h, f, H, W)
    return p


def cg_link64(values, h, f, channels=None, mask=None, lam=1.0, mu=0.0, iters=1):
    return lambda p: project64(p, values, h, f, channels, mask, lam, mu, iters)


# ------------------------------------------------------------------------------------------------ the kernels, in torch fp32
def _band_pass(u, g, dim):
    """(((g[., 0] * u[. - b]) + g[., 1] * u[. - b + 1]) + ...) along `dim` of [B, K, Hc, Wc]; u outside the plane is +0.0f"""
    b, L = g.shape[1] // 2, u.shape[dim]
    shape = list(u.shape)
    shape[dim] = b
    zpad = torch.zeros(shape, dtype=torch.float32)
    pad = torch.cat([zpad, u, zpad], dim)
    col = (lambda j: g[:, j]) if dim == 3 else (lambda j: g[:, j][:, None])
    acc = pad.narrow(dim, 0, L) * col(0)
    for j in range(1, 2 * b + 1):
        pr = pad.narrow(dim, j, L) * col(j)
        acc = acc + pr
    return acc


def gram32(d, gy, gx, mask=None, mu=0.0):
    """eod_psf_gram's q: d [B, K, Hc, Wc] fp32, gy [Hc, 2b + 1] / gx [Wc, 2b + 1] fp32 tensors, mask None or broadcastable, entries 0 or 1"""
    assert d.dtype == torch.float32 and gy.dtype == torch.float32 and gx.dtype == torch.float32 and d.dim() == 4
    u = d if mask is None else mask * d
    t = _band_pass(u, gx, 3)
    v = _band_pass(t, gy, 2)
    mq = v if mask is None else mask * v
    md = d * _f(mu)
    return mq + md


def _dot64(a, b):
    return (a.double() * b.double()).sum(dim=(2, 3), keepdim=True)


def cg32(c, gy, gx, mask=None, mu=0.0, lam=1.0, iters=1):
    """eod_psf_cg's q_out = lam * (m * z)"""
    z, r, d = torch.zeros_like(c), c.clone(), c.clone()
    rho = _dot64(r, r)
    one = torch.ones_like(rho)
    for _ in range(iters):
        q = gram32(d, gy, gx, mask, mu)
        sigma = _dot64(d, q)
        ok = torch.isfinite(rho) & torch.isfinite(sigma) & (rho != 0.0) & (sigma > 0.0)
        alpha = torch.where(ok, rho / torch.where(ok, sigma, one), 0.0 * one).float()
        ad = alpha * d
        z = z + ad
        aq = alpha * q
        r = r - aq
        rho2 = _dot64(r, r)
        beta = torch.where(ok & torch.isfinite(rho2), rho2 / torch.where(ok, rho, one), 0.0 * one).float()
        bd = beta * d
        d = r + bd
        rho = rho2
    mz = z if mask is None else mask * z
    return mz * _f(lam)


def tables(h, f, H, W):
    """(gy, gx) as fp32 tensors from this file's float64 Gram matrices (not the product's psf_gram)"""
    b = half_width(len(h) // 2, f)
    return tuple(torch.from_numpy(bands_of(gram64(h, L, f), b).astype(np.float32)) for L in (H, W))


def project32(p, values, h, f, gy, gx, channels=None, mask=None, lam=1.0, mu=0.0, iters=1):
    """BoundPsf.project with solver = cg: residual with weight 1 -> the solve -> update with step fp32(1 / f^2)"""
    c = PR.residual(p, values, h, f, channels, mask, 1.0)
    q = cg32(c, gy, gx, mask, mu, lam, iters)
    return PR.update(p, q, h, f, channels, _f(1.0 / (f * f)))


def cg_link(values, h, f, gy, gx, channels=None, mask=None, lam=1.0, mu=0.0, iters=1):
    return lambda p: project32(p, values, h, f, gy, gx, channels, mask, lam, mu, iters)
