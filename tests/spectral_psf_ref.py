"""CPU side of the cross-band PSF observation tests (test infrastructure), A = R (x) A_s with A_s = D_f N^-1 B0:

  mix, apply, residual, update   eod_psf_apply_mix / eod_psf_residual_mix / eod_psf_update_mix in torch fp32, one separately rounded
                            operation per line in the order include/eodiff.h states: the band (or channel) sum first product then
                            sequential adds, then psf_ref's blur / norm and consistency_ref's block mean on the mixed planes;
  step32, project           the Landweber link of BoundPsf with a response: step = fp32(tau / sigma_max(R)^2 / f^2), iters x (residual,
                            update with G = R^T);
  project_cg, cg_link       the cg link: residual (weight 1) -> psf_cg_ref.cg32 on the K planes under the shared mask -> update with
                            G = pinv(R) (float64 pseudo-inverse rounded once to fp32) and step fp32(1 / f^2);
  operator64, apply64, adjoint64, dense_correction64   kron(R, line64(H), line64(W)) as a dense float64 matrix, its action and adjoint by
                            einsum, and the exact projection's correction by a dense solve: lstsq on the masked rows (undamped, the minimum
                            norm correction), ((R R^T) (x) (M G M + mu I))^-1 on the observed pixels (damped);
  landweber64, cg64, *_link64    the two links in float64 for the toy loop.
"""
import numpy as np
import torch

from tests import psf_cg_ref as GR
from tests import psf_ref as PR

_f = lambda v: float(np.float32(v))


def r32(R):
    return np.ascontiguousarray(R, dtype=np.float32)


def pinv32(R):
    return np.ascontiguousarray(np.linalg.pinv(r32(R).astype(np.float64)), dtype=np.float32)


def smax64(R):
    return float(np.linalg.svd(r32(R).astype(np.float64), compute_uv=False)[0])


# ------------------------------------------------------------------------------------------------ the kernels, in torch fp32
def mix(x, M):
    """[B, rows, h, w] from x [B, cols, h, w] and M [rows][cols]: M[i][0] * x_0, then + (M[i][j] * x_j) for j = 1 .. in order"""
    assert x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == len(M[0])
    out = []
    for row in M:
        acc = x[:, 0] * _f(row[0])
        for j in range(1, len(row)):
            pr = x[:, j] * _f(row[j])
            acc = acc + pr
        out.append(acc)
    return torch.stack(out, 1).contiguous()


def apply(p, h, f, R):
    """eod_psf_apply_mix: [B, K, H / f, W / f]"""
    return PR.apply(mix(p, r32(R)), h, f)


def residual(p, values, h, f, R, mask=None, lam=1.0):
    """eod_psf_residual_mix"""
    return PR.residual(mix(p, r32(R)), values, h, f, None, mask, lam)


def update(p, q, h, f, G, step=1.0):
    """eod_psf_update_mix: every channel is written"""
    return PR.update(p, mix(q, r32(G)), h, f, None, step)


def step32(h, f, H, W, R):
    return _f(PR.tau64(h, f, H, W) / smax64(R) ** 2 / (f * f))


def project(p, values, h, f, R, mask=None, lam=1.0, iters=1, step=None):
    """BoundPsf.project with a response, solver = landweber"""
    step = step32(h, f, *p.shape[2:], R) if step is None else step
    Rt = r32(R).T
    for _ in range(iters):
        p = update(p, residual(p, values, h, f, R, mask, lam), h, f, Rt, step)
    return p


def project_cg(p, values, h, f, gy, gx, R, mask=None, lam=1.0, mu=0.0, iters=1):
    """BoundPsf.project with a response, solver = cg"""
    c = residual(p, values, h, f, R, mask, 1.0)
    q = GR.cg32(c, gy, gx, mask, mu, lam, iters)
    return update(p, q, h, f, pinv32(R), _f(1.0 / (f * f)))


def link(values, h, f, R, mask=None, lam=1.0, iters=1):
    return lambda p: project(p, values, h, f, R, mask, lam, iters)


def cg_link(values, h, f, gy, gx, R, mask=None, lam=1.0, mu=0.0, iters=1):
    return lambda p: project_cg(p, values, h, f, gy, gx, R, mask, lam, mu, iters)


# ------------------------------------------------------------------------------------------------ float64
def operator64(R, h, f, H, W):
    """A [K Hc Wc, C H W] = kron(R, A1(H), A1(W)), R the fp32 entries"""
    return np.kron(r32(R).astype(np.float64), np.kron(PR.line64(h, H, f)[0], PR.line64(h, W, f)[0]))


def apply64(x, h, f, R):
    return PR.apply64(np.einsum("kc,bchw->bkhw", r32(R).astype(np.float64), np.asarray(x, np.float64)), h, f)


def adjoint64(q, h, f, H, W, R):
    """A^T q: [B, C, H, W]"""
    return np.einsum("kc,bkhw->bchw", r32(R).astype(np.float64), PR.adjoint64(q, h, f, H, W))


def _mask64(mask, shape):
    return np.ones(shape) if mask is None else np.broadcast_to(np.asarray(mask, np.float64), shape)


def dense_correction64(p, values, h, f, R, mask=None, mu=0.0):
    """(correction [B, C, H, W], c): out - p of the exact projection by a dense float64 solve, sample by sample, and its right-hand side
    c = M (A p - values).  mu = 0: -lstsq(M A, c), the minimum-norm solution on the rows the binary mask keeps.  mu > 0: -A^T M z with
    ((R R^T) (x) (M G M + mu I)) z = c on those rows."""
    p = np.asarray(p, np.float64)
    B, C, H, W = p.shape
    R64 = r32(R).astype(np.float64)
    K = R64.shape[0]
    A = operator64(R, h, f, H, W)
    c = apply64(p, h, f, R) - np.asarray(values, np.float64)
    m = _mask64(mask, (B, 1, H // f, W // f))
    c = m * c
    out = np.zeros_like(p)
    for b in range(B):
        rows = np.flatnonzero(np.broadcast_to(m[b], (K, H // f, W // f)).ravel() != 0.0)
        Ar, cr = A[rows], c[b].ravel()[rows]
        if mu == 0.0:
            d = np.linalg.lstsq(Ar, cr, rcond=None)[0]
        else:
            pix = np.flatnonzero(m[b, 0].ravel() != 0.0)
            G = np.kron(GR.gram64(h, H, f), GR.gram64(h, W, f))[np.ix_(pix, pix)]
            S = np.kron(R64 @ R64.T, G + mu * np.eye(pix.size))
            d = Ar.T @ np.linalg.solve(S, cr)
        out[b] = -d.reshape(C, H, W)
    return out, c


def landweber64(p, values, h, f, R, mask=None, lam=1.0, iters=1):
    p = np.array(p, np.float64)
    H, W = p.shape[2:]
    tau = PR.tau64(h, f, H, W) / smax64(R) ** 2
    m = 1.0 if mask is None else np.asarray(mask, np.float64)
    for _ in range(iters):
        p = p - lam * tau * adjoint64(m * (apply64(p, h, f, R) - np.asarray(values, np.float64)), h, f, H, W, R)
    return p


def cg64(p, values, h, f, R, mask=None, lam=1.0, mu=0.0, iters=1):
    """p - lam (pinv(R) (x) A_s^T) (m z), (M G M + mu I) z_k = m (A p - values)_k by `iters` float64 CG iterations per plane"""
    p = np.array(p, np.float64)
    H, W = p.shape[2:]
    m = 1.0 if mask is None else np.asarray(mask, np.float64)
    c = m * (apply64(p, h, f, R) - np.asarray(values, np.float64))
    z = GR.cg64(c, GR.gram64(h, H, f), GR.gram64(h, W, f), mask, mu, iters)
    return p - lam * np.einsum("ck,bkhw->bchw", np.linalg.pinv(r32(R).astype(np.float64)), PR.adjoint64(m * z, h, f, H, W))


def link64(values, h, f, R, mask=None, lam=1.0, iters=1):
    return lambda p: landweber64(p, values, h, f, R, mask, lam, iters)


def cg_link64(values, h, f, R, mask=None, lam=1.0, mu=0.0, iters=1):
    return lambda p: cg64(p, values, h, f, R, mask, lam, mu, iters)
