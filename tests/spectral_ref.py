"""CPU side of the cross-band observation tests (test infrastructure):

  apply64, project64        A = R (x) D_f and the projection p - lam * mask * A+ (A p - values), A+ = pinv(R) (x) replication, in float64;
  apply, project            eod_spec_apply / eod_spec_project in torch fp32, one separately rounded operation per line, in the order
                            include/eodiff.h states (the block mean is tests/consistency_ref.py block_mean);
  spec_link, obs_link       a link of a chain as a function prediction -> projected prediction (the emulations above / consistency_ref's);
  ddim_step, dpm_step       eod_ddim_step_spec / eod_dpmpp_step_spec, and with several links the unfused route eod_pred_x0 -> projections
                            -> eod_ddim_step_p0 / eod_dpmpp_step_p0 (the same operations), in torch fp32;
  ddim_f64                  the float64 DDIM loop on the Gaussian toy with a chain of float64 projectors after every prediction;
  ddim_sampled, dpm_sampled whole sampler calls with a chain as CPU loops;
  response, pinv32, rcond   seeded response matrices (non-negative rows that sum to one), the fp32 pseudo-inverse the product computes,
                            sigma_min / sigma_max in float64.
"""
import numpy as np
import torch

from oracle import sampler_ref as SR
from tests import consistency_ref as CR
from tests import dpm_ref as DR
from tests import repaint_ref as RR

_f = lambda v: float(np.float32(v))
EPS = float(np.finfo(np.float32).eps)
R3 = np.array([[.6, .3, .1], [.2, .6, .2], [.1, .3, .6]])          # the fixed well-conditioned square matrix
MIN_RCOND = 1e-3                                                     # the product's conditioning refusal


def response(K, C, seed):
    """[K, C] float32, non-negative rows that sum to one (to fp32 rounding); K = C = 3: R3"""
    if (K, C) == (3, 3):
        return R3.astype(np.float32)
    R = np.random.default_rng(seed).random((K, C)) + 0.05
    if K == C:
        R = R + 2.0 * np.eye(K)                                      # (a square random matrix can be arbitrarily close to singular)
    return (R / R.sum(axis=1, keepdims=True)).astype(np.float32)


def rcond(R):
    sv = np.linalg.svd(np.asarray(R, np.float32).astype(np.float64), compute_uv=False)
    return float(sv[-1] / sv[0])


def pinv32(R):
    return np.linalg.pinv(np.asarray(R, np.float32).astype(np.float64)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ float64
def apply64(x, R, f):
    x = np.asarray(x, np.float64)
    return np.einsum("kc,bchw->bkhw", np.asarray(R, np.float64), CR.block_mean64(x, (f,) * x.shape[1]))


def project64(p, values, R, f, mask=None, lam=1.0):
    p = np.asarray(p, np.float64)
    m = 1.0 if mask is None else np.asarray(mask, np.float64)
    G = np.linalg.pinv(np.asarray(R, np.float64))
    return p - lam * m * np.einsum("ck,bkhw->bchw", G, apply64(p, R, f) - np.asarray(values, np.float64))


# ------------------------------------------------------------------------------------------------ the kernels, in torch fp32
def apply(p, R, f):
    """d_k on the full-resolution grid: [B, K, H, W]"""
    assert p.dtype == torch.float32 and p.dim() == 4 and R.shape[1] == p.shape[1]
    mean = CR.block_mean(p, (f,) * p.shape[1])
    out = []
    for k in range(R.shape[0]):
        d = mean[:, 0] * _f(R[k, 0])
        for c in range(1, R.shape[1]):
            pr = mean[:, c] * _f(R[k, c])
            d = d + pr
        out.append(d)
    return torch.stack(out, 1)


def project(p0, values, R, G, f, mask=None, lam=1.0):
    K, C = R.shape
    assert G.shape == (C, K) and values.shape[1] == K and (mask is None or mask.shape[1] == 1)
    d = apply(p0, R, f)
    r = d - values
    lm = _f(lam) if mask is None else mask[:, 0] * _f(lam)
    out = []
    for c in range(C):
        t = r[:, 0] * _f(G[c, 0])
        for k in range(1, K):
            pr = r[:, k] * _f(G[c, k])
            t = t + pr
        q = t * lm
        out.append(p0[:, c] - q)
    return torch.stack(out, 1)


def spec_link(values, R, f=1, mask=None, lam=1.0, G=None):
    R = np.asarray(R, np.float32)
    G = pinv32(R) if G is None else G
    return lambda p: project(p, values, R, G, f, mask, lam)


def obs_link(values, factors, mask=None, lam=1.0):
    return lambda p: CR.project(p, values, factors, mask, lam)


def pred_x0(x, e, a, sqrt_1m_a, clip=False):
    se = e * _f(sqrt_1m_a)
    d = x - se
    p0 = d / float(np.sqrt(np.float32(a)))
    if clip:
        p0 = torch.clamp(p0, -1.0, 1.0)                                              # (clamp_pm1: a NaN stays NaN)
    return p0


def ddim_finish(e, p0c, noise, a_prev, sigma_t, temperature):
    """eod_ddim_step_p0: consistency_ref.ddim_step's lines after the projection"""
    one = np.float32(1.0)
    sig2 = np.float32(sigma_t) * np.float32(sigma_t)
    dcoef = float(np.sqrt((one - np.float32(a_prev)) - sig2))
    sq_ap = float(np.sqrt(np.float32(a_prev)))
    dirx = e * dcoef
    if noise is not None:
        sn = noise * _f(sigma_t)
        nz = sn * _f(temperature)
    else:
        nz = float((np.float32(sigma_t) * np.float32(0.0)) * np.float32(temperature))
    a = p0c * sq_ap
    b = a + dirx
    return b + nz


def dpm_finish(x, p0c, d_prev, c_x, c_d, w_cur, w_prev):
    """eod_dpmpp_step_p0"""
    if d_prev is not None:
        u = p0c * _f(w_cur)
        v = d_prev * _f(w_prev)
        D = u + v
    else:
        D = p0c
    p = x * _f(c_x)
    q = D * _f(c_d)
    return p + q


def ddim_step(x, e, noise, a_t, a_prev, sigma_t, sqrt_1m_at, temperature, links):
    """(x_prev, pred_x0): one link = the fused kernel, several = the unfused route"""
    p = pred_x0(x, e, a_t, sqrt_1m_at)
    for link in links:
        p = link(p)
    return ddim_finish(e, p, noise, a_prev, sigma_t, temperature), p


def dpm_step(x, e, d_prev, a_s, sqrt_1m_as, c_x, c_d, w_cur, w_prev, clip, links):
    p = pred_x0(x, e, a_s, sqrt_1m_as, clip)
    for link in links:
        p = link(p)
    return dpm_finish(x, p, d_prev, c_x, c_d, w_cur, w_prev), p


# ------------------------------------------------------------------------------------------------ the toy, float64
def ddim_f64(acp, levels, links64=()):
    """tests/consistency_ref.py ddim_f64 with a chain: links64 = functions prediction [1, 4, 32, 32] -> prediction, applied in order.
    No links: the unconstrained loop.  Returns (end state, last prediction, last estimate)."""
    mu, s, x = DR.toy()
    acp = np.asarray(acp, np.float64)
    p0 = e = None
    for index in range(len(levels) - 1, -1, -1):
        a_s = acp[levels[index]]
        a_t = acp[levels[index - 1]] if index > 0 else acp[0]
        e = DR.toy_eps(x, a_s, mu, s)
        p0 = (x - np.sqrt(1.0 - a_s) * e) / np.sqrt(a_s)
        for link in links64:
            p0 = link(p0.reshape(CR.TOY_SHAPE)).reshape(-1)
        x = np.sqrt(a_t) * p0 + np.sqrt(1.0 - a_t) * e
    return x, p0, e


# ------------------------------------------------------------------------------------------------ whole calls as CPU loops
def ddim_sampled(tb, dd, steps, eps_fn, x_T, step_noises, links_of, x0=None, mask=None, mix_noises=None, resample=None, jump_noises=None):
    """DDIMSampler.sample with a chain: links_of(k) = the links of evaluation number k (their weights taken at k)"""
    n_lv = len(steps)
    visits, _ = RR.walk_of(n_lv, resample)
    jumps = RR.resample_schedule(n_lv, *resample)[1] if resample is not None else []
    after = {k: (j, lo, hi) for j, (k, lo, hi) in enumerate(jumps)}
    img, n, p0 = x_T, x_T.shape[0], None
    for k, index in enumerate(visits):
        ts = torch.full((n,), int(steps[index]), dtype=torch.long)
        if mask is not None:
            img = SR.q_sample(tb, x0, ts, mix_noises[k]) * mask + (1.0 - mask) * img
        e_t = eps_fn(img, ts)
        img, p0 = ddim_step(img, e_t, step_noises[k], float(dd["a"][index]), float(dd["a_prev"][index]), float(dd["sigma"][index]),
                            float(dd["sqrt_1m_a"][index]), 1.0, links_of(k))
        if k + 1 in after:
            j, lo, hi = after[k + 1]
            img = RR.renoise(img, jump_noises[j], float(dd["a"][lo]), float(dd["a"][hi]))
    return img, p0


def dpm_sampled(tb, levels, eps_fn, x_T, links_of, order=2, clip=False, x0=None, mask=None, mix_noises=None, resample=None, jump_noises=None):
    acp = tb["alphas_cumprod"]
    a, s1m, first, second = DR.tables(acp.numpy(), levels)
    visits, _ = RR.walk_of(len(levels), resample)
    jumps = RR.resample_schedule(len(levels), *resample)[1] if resample is not None else []
    after = {k: (j, lo, hi) for j, (k, lo, hi) in enumerate(jumps)}
    img, n = x_T, x_T.shape[0]
    hist = p0 = None
    for k, index in enumerate(visits):
        ts = torch.full((n,), int(levels[index]), dtype=torch.long)
        if mask is not None:
            img = SR.q_sample(tb, x0, ts, mix_noises[k]) * mask + (1.0 - mask) * img
        e_t = eps_fn(img, ts)
        use = order == 2 and hist is not None and index > 0
        c = second[index] if use else first[index]
        img, p0 = dpm_step(img, e_t, hist if use else None, a[index], s1m[index], *c, clip, links_of(k))
        hist = p0
        if k + 1 in after:
            j, lo, hi = after[k + 1]
            img = RR.renoise(img, jump_noises[j], float(a[lo]), float(a[hi]))
            hist = None
    return img, p0
