"""CPU side of the observation-consistency tests (test infrastructure):

  project64, block_mean64   the operator and the projection p0 - lam * mask * (A+ A p0 - values) in float64 (numpy);
  block_mean                eod_block_mean in torch fp32: the block sum in the kernel's order (the first pixel, then each further pixel of
                            the block row by row, left to right, sequential fp32 adds), one division by float(f * f);
  project                   the four operations of the projection in torch fp32;
  ddim_step, dpm_step       eod_ddim_step_obs / eod_dpmpp_step_obs in torch fp32, one separately rounded operation per line, in the style
                            of tests/dpm_ref.py step (a python float times an fp32 tensor is an fp32 multiply by the fp32 value it holds);
  ddim_f64                  tests/dpm_ref.py's float64 DDIM loop on the Gaussian toy with the projector after every prediction;
  ddim_sampled, dpm_sampled whole DDIMSampler.sample / DPMSolverSampler.sample calls with an observation as CPU loops.
"""
import numpy as np
import torch

from oracle import sampler_ref as SR
from tests import dpm_ref as DR
from tests import repaint_ref as RR

S2_FACTORS = (6, 1, 1, 1, 2, 2, 2, 1, 2, 6, 6, 2, 2)   # Sentinel-2 L1C: B1 60 m, B2-B4 10 m, B5-B7 20 m, B8 10 m, B8A 20 m, B9 B10 60 m, B11 B12 20 m
_f = lambda v: float(np.float32(v))


# ------------------------------------------------------------------------------------------------ float64
def block_mean64(x, factors):
    x = np.asarray(x, np.float64)
    out = np.empty_like(x)
    B, C, H, W = x.shape
    for c, f in enumerate(factors):
        m = x[:, c].reshape(B, H // f, f, W // f, f).mean(axis=(2, 4), keepdims=True)
        out[:, c] = np.broadcast_to(m, (B, H // f, f, W // f, f)).reshape(B, H, W)
    return out


def project64(p0, values, factors, mask=None, lam=1.0):
    p0 = np.asarray(p0, np.float64)
    m = 1.0 if mask is None else np.asarray(mask, np.float64)
    return p0 - lam * m * (block_mean64(p0, factors) - np.asarray(values, np.float64))


# ------------------------------------------------------------------------------------------------ the kernels, in torch fp32
def block_mean(p0, factors):
    assert p0.dtype == torch.float32 and p0.dim() == 4 and p0.shape[1] == len(factors)
    B, C, H, W = p0.shape
    out = torch.empty_like(p0)
    for c, f in enumerate(factors):
        v = p0[:, c].reshape(B, H // f, f, W // f, f)
        s = v[:, :, 0, :, 0].clone()
        for r in range(f):
            for j in range(f):
                if r or j:
                    s = s + v[:, :, r, :, j]
        mean = s / float(f * f)
        out[:, c] = mean[:, :, None, :, None].expand(B, H // f, f, W // f, f).reshape(B, H, W)
    return out


def project(p0, values, factors, mask, lam):
    mean = block_mean(p0, factors)
    lm = _f(lam) if mask is None else mask * _f(lam)
    df = mean - values
    t = df * lm
    return p0 - t


def ddim_step(x, e, noise, a_t, a_prev, sigma_t, sqrt_1m_at, temperature, values, factors, mask=None, lam=1.0):
    """(x_prev, pred_x0) of eod_ddim_step_obs; the scalars of ddim_step_kernel with numpy's correctly rounded fp32 sqrt"""
    one = np.float32(1.0)
    sq_at = float(np.sqrt(np.float32(a_t)))
    sig2 = np.float32(sigma_t) * np.float32(sigma_t)
    dcoef = float(np.sqrt((one - np.float32(a_prev)) - sig2))
    sq_ap = float(np.sqrt(np.float32(a_prev)))
    se = e * _f(sqrt_1m_at)
    d = x - se
    p0 = d / sq_at
    dirx = e * dcoef
    if noise is not None:
        sn = noise * _f(sigma_t)
        nz = sn * _f(temperature)
    else:
        nz = float((np.float32(sigma_t) * np.float32(0.0)) * np.float32(temperature))
    p0c = project(p0, values, factors, mask, lam)
    a = p0c * sq_ap
    b = a + dirx
    return b + nz, p0c


def dpm_step(x, e, d_prev, a_s, sqrt_1m_as, c_x, c_d, w_cur, w_prev, clip, values, factors, mask=None, lam=1.0):
    """(x_next, pred_x0) of eod_dpmpp_step_obs: tests/dpm_ref.py step with the projection between the clamp and the combination"""
    se = e * _f(sqrt_1m_as)
    d = x - se
    p0 = d / float(np.sqrt(np.float32(a_s)))
    if clip:
        p0 = torch.clamp(p0, -1.0, 1.0)                                              # (clamp_pm1: a NaN stays NaN)
    p0c = project(p0, values, factors, mask, lam)
    if d_prev is not None:
        u = p0c * _f(w_cur)
        v = d_prev * _f(w_prev)
        D = u + v
    else:
        D = p0c
    p = x * _f(c_x)
    q = D * _f(c_d)
    return p + q, p0c


# ------------------------------------------------------------------------------------------------ the toy, float64
TOY_SHAPE = (1, 4, 32, 32)          # tests/dpm_ref.py's 4096 independent Gaussian pixels as an image
TOY_FACTORS = (1, 2, 4, 8)


def ddim_f64(acp, levels, values=None, mask=None, lam=1.0, factors=TOY_FACTORS):
    """DR.ddim_f64 with the projector applied to every prediction (values None: the unconstrained loop, DR.ddim_f64's operations).
    Returns (end state, last prediction, last estimate)."""
    mu, s, x = DR.toy()
    acp = np.asarray(acp, np.float64)
    p0 = e = None
    for index in range(len(levels) - 1, -1, -1):
        a_s = acp[levels[index]]
        a_t = acp[levels[index - 1]] if index > 0 else acp[0]
        e = DR.toy_eps(x, a_s, mu, s)
        p0 = (x - np.sqrt(1.0 - a_s) * e) / np.sqrt(a_s)
        if values is not None:
            p0 = project64(p0.reshape(TOY_SHAPE), values, factors, mask, lam).reshape(-1)
        x = np.sqrt(a_t) * p0 + np.sqrt(1.0 - a_t) * e
    return x, p0, e


# ------------------------------------------------------------------------------------------------ whole calls as CPU loops
def ddim_sampled(tb, dd, steps, eps_fn, x_T, step_noises, obs, x0=None, mask=None, mix_noises=None, resample=None, jump_noises=None):
    """DDIMSampler.sample with an observation: obs = dict(values, factors, mask, weights[i]); dd = oracle.schedule.ddim_tables;
    the walk of tests/repaint_ref.py.  Returns (end state, last pred_x0)."""
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
                            float(dd["sqrt_1m_a"][index]), 1.0, obs["values"], obs["factors"], obs["mask"], obs["weights"][k])
        if k + 1 in after:
            j, lo, hi = after[k + 1]
            img = RR.renoise(img, jump_noises[j], float(dd["a"][lo]), float(dd["a"][hi]))
    return img, p0


def dpm_sampled(tb, levels, eps_fn, x_T, obs, order=2, clip=False, x0=None, mask=None, mix_noises=None, resample=None, jump_noises=None):
    """DR.dpm_sampled with dpm_step in place of DR.step (first order on the first evaluation, after a jump and at index 0)"""
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
        img, p0 = dpm_step(img, e_t, hist if use else None, a[index], s1m[index], *c, clip, obs["values"], obs["factors"], obs["mask"],
                           obs["weights"][k])
        hist = p0
        if k + 1 in after:
            j, lo, hi = after[k + 1]
            img = RR.renoise(img, jump_noises[j], float(a[lo]), float(a[hi]))
            hist = None
    return img, p0
