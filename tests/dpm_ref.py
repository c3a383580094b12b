"""CPU side of the DPM-Solver++ (2M) tests (test infrastructure):

  toy, toy_eps, toy_exact   Gaussian data with a closed-form denoiser: n independent pixels, pixel k ~ N(mu_k, s_k^2).  The
                            probability-flow ODE is linear per pixel and its exact solution maps x_T at level `top` to
                            sqrt(a0) mu + sqrt(a0 s^2 + 1 - a0) (x_T - sqrt(a_top) mu) / sqrt(a_top s^2 + 1 - a_top) at acp[0];
  dpm_f64, ddim_f64         float64 loops of the sampler and of DDIM with eta 0.  dpm_f64 applies the PRODUCT's make_dpm_timesteps
                            and dpm_coefficients, so a wrong coefficient or grid shows as a wrong error on the toy;
  toy_error                 relative L2 against the exact end state;
  step                      eod_dpmpp_step in plain torch fp32, one separately rounded operation per line;
  dpm_sampled               a whole DPMSolverSampler.sample call as a CPU loop: an eps function (the oracle UNet), `step`, the RePaint
                            mix, the resampling walk of tests/repaint_ref.py with "first order after a jump" (stale=True keeps the
                            history across a jump: the version that must NOT pass).
"""
import numpy as np
import torch

from eo_diffusion_amd.diffusion.util import dpm_coefficients, dpm_lambda, make_dpm_timesteps
from oracle import sampler_ref as SR
from tests import repaint_ref as RR

TOY_N = 4096


def toy():
    """(mu, s, x_T) as float64 arrays"""
    rng = np.random.default_rng(0)
    mu = rng.uniform(-0.8, 0.8, TOY_N)
    s = rng.uniform(0.05, 0.5, TOY_N)
    x_T = np.random.default_rng(1).standard_normal(TOY_N)
    return mu, s, x_T


def toy_eps(x, a, mu, s):
    """E[eps | x_t = x] for x_t = sqrt(a) x_0 + sqrt(1 - a) eps, x_0 ~ N(mu, s^2)"""
    return np.sqrt(1.0 - a) * (x - np.sqrt(a) * mu) / (a * s * s + 1.0 - a)


def toy_exact(acp, top):
    mu, s, x_T = toy()
    a0, a_top = float(acp[0]), float(acp[top])
    return np.sqrt(a0) * mu + np.sqrt(a0 * s * s + 1.0 - a0) * (x_T - np.sqrt(a_top) * mu) / np.sqrt(a_top * s * s + 1.0 - a_top)


def toy_error(got, acp, top):
    want = toy_exact(acp, top)
    return float(np.linalg.norm(np.asarray(got, np.float64).reshape(-1) - want) / np.linalg.norm(want))


def dpm_f64(acp, S, order, discretize, eps_fn=None, x_T=None):
    """(end state, levels): the multistep loop in float64 with the product's grid and coefficients"""
    mu, s, x0_T = toy()
    eps_fn = eps_fn or (lambda x, a: toy_eps(x, a, mu, s))
    x = x0_T if x_T is None else x_T
    acp = np.asarray(acp, np.float64)
    levels = make_dpm_timesteps(discretize, S, acp)
    prev_p0 = h_prev = None
    for index in range(len(levels) - 1, -1, -1):
        a_s = acp[levels[index]]
        a_t = acp[levels[index - 1]] if index > 0 else acp[0]
        p0 = (x - np.sqrt(1.0 - a_s) * eps_fn(x, a_s)) / np.sqrt(a_s)
        second = order == 2 and prev_p0 is not None and index > 0
        c_x, c_d, w_cur, w_prev = dpm_coefficients(a_s, a_t, h_prev if second else None, order, dtype=np.float64)
        D = w_cur * p0 + w_prev * prev_p0 if second else p0
        x = c_x * x + c_d * D
        prev_p0, h_prev = p0, float(dpm_lambda(a_t) - dpm_lambda(a_s))
    return x, levels


def ddim_f64(acp, levels, eps_fn=None):
    """DDIM with eta 0 over `levels` (ascending), a_prev of the lowest = acp[0]"""
    mu, s, x = toy()
    eps_fn = eps_fn or (lambda x, a: toy_eps(x, a, mu, s))
    acp = np.asarray(acp, np.float64)
    for index in range(len(levels) - 1, -1, -1):
        a_s = acp[levels[index]]
        a_t = acp[levels[index - 1]] if index > 0 else acp[0]
        e = eps_fn(x, a_s)
        p0 = (x - np.sqrt(1.0 - a_s) * e) / np.sqrt(a_s)
        x = np.sqrt(a_t) * p0 + np.sqrt(1.0 - a_t) * e
    return x


# ------------------------------------------------------------------------------------------------ the kernel, in torch fp32
def step(x, e, d_prev, a_s, sqrt_1m_as, c_x, c_d, w_cur, w_prev, clip):
    """(x_next, pred_x0) of eod_dpmpp_step: every line one fp32 operation (a python float times an fp32 tensor is an fp32 multiply by
    the fp32 value the float holds); sqrtf(a_s) is numpy's correctly rounded one (oracle.sampler_ref._sqrt explains why)"""
    f = lambda v: float(np.float32(v))
    assert x.dtype == torch.float32 and e.dtype == torch.float32
    se = e * f(sqrt_1m_as)
    d = x - se
    p0 = d / float(np.sqrt(np.float32(a_s)))
    if clip:
        p0 = torch.clamp(p0, -1.0, 1.0)                                          # clamp_pm1 of csrc/ddpm_p0_body.h: a NaN stays NaN
    if d_prev is not None:
        u = p0 * f(w_cur)
        v = d_prev * f(w_prev)
        D = u + v
    else:
        D = p0
    p = x * f(c_x)
    q = D * f(c_d)
    return p + q, p0


def tables(acp, levels):
    """per index of `levels` (ascending): fp32 a_s, fp32 sqrt(1 - a_s), first-order and second-order coefficient tuples"""
    acp = np.asarray(acp, np.float32)
    a = acp[levels]
    a_prev = np.concatenate([acp[:1], a[:-1]])
    s1m = np.sqrt(np.float32(1.0) - a)
    h = dpm_lambda(a_prev) - dpm_lambda(a)
    first = [dpm_coefficients(a[i], a_prev[i]) for i in range(len(levels))]
    second = [dpm_coefficients(a[i], a_prev[i], h[i + 1], 2) if i + 1 < len(levels) else None for i in range(len(levels))]
    return a, s1m, first, second


def dpm_sampled(tb, levels, eps_fn, x_T, order=2, clip=False, x0=None, mask=None, mix_noises=None, resample=None, jump_noises=None,
                stale=False):
    """(end state, last pred_x0, first pred_x0).  First order on the first evaluation, on the evaluation right after a jump (unless
    `stale`), at index 0 and everywhere with order 1."""
    acp = tb["alphas_cumprod"]
    a, s1m, first, second = tables(acp.numpy(), levels)
    visits, _ = RR.walk_of(len(levels), resample)
    jumps = RR.resample_schedule(len(levels), *resample)[1] if resample is not None else []
    after = {k: (j, lo, hi) for j, (k, lo, hi) in enumerate(jumps)}
    img, n = x_T, x_T.shape[0]
    hist, hist_h_index, p0_first = None, None, None
    for k, index in enumerate(visits):
        ts = torch.full((n,), int(levels[index]), dtype=torch.long)
        if mask is not None:
            img = SR.q_sample(tb, x0, ts, mix_noises[k]) * mask + (1.0 - mask) * img
        e_t = eps_fn(img, ts)
        use = order == 2 and hist is not None and index > 0
        if use and hist_h_index != index + 1:        # (stale history: the h of the step that made it)
            a_hi = a[hist_h_index]
            a_lo = a[hist_h_index - 1] if hist_h_index > 0 else np.asarray(acp.numpy(), np.float32)[0]
            c = dpm_coefficients(a[index], a[index - 1], float(dpm_lambda(a_lo) - dpm_lambda(a_hi)), 2)
        else:
            c = second[index] if use else first[index]
        img, p0 = step(img, e_t, hist if use else None, a[index], s1m[index], *c, clip)
        p0_first = p0 if p0_first is None else p0_first
        hist, hist_h_index = p0, index
        if k + 1 in after:
            j, lo, hi = after[k + 1]
            img = RR.renoise(img, jump_noises[j], float(a[lo]), float(a[hi]))
            if not stale:
                hist = None
    return img, p0, p0_first
