"""CPU side of the prediction-target tests (test infrastructure; DESIGN.md sections 8.2 and 9.16):

  pred, ddpm_pred, q_sample_v   eod_param_pred / eod_ddpm_param_pred / eod_q_sample_v in torch fp32, one separately rounded operation per line in
                                the order include/eodiff_param.h states (a python float times an fp32 tensor is an fp32 multiply by the fp32 value
                                the float holds; sqrtf(a) is numpy's correctly rounded one, as tests/dpm_ref.py has it).  kind 1 = x0, 2 = v;
  via_eps                       the route the design rejects, in numpy fp32: the output converted to a noise estimate, then eod_pred_x0's form;
  pred64, eps64, views64        the same quantities in float64 (numpy), and the three outputs (eps, x0, v) that describe one (x, x0, eps);
  ddim_finish, dpm_finish       the `_p0` halves of tests/consistency_ref.py ddim_step and tests/dpm_ref.py step: the update from a given
                                prediction (eod_ddim_step_p0 / eod_dpmpp_step_p0);
  ddim_sampled, dpm_sampled, ddpm_sampled
                                whole DDIMSampler.sample / DPMSolverSampler.sample / EODiffusion.sampling calls of an x0 / v model as CPU loops:
                                an output function (the oracle UNet), pred / ddpm_pred, the links, the finishing half (tests/ancestral_ref.py
                                finish for the ancestral sampler);
  toy_out, dpm_f64, ddim_f64, ddpm_f64
                                the Gaussian toy of tests/dpm_ref.py with a denoiser that returns eps, x0 or v, and the float64 loops under it;
  min_snr64                     the three min-SNR tables in float64, written from their meaning (min(SNR, gamma) over the loss's SNR scale).
"""
import numpy as np
import torch

from eo_diffusion_amd.diffusion.util import dpm_coefficients, dpm_lambda, make_dpm_timesteps
from oracle import sampler_ref as SR
from tests import ancestral_ref as AR
from tests import dpm_ref as DR

X0, V = 1, 2
KINDS = {"eps": 0, "x0": X0, "v": V}
_f = lambda v: float(np.float32(v))


# ------------------------------------------------------------------------------------------------ the kernels, in torch fp32
def _forms(x, o, kind, sa, s1, with_e):
    """(p, e) from sa / s1 as python floats or [N, 1, 1, 1] fp32 tensors"""
    assert x.dtype == torch.float32 and o.dtype == torch.float32 and kind in (X0, V)
    e = None
    if kind == V:
        u = x * sa
        w = o * s1
        p = u - w
        if with_e:
            r = o * sa
            q = x * s1
            e = r + q
    else:
        p = o.clone()
        if with_e:
            u = o * sa
            d = x - u
            e = d / s1
    return p, e


def pred(x, o, kind, a, sqrt_1m_a, clip=False, with_e=True):
    """(p0, e_t) of eod_param_pred; e_t None without with_e"""
    sa = float(np.sqrt(np.float32(a)))
    p, e = _forms(x, o, kind, sa, _f(sqrt_1m_a), with_e)
    if clip:
        p = torch.clamp(p, -1.0, 1.0)                                                # clamp_pm1: a NaN stays NaN
    return p, e


def ddpm_pred(tb, x, o, t, kind, clip=False):
    """eod_ddpm_param_pred: the level of every sample from the two [T] tables; a timestep outside [0, T) fills its sample with NaN"""
    n = x.shape[0]
    tn, bad = AR._checked(tb, t)
    view = (n,) + (1,) * (x.dim() - 1)
    sa = tb["sqrt_alphas_cumprod"].gather(-1, tn).reshape(view)
    s1 = tb["sqrt_one_minus_alphas_cumprod"].gather(-1, tn).reshape(view)
    p, _ = _forms(x, o, kind, sa, s1, False)
    if clip:
        p = torch.clamp(p, -1.0, 1.0)
    return AR._poison(p, bad)


def q_sample_v(tb, x0, noise, t):
    """(x_t, v) of eod_q_sample_v"""
    assert x0.dtype == torch.float32 and noise.dtype == torch.float32
    n = x0.shape[0]
    tn, bad = AR._checked(tb, t)
    view = (n,) + (1,) * (x0.dim() - 1)
    sa = tb["sqrt_alphas_cumprod"].gather(-1, tn).reshape(view)
    s1 = tb["sqrt_one_minus_alphas_cumprod"].gather(-1, tn).reshape(view)
    p = sa * x0
    q = s1 * noise
    x_t = p + q
    r = sa * noise
    w = s1 * x0
    v = r - w
    return AR._poison(x_t, bad), AR._poison(v, bad)


def via_eps(x, v, a, sqrt_1m_a):
    """the prediction of a v output through a noise estimate, numpy fp32: e = (sa * v) + (s1 * x), then eod_pred_x0's (x - (s1 * e)) / sa"""
    x, v = np.asarray(x, np.float32), np.asarray(v, np.float32)
    sa, s1 = np.sqrt(np.float32(a)), np.float32(sqrt_1m_a)
    e = sa * v + s1 * x
    return (x - s1 * e) / sa


# ------------------------------------------------------------------------------------------------ float64
def pred64(x, o, kind, sa, s1):
    """the data prediction in float64 from float64 (sa, s1)"""
    x, o = np.asarray(x, np.float64), np.asarray(o, np.float64)
    return sa * x - s1 * o if kind == V else (o if kind == X0 else (x - s1 * o) / sa)


def eps64(x, o, kind, sa, s1):
    x, o = np.asarray(x, np.float64), np.asarray(o, np.float64)
    return sa * o + s1 * x if kind == V else ((x - sa * o) / s1 if kind == X0 else o)


def views64(x0, eps, a):
    """(x, {kind: the output that describes (x0, eps) at level a}) in float64"""
    sa, s1 = np.sqrt(a), np.sqrt(1.0 - a)
    return sa * x0 + s1 * eps, {0: eps, X0: x0, V: sa * eps - s1 * x0}


def min_snr64(acp, gamma):
    """{kind: min(SNR, gamma) / the scale of that target's loss in SNR} in float64; SNR = a / (1 - a), needs 0 < a < 1"""
    a = np.asarray(acp, np.float64)
    snr = a / (1.0 - a)
    m = np.minimum(snr, gamma)
    return {0: m / snr, X0: m, V: m / (snr + 1.0)}


# ------------------------------------------------------------------------------------------------ the `_p0` halves, in torch fp32
def ddim_finish(e, p0c, noise, a_prev, sigma_t, temperature=1.0):
    """eod_ddim_step_p0: tests/consistency_ref.py ddim_step from its projected prediction on"""
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
    """eod_dpmpp_step_p0: tests/dpm_ref.py step from its prediction on"""
    if d_prev is not None:
        u = p0c * _f(w_cur)
        v = d_prev * _f(w_prev)
        D = u + v
    else:
        D = p0c
    p = x * _f(c_x)
    q = D * _f(c_d)
    return p + q


# ------------------------------------------------------------------------------------------------ whole calls as CPU loops
def _apply(links, p):
    for link in links:
        p = link(p)
    return p


def ddim_sampled(tb, dd, steps, out_fn, kind, x_T, step_noises, links_of=lambda k: (), x0=None, mask=None, mix_noises=None):
    """DDIMSampler.sample of an x0 / v model: dd = oracle.schedule.ddim_tables; out_fn(img, ts) the model's output; step_noises[k] None
    where sigma is 0.  Returns (end state, last pred_x0, first pred_x0)."""
    img, n, p0, first = x_T, x_T.shape[0], None, None
    for k, index in enumerate(range(len(steps) - 1, -1, -1)):
        ts = torch.full((n,), int(steps[index]), dtype=torch.long)
        if mask is not None:
            img = SR.q_sample(tb, x0, ts, mix_noises[k]) * mask + (1.0 - mask) * img
        p0, e = pred(img, out_fn(img, ts), kind, float(dd["a"][index]), float(dd["sqrt_1m_a"][index]))
        p0 = _apply(links_of(k), p0)
        first = p0 if first is None else first
        img = ddim_finish(e, p0, None if step_noises is None else step_noises[k], float(dd["a_prev"][index]), float(dd["sigma"][index]))
    return img, p0, first


def dpm_sampled(tb, levels, out_fn, kind, x_T, order=2, clip=False, links_of=lambda k: (), x0=None, mask=None, mix_noises=None):
    """DPMSolverSampler.sample of an x0 / v model (no resampling): first order on the first evaluation, at index 0 and with order 1.
    Returns (end state, last pred_x0, first pred_x0)."""
    a, s1m, first_c, second_c = DR.tables(tb["alphas_cumprod"].numpy(), levels)
    img, n = x_T, x_T.shape[0]
    hist = p0 = first = None
    for k, index in enumerate(range(len(levels) - 1, -1, -1)):
        ts = torch.full((n,), int(levels[index]), dtype=torch.long)
        if mask is not None:
            img = SR.q_sample(tb, x0, ts, mix_noises[k]) * mask + (1.0 - mask) * img
        p0, _ = pred(img, out_fn(img, ts), kind, a[index], s1m[index], clip, with_e=False)
        p0 = _apply(links_of(k), p0)
        first = p0 if first is None else first
        use = order == 2 and hist is not None and index > 0
        img = dpm_finish(img, p0, hist if use else None, *(second_c[index] if use else first_c[index]))
        hist = p0
    return img, p0, first


def ddpm_sampled(tb, out_fn, kind, x_T, noises, clip=True, links_of=lambda k: (), gt=None, mask=None):
    """EODiffusion.sampling of an x0 / v model: noises[k] belongs to evaluation k (the mix and the step share it)"""
    T = tb["alphas_cumprod"].shape[0]
    x_t, n = x_T, x_T.shape[0]
    for k, i in enumerate(range(T - 1, -1, -1)):
        t = torch.full((n,), i, dtype=torch.int64)
        if gt is not None:
            x_t = SR.repaint_mix(tb, x_t, gt, mask, t, noises[k])
        p = _apply(links_of(k), ddpm_pred(tb, x_t, out_fn(x_t, t), t, kind, clip))
        x_t = AR.finish(tb, x_t, p, noises[k], t)
    return x_t


# ------------------------------------------------------------------------------------------------ the toy, float64
def toy_out(kind):
    """the closed-form denoiser of tests/dpm_ref.py's Gaussian pixels returning eps (0), x0 (1) or v (2): out(x, a) in float64"""
    mu, s, _ = DR.toy()

    def out(x, a):
        e = DR.toy_eps(x, a, mu, s)
        sa, s1 = np.sqrt(a), np.sqrt(1.0 - a)
        p0 = (x - s1 * e) / sa
        return e if kind == 0 else (p0 if kind == X0 else sa * e - s1 * p0)
    return out


def dpm_f64(acp, S, order, discretize, kind):
    """tests/dpm_ref.py dpm_f64 with the prediction formed from the toy's output of `kind`"""
    _, _, x = DR.toy()
    out = toy_out(kind)
    acp = np.asarray(acp, np.float64)
    levels = make_dpm_timesteps(discretize, S, acp)
    prev_p0 = h_prev = None
    for index in range(len(levels) - 1, -1, -1):
        a_s = acp[levels[index]]
        a_t = acp[levels[index - 1]] if index > 0 else acp[0]
        p0 = pred64(x, out(x, a_s), kind, np.sqrt(a_s), np.sqrt(1.0 - a_s))
        second = order == 2 and prev_p0 is not None and index > 0
        c_x, c_d, w_cur, w_prev = dpm_coefficients(a_s, a_t, h_prev if second else None, order, dtype=np.float64)
        D = w_cur * p0 + w_prev * prev_p0 if second else p0
        x = c_x * x + c_d * D
        prev_p0, h_prev = p0, float(dpm_lambda(a_t) - dpm_lambda(a_s))
    return x, levels


def ddim_f64(acp, levels, kind):
    """tests/dpm_ref.py ddim_f64 (eta 0) under the toy's output of `kind`"""
    _, _, x = DR.toy()
    out = toy_out(kind)
    acp = np.asarray(acp, np.float64)
    for index in range(len(levels) - 1, -1, -1):
        a_s = acp[levels[index]]
        a_t = acp[levels[index - 1]] if index > 0 else acp[0]
        o = out(x, a_s)
        sa, s1 = np.sqrt(a_s), np.sqrt(1.0 - a_s)
        x = np.sqrt(a_t) * pred64(x, o, kind, sa, s1) + np.sqrt(1.0 - a_t) * eps64(x, o, kind, sa, s1)
    return x


def ddpm_f64(tb64, noises, kind):
    """tests/ancestral_ref.py ddpm_f64 (no links, no clamp) under the toy's output of `kind`; noises [T, 4096]"""
    _, _, x = DR.toy()
    out = toy_out(kind)
    T = tb64["betas"].shape[0]
    for k, i in enumerate(range(T - 1, -1, -1)):
        a = tb64["alphas_cumprod"][i]
        p0 = pred64(x, out(x, a), kind, np.sqrt(a), np.sqrt(1.0 - a))
        x = AR.finish64(tb64, x, p0, np.asarray(noises[k], np.float64).reshape(-1), i)
    return x
