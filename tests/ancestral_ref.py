"""CPU side of the tests of observations on the ancestral samplers (test infrastructure):

  pred_x0, finish           eod_ddpm_pred_x0 / eod_ddpm_step_p0 in torch fp32, one separately rounded operation per line, in the order
                            include/eodiff.h states (correctly rounded square roots: oracle.sampler_ref._sqrt); a timestep outside [0, T)
                            is computed with index 0 and fills its sample with NaN, as the kernels do;
  step                      pred_x0 -> the links in order -> finish (links: functions prediction -> prediction, tests/spectral_ref.py's
                            obs_link / spec_link, tests/psf_ref.py's psf_link);
  ddpm_sampled              EODiffusion.sampling with an observation as a CPU loop: the walk of tests/repaint_ref.py, the RePaint mix in
                            front of the network, links_of(k) = the links of evaluation number k;
  pred_x0_64, finish64, eps_form64, tables64, ddpm_f64
                            the same step in float64 (numpy), the reference's epsilon form, and the ancestral loop on the Gaussian toy of
                            tests/dpm_ref.py as a 4 x 32 x 32 image with a chain of float64 projectors after every prediction.
"""
import numpy as np
import torch

from oracle import sampler_ref as SR
from tests import consistency_ref as CR
from tests import dpm_ref as DR
from tests import repaint_ref as RR

EPS = float(np.finfo(np.float32).eps)


# ------------------------------------------------------------------------------------------------ the kernels, in torch fp32
def _checked(tb, t):
    """(timesteps with the ones outside [0, T) replaced by 0, which ones those are)"""
    T = tb["alphas_cumprod"].shape[0]
    bad = (t < 0) | (t >= T)
    return torch.where(bad, torch.zeros_like(t), t), bad


def _poison(out, bad):
    out = out.clone()
    out[bad] = float("nan")
    return out


def pred_x0(tb, x, e, t, clip=True):
    """eod_ddpm_pred_x0"""
    assert x.dtype == torch.float32 and e.dtype == torch.float32
    n = x.shape[0]
    tn, bad = _checked(tb, t)
    acp = SR._g(tb["alphas_cumprod"], tn, n)
    r = 1.0 / acp
    c_x0 = SR._sqrt(r)
    rm = r - 1.0
    c_pred = SR._sqrt(rm)
    u = c_x0 * x
    v = c_pred * e
    p0 = u - v
    if clip:
        p0 = torch.clamp(p0, -1.0, 1.0)                                              # (a NaN stays NaN, as clamp_pm1 keeps it)
    return _poison(p0, bad)


def finish(tb, x, p0c, z, t):
    """eod_ddpm_step_p0"""
    assert x.dtype == torch.float32 and p0c.dtype == torch.float32 and z.dtype == torch.float32
    n = x.shape[0]
    tn, bad = _checked(tb, t)
    alpha_t = SR._g(tb["alphas"], tn, n)
    acp = SR._g(tb["alphas_cumprod"], tn, n)
    beta_t = SR._g(tb["betas"], tn, n)
    om = 1.0 - acp
    if t.min() > 0:                                                  # the batch minimum, of the timesteps as given
        acp_prev = SR._g(tb["alphas_cumprod"], (tn - 1).clamp(min=0), n)
        sp = SR._sqrt(acp_prev)
        bp = beta_t * sp
        m_x0 = bp / om
        omp = 1.0 - acp_prev
        sa = SR._sqrt(alpha_t)
        ops = omp * sa
        m_xt = ops / om
        bo = beta_t * omp
        var = bo / om
        std = SR._sqrt(var)
        p = m_x0 * p0c
        q = m_xt * x
        mean = p + q
    else:
        m_x0 = beta_t / om
        std = torch.zeros_like(m_x0)
        mean = m_x0 * p0c
    sz = std * z
    return _poison(mean + sz, bad)


def step(tb, x, e, z, t, links=(), clip=True):
    """(x_prev, the projected prediction)"""
    p = pred_x0(tb, x, e, t, clip)
    for link in links:
        p = link(p)
    return finish(tb, x, p, z, t), p


def ddpm_sampled(tb, eps_fn, x_T, noises, links_of, clip=True, gt=None, mask=None, resample=None, jump_noises=None, record=None):
    """EODiffusion.sampling(observation=...) as a CPU loop: noises[k] belongs to evaluation k of the walk (the mix and the step share it),
    jump_noises[j] to jump j, links_of(k) are the links of evaluation k with their weights taken at k.  record: a list that receives
    (x_t after the mix, estimate, noise, timestep) of every evaluation."""
    T = tb["alphas_cumprod"].shape[0]
    visits, _ = RR.walk_of(T, resample)
    jumps = RR.resample_schedule(T, *resample)[1] if resample is not None else []
    after = {k: (j, a, b) for j, (k, a, b) in enumerate(jumps)}
    acp = tb["alphas_cumprod"]
    x_t, n = x_T, x_T.shape[0]
    for k, i in enumerate(visits):
        t = torch.full((n,), i, dtype=torch.int64)
        if gt is not None:
            x_t = SR.repaint_mix(tb, x_t, gt, mask, t, noises[k])
        e = eps_fn(x_t, t)
        if record is not None:
            record.append((x_t, e, noises[k], i))
        x_t, _ = step(tb, x_t, e, noises[k], t, links_of(k), clip)
        if k + 1 in after:
            j, a, b = after[k + 1]
            x_t = RR.renoise(x_t, jump_noises[j], acp[a].item(), acp[b].item())
    return x_t


# ------------------------------------------------------------------------------------------------ float64
def tables64(tb):
    return {k: v.numpy().astype(np.float64) for k, v in tb.items()}


def pred_x0_64(tb64, x, e, i, clip=False):
    acp = tb64["alphas_cumprod"][i]
    p0 = np.sqrt(1.0 / acp) * x - np.sqrt(1.0 / acp - 1.0) * e
    return np.clip(p0, -1.0, 1.0) if clip else p0


def finish64(tb64, x, p0c, z, i):
    b, a, acp = tb64["betas"][i], tb64["alphas"][i], tb64["alphas_cumprod"][i]
    if i > 0:
        acp_prev = tb64["alphas_cumprod"][i - 1]
        mean = (b * np.sqrt(acp_prev) / (1.0 - acp)) * p0c + ((1.0 - acp_prev) * np.sqrt(a) / (1.0 - acp)) * x
        return mean + np.sqrt(b * (1.0 - acp_prev) / (1.0 - acp)) * z
    return (b / (1.0 - acp)) * p0c


def eps_form64(tb64, x, e, z, i):
    """the reference's unclipped step (model.py:101-122) in float64"""
    b, a, acp = tb64["betas"][i], tb64["alphas"][i], tb64["alphas_cumprod"][i]
    mean = (1.0 / np.sqrt(a)) * (x - ((1.0 - a) / np.sqrt(1.0 - acp)) * e)
    if i > 0:
        acp_prev = tb64["alphas_cumprod"][i - 1]
        return mean + np.sqrt(b * (1.0 - acp_prev) / (1.0 - acp)) * z
    return mean


def ddpm_f64(tb64, noises, links64=()):
    """the ancestral loop t = T - 1 .. 0 on the Gaussian toy as the image CR.TOY_SHAPE, links64 = functions prediction [1, 4, 32, 32] ->
    prediction applied in order after every prediction; noises [T, *TOY_SHAPE].  No clamp.  Returns (end state, last prediction)."""
    mu, s, x = DR.toy()
    T = tb64["betas"].shape[0]
    p0 = None
    for k, i in enumerate(range(T - 1, -1, -1)):
        e = DR.toy_eps(x, tb64["alphas_cumprod"][i], mu, s)
        p0 = pred_x0_64(tb64, x, e, i)
        for link in links64:
            p0 = link(p0.reshape(CR.TOY_SHAPE)).reshape(-1)
        x = finish64(tb64, x, p0, np.asarray(noises[k], np.float64).reshape(-1), i)
    return x, p0
