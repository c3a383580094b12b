"""CPU side of the learned-variance tests (test infrastructure; DESIGN.md sections 8.3 and 9.17):

  tables64                      the per-timestep levels in float64 (numpy) from the fp32 tables, written from the issue's definitions:
                                beta~_t, lmin, gap, c1, and the two fp32 tables of the step kernel;
  sigma, sigma_direct, sigma64  the per-element standard deviation: the kernel's form in torch fp32 (one separately rounded operation per line,
                                torch's expf), the form the design rejects (expf(0.5 (frac lmax + (1 - frac) lmin))), and float64;
  var_pred, var_step            eod_ddpm_var_pred / eod_ddpm_step_p0_var in torch fp32: the mean half through tests/ancestral_ref.py pred_x0 or
                                tests/param_ref.py ddpm_pred, the step as tests/ancestral_ref.py finish with sigma per element;
  p0_64, vlb64, hybrid64        the float64 prediction of the mean half, the variational-bound term of every element with its derivative
                                with respect to v and the sum of the absolute values of its summands (what a float64 evaluation's rounding
                                error is proportional to), and the whole objective with both gradients;
  vlb_torch                     the same term as a torch float64 expression, for autograd;
  sampled                       EODiffusion.sampling of a learned-variance model as a CPU loop.
"""
import math

import numpy as np
import torch

from oracle import sampler_ref as SR
from tests import ancestral_ref as AR
from tests import param_ref as PR

LN2 = math.log(2.0)
CLAMP = 1e-12
_erfc = np.vectorize(math.erfc, otypes=[np.float64])


# ------------------------------------------------------------------------------------------------ the levels
def tables64(tb):
    """tb: {"betas", "alphas_cumprod"[, ...]} fp32 torch tables [T]"""
    b = tb["betas"].numpy().astype(np.float64)
    a = tb["alphas_cumprod"].numpy().astype(np.float64)
    assert b.shape == a.shape and b.size >= 2
    a_prev = np.concatenate([[1.0], a[:-1]])
    bt = b * (1.0 - a_prev) / (1.0 - a)
    bt[0] = bt[1]
    assert np.isfinite(bt).all() and (bt > 0).all()
    lmin = np.log(bt)
    gap = np.log(b) - lmin
    out = {"beta_tilde": bt, "lmin": lmin, "gap": gap, "c1": b * np.sqrt(a_prev) / (1.0 - a),
           "sigma_min": torch.from_numpy(np.sqrt(bt).astype(np.float32)), "half_gap": torch.from_numpy((gap / 2.0).astype(np.float32))}
    for k in ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod"):
        if k in tb:
            out[k] = tb[k].numpy().astype(np.float64)
    return out


# ------------------------------------------------------------------------------------------------ sigma
def sigma(v, sigma_min, half_gap):
    """the kernel's form; sigma_min / half_gap: fp32 tensors that broadcast against v"""
    assert v.dtype == torch.float32
    s = v + 1.0
    frac = s * 0.5
    arg = frac * half_gap
    e = torch.exp(arg)
    return sigma_min * e


def sigma_direct(v, lmin32, lmax32):
    """the rejected form: expf(0.5 * (frac * lmax + (1 - frac) * lmin)) from fp32 tables of the two logarithms"""
    frac = (v + 1.0) * 0.5
    a = frac * lmax32
    b = (1.0 - frac) * lmin32
    return torch.exp(0.5 * (a + b))


def sigma64(v, lmin, gap):
    return np.exp(0.5 * (lmin + (np.asarray(v, np.float64) + 1.0) * 0.5 * gap))


# ------------------------------------------------------------------------------------------------ the two sampling kernels, torch fp32
def var_pred(tb, x, o, t, kind, clip):
    """eod_ddpm_var_pred: o [N, 2, chw] (or [N, 2 C, ...]); the variance half is not touched"""
    mean = o.reshape(o.shape[0], 2, -1)[:, 0].reshape(x.shape).contiguous()
    if kind == 0:
        return AR.pred_x0(tb, x, mean, t, clip)
    return PR.ddpm_pred(tb, x, mean, t, kind, clip)


def var_step(tb, vt, x, p0c, o, z, t):
    """eod_ddpm_step_p0_var; vt = tables64(tb)"""
    assert x.dtype == torch.float32 and p0c.dtype == torch.float32 and z.dtype == torch.float32 and o.dtype == torch.float32
    n = x.shape[0]
    if not t.min() > 0:
        return AR.finish(tb, x, p0c, z, t)                           # std = 0 for the whole batch: v is not read
    tn, bad = AR._checked(tb, t)
    v = o.reshape(n, 2, -1)[:, 1].reshape(x.shape)
    alpha_t = SR._g(tb["alphas"], tn, n)
    acp = SR._g(tb["alphas_cumprod"], tn, n)
    beta_t = SR._g(tb["betas"], tn, n)
    om = 1.0 - acp
    acp_prev = SR._g(tb["alphas_cumprod"], (tn - 1).clamp(min=0), n)
    sp = SR._sqrt(acp_prev)
    bp = beta_t * sp
    m_x0 = bp / om
    omp = 1.0 - acp_prev
    sa = SR._sqrt(alpha_t)
    ops = omp * sa
    m_xt = ops / om
    p = m_x0 * p0c
    q = m_xt * x
    mean = p + q
    std = sigma(v, SR._g(vt["sigma_min"], tn, n), SR._g(vt["half_gap"], tn, n))
    sz = std * z
    return AR._poison(mean + sz, bad)


def sampled(tb, out_fn, kind, x_T, noises, clip=True, links_of=lambda k: ()):
    """EODiffusion.sampling of a learned-variance model: out_fn(x_t, t) -> [N, 2 C, H, W]"""
    vt = tables64(tb)
    T = tb["alphas_cumprod"].shape[0]
    x_t, n = x_T, x_T.shape[0]
    for k, i in enumerate(range(T - 1, -1, -1)):
        t = torch.full((n,), i, dtype=torch.int64)
        o = out_fn(x_t, t)
        p = var_pred(tb, x_t, o, t, kind, clip)
        for link in links_of(k):
            p = link(p)
        x_t = var_step(tb, vt, x_t, p, o, noises[k], t)
    return x_t


# ------------------------------------------------------------------------------------------------ the loss, float64
def p0_64(kind, x_t, o, sa, s1):
    """the unclamped prediction of the mean half; sa / s1: the fp32 buffers' values as float64"""
    if kind == PR.X0:
        return np.array(o, np.float64)
    if kind == PR.V:
        return sa * x_t - s1 * o
    return (x_t - s1 * o) / sa


def _pdf(z):
    return np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def vlb64(x0, p0, v, t0, c1, lmin, gap, h=1.0 / 255.0):
    """(term, d term / d v, scale, edge) of every element, float64.  t0: the sample is at t = 0.  scale: the sum of the absolute values of
    the term's summands, each times 1 + the magnitude of the argument of its exp / erfc (a relative error u of the argument is a relative
    error |argument| u of the function), so that a float64 evaluation is within a small multiple of 2^-53 * scale; for the t = 0 branch the
    summands are the two distribution values over P (the condition of the logarithm) and the logarithm itself.  edge: the element's P,
    or inf for t > 0 (the test refuses elements whose P is within a factor 2 of the clamp)."""
    x0, p0, v = (np.asarray(a, np.float64) for a in (x0, p0, v))
    frac = (v + 1.0) * 0.5
    up = frac * gap
    lv = lmin + up
    if not t0:
        dmu = c1 * (x0 - p0)
        r = np.exp(-up)
        w = np.exp(-lv)
        q = dmu * dmu * w
        term = 0.5 * (((-1.0 + up) + r) + q) / LN2
        dlv = 0.5 * ((1.0 - r) - q) / LN2
        scale = 0.5 * (1.0 + np.abs(up) + r * (1.0 + np.abs(up)) + q * (3.0 + np.abs(lv))) / LN2
        return term, dlv * (0.5 * gap), scale, np.full(term.shape, np.inf)
    c = x0 - c1 * p0
    inv_std = np.exp(-0.5 * lv)
    plus, minus = inv_std * (c + h), inv_std * (c - h)
    lo, hi = x0 < -0.999, x0 > 0.999
    cdf_p, cdf_m = 0.5 * _erfc(-plus * math.sqrt(0.5)), 0.5 * _erfc(-minus * math.sqrt(0.5))
    tail_m = 0.5 * _erfc(minus * math.sqrt(0.5))
    P = np.where(lo, cdf_p, np.where(hi, tail_m, cdf_p - cdf_m))
    dP = np.where(lo, -0.5 * plus * _pdf(plus), np.where(hi, 0.5 * minus * _pdf(minus), -0.5 * (plus * _pdf(plus) - minus * _pdf(minus))))
    live = P > CLAMP
    Pc = np.where(live, P, CLAMP)
    term = -np.log(Pc) / LN2
    dlv = np.where(live, -(dP / Pc) / LN2, 0.0)
    # the arguments plus / minus carry the relative error of exp(-lv / 2) and of two additions and a product: (3 + |lv| / 2) u
    arg_err = 3.0 + 0.5 * np.abs(lv)
    used_p, used_m = np.where(hi, 0.0, 1.0), np.where(lo, 0.0, 1.0)
    val_p, val_m = cdf_p, np.where(hi, tail_m, cdf_m)
    num = used_p * (val_p + arg_err * np.abs(plus) * _pdf(plus)) + used_m * (val_m + arg_err * np.abs(minus) * _pdf(minus))
    scale = (num / Pc + np.abs(np.log(Pc))) / LN2
    return term, dlv * (0.5 * gap), scale, P


def vlb_torch(x0, p0, v, t0, c1, lmin, gap, h=1.0 / 255.0):
    """the term as a torch float64 expression of v (autograd), from the issue's formulas and not from vlb64's lines"""
    lv = lmin + (v + 1.0) / 2.0 * gap
    if not t0:
        d = c1 * (x0 - p0)
        return 0.5 * (-1.0 + lv - lmin + torch.exp(lmin - lv) + d * d * torch.exp(-lv)) / LN2
    Phi = lambda z: 0.5 * torch.special.erfc(-z / math.sqrt(2.0))
    c = x0 - c1 * p0
    plus, minus = (c + h) * torch.exp(-0.5 * lv), (c - h) * torch.exp(-0.5 * lv)
    floor = torch.full_like(plus, CLAMP)
    logp = torch.where(x0 < -0.999, torch.log(torch.maximum(Phi(plus), floor)),
                       torch.where(x0 > 0.999, torch.log(torch.maximum(1.0 - Phi(minus), floor)),
                                   torch.log(torch.maximum(Phi(plus) - Phi(minus), floor))))
    return -logp / LN2


def simple64(d, kind, delta):
    a = np.abs(d)
    if kind == "l2":
        return d * d
    if kind == "l1":
        return a
    return np.where(a <= delta, 0.5 * d * d, delta * (a - 0.5 * delta))


def hybrid64(vt, o, target, x0, x_t, t, kind_param, mask=None, weight=None, kind="l2", delta=1.0, lam=1e-3, h=1.0 / 255.0):
    """the whole objective in float64 from fp32 inputs (numpy arrays; o [N, 2 C, H, W]).  Returns a dict: loss, simple [N], vlb [N], gv (the
    gradient of the variance half, float64), term / scale / edge per element and vlb_scale [N] (the masked mean of scale)."""
    o, target, x0, x_t = (np.asarray(a, np.float64) for a in (o, target, x0, x_t))
    N, C = target.shape[:2]
    mean, v = o[:, :C], o[:, C:]
    m = np.ones_like(target) if mask is None else np.broadcast_to(np.asarray(mask, np.float64), target.shape)
    w = np.ones(N) if weight is None else np.asarray(weight, np.float64)
    out = {k: np.zeros(N) for k in ("simple", "vlb", "vlb_scale")}
    out.update({k: np.zeros_like(target) for k in ("gv", "term", "scale")})
    out["edge"] = np.full(target.shape, np.inf)
    for n in range(N):
        tn = int(t[n])
        S = m[n].sum()
        keep = m[n] != 0
        if S <= 0:
            continue
        p0 = p0_64(kind_param, x_t[n], mean[n], vt["sqrt_alphas_cumprod"][tn], vt["sqrt_one_minus_alphas_cumprod"][tn])
        with np.errstate(all="ignore"):
            term, dv, scale, edge = vlb64(x0[n], p0, v[n], tn == 0, vt["c1"][tn], vt["lmin"][tn], vt["gap"][tn], h)
            sterm = simple64(mean[n] - target[n], kind, delta)
        out["simple"][n] = np.where(keep, m[n] * sterm, 0.0).sum() / S
        out["vlb"][n] = np.where(keep, m[n] * term, 0.0).sum() / S
        out["vlb_scale"][n] = np.where(keep, m[n] * scale, 0.0).sum() / S
        out["gv"][n] = np.where(keep, (lam / (N * S)) * m[n] * dv, 0.0)
        out["term"][n], out["scale"][n], out["edge"][n] = np.where(keep, term, 0.0), np.where(keep, scale, 0.0), np.where(keep, edge, np.inf)
    out["loss"] = float((w * out["simple"] + lam * out["vlb"]).sum() / N)
    return out


def check_conditions(ref, x0, mean_minus, lv):
    """the issue's conditions on the inputs of a gradient comparison: no used P within a factor 2 of the clamp, |x_0 - mu| exp(-lv / 2) <= 6"""
    edge = ref["edge"]
    assert not ((edge > CLAMP / 2.0) & (edge < CLAMP * 2.0)).any(), "an element's P lies within a factor 2 of the 1e-12 clamp"
    assert (np.abs(mean_minus) * np.exp(-0.5 * lv) <= 6.0).all(), "|x_0 - mu_theta| exp(-lv / 2) > 6"
