"""TEST INFRASTRUCTURE: plain numpy references for the training objective -- the masked, weighted l1 / l2 / huber loss with its gradient
(eod_diffusion_loss), the squared gradient norm (eod_grad_sumsq) and the clipped AdamW update (eod_adamw_step_clipped).  No GPU; checked
on their own in tests/test_train_objective_host.py, used by tests/test_gpu_train_objective.py.

Every function restates the documented definition (include/eodiff.h), not a kernel's index arithmetic:
  d = pred - target;  l2: l = d^2, l' = 2 d;  l1: l = |d|, l' = sign(d) with sign(+-0) = 0;  huber: torch's huber_loss
  S_n = sum_e m_e (a one-channel mask counts once per channel);  L_n = sum_e m_e l(d_e) / S_n (0 where S_n = 0)
  loss = (1/N) sum_n w_n L_n;  dpred_e = (s_n * m_e) * l'(d_e) in float32, s_n = (float)(w_n / (N * S_n)) formed in double
  an element with m_e == 0 is skipped: it adds 0 and its dpred is +0.0 whatever pred / target hold there
The loss terms are float64 from the start (d = (double)pred - (double)target) and are added with math.fsum; the gradient is float32 from
the float32 difference, one rounded operation at a time."""
import math

import numpy as np

from tests.train_tail_ref import adamw_step_scalars

f32, f64 = np.float32, np.float64
KINDS = ("l2", "l1", "huber")


def _sign(d):
    """sign(+-0) = +0; a NaN stays a NaN"""
    return np.where(d > 0, d.dtype.type(1), np.where(d < 0, d.dtype.type(-1), np.where(d == 0, d.dtype.type(0), d)))


def loss_terms(d, kind, delta):
    """l(d) elementwise in d's precision"""
    if kind == "l2":
        return d * d
    a = np.abs(d)
    if kind == "l1":
        return a
    dl = d.dtype.type(delta)
    return np.where(a <= dl, (d.dtype.type(0.5) * d) * d, dl * (a - d.dtype.type(0.5) * dl))


def loss_slope(d, kind, delta):
    """l'(d) elementwise in d's precision"""
    if kind == "l2":
        return d.dtype.type(2) * d
    if kind == "l1":
        return _sign(d)
    dl = d.dtype.type(delta)
    return np.where(np.abs(d) <= dl, d, dl * _sign(d))


def loss_ref(pred, target, mask=None, weight=None, kind="l2", delta=1.0):
    """pred, target [N,C,H,W] float32; mask [N or 1, 1 or C, H, W] float32 or None; weight [N] float32 or None; delta is rounded to
    float32 first (the C ABI takes a float).  Returns dict(loss float32, per_sample [N] float32, dpred [N,C,H,W] float32, and for the
    tolerances loss64, per64 [N], S [N], abs_terms [N] = sum_e |m_e l(d_e)| as float64)"""
    assert kind in KINDS
    pred, target = np.asarray(pred, f32), np.asarray(target, f32)
    N, C, H, W = pred.shape
    E = C * H * W
    delta = float(f32(delta))
    if mask is None:
        m = np.ones((N, C, H, W), f32)
    else:
        m = np.broadcast_to(np.asarray(mask, f32), (N, C, H, W))
    w = np.ones((N,), f32) if weight is None else np.asarray(weight, f32)
    per64, S, abs_terms = np.zeros(N, f64), np.zeros(N, f64), np.zeros(N, f64)
    dpred = np.zeros((N, C, H, W), f32)
    with np.errstate(all="ignore"):
        for n in range(N):
            mn, live = m[n].reshape(E), m[n].reshape(E) != 0
            S[n] = math.fsum(mn.astype(f64).tolist()) if mask is not None else float(E)
            if S[n] <= 0.0:
                continue
            p, t = pred[n].reshape(E)[live], target[n].reshape(E)[live]
            terms = mn[live].astype(f64) * loss_terms(p.astype(f64) - t.astype(f64), kind, delta)
            per64[n] = math.fsum(terms.tolist()) / S[n]
            abs_terms[n] = math.fsum(np.abs(terms).tolist())
            s_n = f32(float(w[n]) / (float(N) * S[n]))
            g = np.zeros(E, f32)
            g[live] = (s_n * mn[live]) * loss_slope(p - t, kind, f32(delta)).astype(f32)
            dpred[n] = g.reshape(C, H, W)
    loss64 = math.fsum((w.astype(f64) * per64).tolist()) / float(N)
    return dict(loss=f32(loss64), per_sample=per64.astype(f32), dpred=dpred, loss64=loss64, per64=per64, S=S, abs_terms=abs_terms)


def grad_sumsq_ref(g):
    """the exact sum of squares, rounded once"""
    g = np.asarray(g, f32).astype(f64).reshape(-1)
    return math.fsum((g * g).tolist())   # (a float32 squared is exact in float64)


def grad_norm_ref(*gs):
    """the norm of the concatenation of the given gradients"""
    return math.sqrt(math.fsum([grad_sumsq_ref(g) for g in gs]))


def clip_coef_ref(total_norm, max_norm):
    """torch.nn.utils.clip_grad_norm_'s rule, rounded to float32"""
    if math.isinf(max_norm):
        return f32(1.0)
    return f32(min(1.0, max_norm / (total_norm + 1e-6)))


def adamw_clipped_ref(p, g, m, v, coef, decay_mul, beta1, beta2, eps, bc2_sqrt, neg_step_size):
    """tests/train_tail_ref.adamw_step_scalars fed g * coef in float32"""
    with np.errstate(all="ignore"):
        gc = np.asarray(g, f32) * f32(coef)
    return adamw_step_scalars(p, gc, m, v, decay_mul, beta1, beta2, eps, bc2_sqrt, neg_step_size)


def loss_weights_ref(alphas_cumprod, kind, gamma=0.0, k=1.0):
    """EODiffusion.loss_weights, one timestep at a time in Python floats"""
    out = []
    for a in np.asarray(alphas_cumprod, f32).astype(f64).tolist():
        if kind == "uniform":
            out.append(1.0)
        elif kind == "min_snr":
            out.append(1.0 if a <= 0.0 else min(1.0, gamma * (1.0 - a) / a))
        else:
            snr = math.inf if a >= 1.0 else a / (1.0 - a)
            out.append((k + snr) ** -gamma if gamma != 0 else 1.0)
    return np.asarray(out, f64).astype(f32)
