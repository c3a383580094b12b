"""Observation-consistent sampling: the host-side description of a block-mean observation and the calls of the fused kernels that impose
it (eod_ddim_step_obs, eod_dpmpp_step_obs, eod_block_mean in csrc/sampler.hip).  No counterpart in the reference; DESIGN.md section 9.5.

What is known about channel c is its mean over every f_c x f_c block (f_c = 1: the channel at full resolution), where a mask says so.
With A = masked per-channel block mean and A+ = replication, every evaluation of DDIMSampler / DPMSolverSampler replaces its data
prediction p0 by p0 - weight * mask * (A+ A p0 - values) before the update uses it: the range / null-space projection of DDNM
(Wang et al. 2022) fused into the step kernel.  Per pixel, what the kernel computes for ANY values / mask is stated in include/eodiff.h;
it is the projection when values and mask are constant on every block and the mask is 0 or 1.

SpectralObservation is the observation that mixes bands: K known linear mixes `response` [K, C] of the channels'
f x f block means (a panchromatic band, a second sensor's broad bands), A = R (x) D_f, A+ = pinv(R) (x) replication, imposed by
eod_ddim_step_spec / eod_dpmpp_step_spec.  `observation=` also takes a list of 1 .. 4 observations of either kind, a chain: every
evaluation forms its prediction (eod_pred_x0), projects it by one link after the other (eod_spec_project / eod_obs_project, each with its
own weight) and finishes the step from the result (eod_ddim_step_p0 / eod_dpmpp_step_p0).  A list of one takes the fused kernel.

SeparablePsf gives a PsfObservation one tap vector per axis, asymmetric ones allowed: an anisotropic or shifted PSF
(eod_psf_residual_xy, eod_psf_update_xy; A^T is the correlation with the reversed taps).

PsfObservation is the observation through a sensor's point spread function: A = D_f N^-1 B0, a renormalised
zero-padded separable blur followed by the f x f block mean, with values and mask on the COARSE grid.  A+ has no local form, so the link
takes `iters` Landweber steps p <- p - weight * tau * A^T(mask * (A p - values)) per evaluation (eod_psf_residual, eod_psf_update;
csrc/psf.hip).  It is a link like the others; alone it runs as a chain of one through the unfused ends.  With solver="cg" (DESIGN.md
section 9.9) the link lands on its constraint instead: p - weight * A^T z with (M A A^T M + damping I) z = mask * (A p - values) solved by
`iters` conjugate-gradient iterations on the coarse grid (eod_psf_cg; csrc/psf_cg.hip), where A A^T is a separable banded stencil (psf_gram).
With `response=` [K, C] the link observes K band mixes through the PSF, A = R (x) A_s: a panchromatic band with its
own MTF, a second sensor's broad bands on that sensor's grid (eod_psf_residual_mix, eod_psf_update_mix; M A A^T M = (R R^T) (x) (M_s G M_s), so
the exact projection stays K independent plane solves of the unchanged eod_psf_cg).

The ancestral samplers (EODiffusion.sampling / sampling_scene) take the same observations through ddpm_step below:
eod_ddpm_pred_x0, every link's project(k, p) in order, eod_ddpm_step_p0 -- the clipped DDPM step cut where its prediction is complete.
There is no fused kernel on that route; a single link is a chain of one.  shard(n_total, lo, hi) of the three classes cuts an observation
of a batch to the samples [lo, hi) (dist.sharded_sampling / sharded_sampling_scene).
"""
import copy
import ctypes
import math
import numbers

import numpy as np
import torch

from .. import _lib
from ..engine import current_stream_ptr, f32c, require_gpu

MAX_FACTOR = 8
MAX_CHANNELS = 32
MAX_ROWS = 8            # rows of a response matrix (EOD_SPEC_MAXK of csrc/sampler.hip)
MAX_LINKS = 4           # observations in one chain
MAX_RADIUS = 12         # of a PSF's taps (PSF_MAXR of csrc/psf_body.h)
MAX_ITERS = 8           # Landweber steps of a PsfObservation per evaluation
MAX_CG_ITERS = 64       # conjugate-gradient iterations of a PsfObservation(solver="cg") per evaluation (CG_MAX_ITERS of csrc/psf_cg_body.h)
PARAMETERIZATIONS = ("eps", "x0", "v")   # what a model's output is; the index is the `kind` of eod_param_pred / eod_ddpm_param_pred


def parameterization_kind(what, parameterization):
    """0 / 1 / 2 for "eps" / "x0" / "v"; anything else is refused"""
    if not isinstance(parameterization, str) or parameterization not in PARAMETERIZATIONS:
        raise _lib.EodError(f"{what}: parameterization is one of {PARAMETERIZATIONS}, got {parameterization!r}")
    return PARAMETERIZATIONS.index(parameterization)
SOLVERS = ("landweber", "cg")
MIN_RCOND = 1e-3        # sigma_min / sigma_max of a response matrix below which it is refused (the fp32 residual
                        # of the projection grows with the conditioning, 0.55 eps at cond 45 and 11.6 eps at cond 268)


def _factors(what, factors):
    try:
        fs = list(factors)
    except TypeError:
        raise _lib.EodError(f"{what}: `factors` is a sequence of one block edge per channel, got {factors!r}") from None
    if not 1 <= len(fs) <= MAX_CHANNELS:
        raise _lib.EodError(f"{what}: `factors` has one entry per channel, 1 .. {MAX_CHANNELS} of them; got {len(fs)}")
    for f in fs:
        if isinstance(f, bool) or not isinstance(f, numbers.Integral) or not 1 <= f <= MAX_FACTOR:
            raise _lib.EodError(f"{what}: a factor is an integer in 1 .. {MAX_FACTOR}, got {f!r}")
    return tuple(int(f) for f in fs)


def _divides(what, factors, H, W):
    for c, f in enumerate(factors):
        if H % f or W % f:
            raise _lib.EodError(f"{what}: factors[{c}] = {f} does not divide {H} x {W}")


def _c_factors(factors):
    return (ctypes.c_int32 * len(factors))(*factors)


def _weights(what, weight):
    """([fp32-rounded weights], one per evaluation?) of a `weight` argument: a float in [0, 1] or a sequence of them"""
    if isinstance(weight, (numbers.Real, np.floating)) and not isinstance(weight, bool):
        ws, per_evaluation = [weight], False
    else:
        try:
            ws = list(weight)
        except TypeError:
            raise _lib.EodError(f"{what}: `weight` is a float or a sequence of floats, got {weight!r}") from None
        per_evaluation = True
    for w in ws:
        if isinstance(w, bool) or not isinstance(w, (numbers.Real, np.floating)) or not math.isfinite(float(w)):
            raise _lib.EodError(f"{what}: a weight is a finite float, got {w!r}")
        if not 0.0 <= float(np.float32(w)) <= 1.0:
            raise _lib.EodError(f"{what}: a weight lies in [0, 1], got {w!r}")
    return [float(np.float32(w)) for w in ws], per_evaluation


def _response(what, response):
    """the response matrix [K, C] as the fp32 array the kernels use; shape, dtype, limits and finiteness refused here"""
    try:
        R = np.asarray(response.detach().cpu().numpy() if torch.is_tensor(response) else response)
    except Exception:
        raise _lib.EodError(f"{what}: `response` is array-like [K, C], got {type(response).__name__}") from None
    if R.dtype == np.bool_ or not (np.issubdtype(R.dtype, np.floating) or np.issubdtype(R.dtype, np.integer)):
        raise _lib.EodError(f"{what}: `response` must hold real numbers, got dtype {R.dtype}")
    if R.ndim != 2 or 0 in R.shape:
        raise _lib.EodError(f"{what}: `response` is [K, C] (K observed bands as mixes of C channels), got shape {R.shape}")
    K, C = R.shape
    if C > MAX_CHANNELS or K > MAX_ROWS or K > C:
        raise _lib.EodError(f"{what}: `response` [K, C] needs K <= min(C, {MAX_ROWS}) and C <= {MAX_CHANNELS}, got {K} x {C}")
    with np.errstate(over="ignore"):
        R = np.ascontiguousarray(R, dtype=np.float32)
    if not np.isfinite(R).all():
        raise _lib.EodError(f"{what}: `response` has a non-finite entry (as float32)")
    return R


def _conditioned(what, response):
    """(R, pinv): _response's fp32 [K, C] under the conditioning rule (sigma_min >= MIN_RCOND sigma_max, float64 SVD of the fp32 entries) and
    its float64 pseudo-inverse [C, K] rounded once to fp32"""
    R = _response(what, response)
    sv = np.linalg.svd(R.astype(np.float64), compute_uv=False)
    if not (sv[0] > 0.0 and sv[-1] >= MIN_RCOND * sv[0]):
        raise _lib.EodError(f"{what}: `response` is too badly conditioned to project with in fp32 (sigma_min {sv[-1]:.3g} < "
                            f"{MIN_RCOND:g} * sigma_max {sv[0]:.3g}); rows must be linearly independent")
    return R, np.ascontiguousarray(np.linalg.pinv(R.astype(np.float64)), dtype=np.float32)


def _factor(what, factor):
    if isinstance(factor, bool) or not isinstance(factor, numbers.Integral) or not 1 <= factor <= MAX_FACTOR:
        raise _lib.EodError(f"{what}: `factor` is an integer in 1 .. {MAX_FACTOR}, got {factor!r}")
    return int(factor)


def _c_floats(a):
    return (ctypes.c_float * a.size)(*a.ravel().tolist())


def _shard(obs, n_total, lo, hi):
    """a copy of `obs` with every tensor whose leading dimension is n_total cut to [lo:hi]; leading dimension 1 is kept.  Host only."""
    what = f"{type(obs).__name__}.shard"
    for v in (n_total, lo, hi):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise _lib.EodError(f"{what}: n_total, lo and hi are integers, got {(n_total, lo, hi)!r}")
    if not 0 <= lo <= hi <= n_total or n_total < 1:
        raise _lib.EodError(f"{what}: needs 0 <= lo <= hi <= n_total and n_total >= 1, got n_total = {n_total}, [{lo}, {hi})")
    out = copy.copy(obs)
    for name in ("values", "mask"):
        t = getattr(obs, name)
        if t is None:
            continue
        if t.shape[0] not in (1, n_total):
            raise _lib.EodError(f"{what}: `{name}` has leading dimension {t.shape[0]}, not {n_total} or 1")
        if t.shape[0] == n_total:                      # (n_total == 1: [0:1] or the empty shard, like every other size)
            setattr(out, name, t[lo:hi])
    return out


class Observation:
    """values [B or 1, C, H, W] fp32: the observation on the full-resolution grid (a coarse one replicated over its blocks, i.e. A+ y);
    factors: C integers in 1 .. 8, the block edge per channel; mask None or [B or 1, C or 1, H, W] fp32, 1 = observed, 0 = free (soft values
    allowed); weight: a float in [0, 1], or one per UNet evaluation of the walk (checked against the walk before anything is launched).
    Everything that can be refused without knowing the call is refused here, the rest in bind()."""

    def __init__(self, values, factors, mask=None, weight=1.0):
        what = "Observation"
        self.factors = _factors(what, factors)
        C = len(self.factors)
        v = torch.as_tensor(values)
        if v.dtype != torch.float32:
            raise _lib.EodError(f"{what}: `values` must be float32, got {v.dtype}")
        if v.dim() != 4 or v.shape[1] != C:
            raise _lib.EodError(f"{what}: `values` must be [B or 1, {C}, H, W] ({C} factors were given), got {tuple(v.shape)}")
        H, W = int(v.shape[2]), int(v.shape[3])
        _divides(what, self.factors, H, W)
        if mask is not None:
            mask = torch.as_tensor(mask)
            if mask.dtype != torch.float32:
                raise _lib.EodError(f"{what}: `mask` must be float32, got {mask.dtype}")
            if mask.dim() != 4 or mask.shape[1] not in (1, C) or tuple(mask.shape[2:]) != (H, W):
                raise _lib.EodError(f"{what}: `mask` must be [B or 1, {C} or 1, {H}, {W}], got {tuple(mask.shape)}")
            if 1 not in (v.shape[0], mask.shape[0]) and v.shape[0] != mask.shape[0]:
                raise _lib.EodError(f"{what}: `values` is for {v.shape[0]} samples, `mask` for {mask.shape[0]}")
        self.weights, self.per_evaluation = _weights(what, weight)
        self.values, self.mask = v, mask

    def bind(self, what, shape, n_evaluations, device):
        """The observation for a call on a state of `shape` = (B, C, H, W) that evaluates the UNet n_evaluations times: every remaining
        refusal first, then values / mask contiguous on the device.  Returns a BoundObservation."""
        B, C, H, W = (int(s) for s in shape)
        if len(self.factors) != C:
            raise _lib.EodError(f"{what}: the observation has {len(self.factors)} channels, the state has {C}")
        if tuple(self.values.shape[2:]) != (H, W):
            raise _lib.EodError(f"{what}: the observation is {tuple(self.values.shape[2:])}, the state is {(H, W)}")
        for name, t in (("values", self.values), ("mask", self.mask)):
            if t is not None and t.shape[0] not in (1, B):
                raise _lib.EodError(f"{what}: the observation's `{name}` has leading dimension {t.shape[0]}; the call needs {B} or 1")
        if self.per_evaluation and len(self.weights) != n_evaluations:
            raise _lib.EodError(f"{what}: the call evaluates the UNet {n_evaluations} times, the observation's `weight` has {len(self.weights)} entries")
        if device is None:                             # (check(): the refusals alone, nothing copied)
            return None
        return BoundObservation(self, (B, C, H, W), n_evaluations, device)

    def shard(self, n_total, lo, hi):
        """the observation of samples [lo, hi) of a batch of n_total: tensors with leading dimension n_total cut, leading dimension 1 kept"""
        return _shard(self, n_total, lo, hi)


class BoundObservation:
    def __init__(self, obs, shape, n_evaluations, device):
        self.shape, self.factors = shape, obs.factors
        self.c_factors = _c_factors(obs.factors)
        self.values = f32c(obs.values.to(device))
        self.mask = None if obs.mask is None else f32c(obs.mask.to(device))
        self.weights = obs.weights if obs.per_evaluation else obs.weights * n_evaluations

    def _tail(self, x, i):
        """the arguments both _obs entry points share, from `values` to `W` and the broadcast flags"""
        if tuple(x.shape) != self.shape:
            raise _lib.EodError(f"observation bound to a state of shape {self.shape}, the step got {tuple(x.shape)}")
        B, C, H, W = self.shape
        m = self.mask
        return (self.values.data_ptr(), _lib.ptr(m), self.weights[i], self.c_factors, B, C, H, W, int(self.values.shape[0] != B),
                int(m is not None and m.shape[0] != B), int(m is not None and m.shape[1] != C))

    def ddim_step(self, i, x, e_t, noise, a_t, a_prev, sigma_t, sqrt_1m_at, temperature):
        """(x_prev, pred_x0) of evaluation number i: eod_ddim_step_obs"""
        x, e_t = f32c(x), f32c(e_t)
        x_prev, pred_x0 = torch.empty_like(x), torch.empty_like(x)
        _lib.check(_lib.lib().eod_ddim_step_obs(x.data_ptr(), e_t.data_ptr(), _lib.ptr(noise), float(a_t), float(a_prev), float(sigma_t),
                                                float(sqrt_1m_at), float(temperature), *self._tail(x, i), x_prev.data_ptr(),
                                                pred_x0.data_ptr(), current_stream_ptr(x.device)), "eod_ddim_step_obs")
        return x_prev, pred_x0

    def dpmpp_step(self, i, x, e_t, d_prev, a_s, sqrt_1m_as, c_x, c_d, w_cur, w_prev, clip):
        """(x_next, pred_x0) of evaluation number i: eod_dpmpp_step_obs"""
        x, e_t = f32c(x), f32c(e_t)
        x_next, pred_x0 = torch.empty_like(x), torch.empty_like(x)
        _lib.check(_lib.lib().eod_dpmpp_step_obs(x.data_ptr(), e_t.data_ptr(), _lib.ptr(d_prev), float(a_s), float(sqrt_1m_as), float(c_x),
                                                 float(c_d), float(w_cur), float(w_prev), int(bool(clip)), *self._tail(x, i),
                                                 x_next.data_ptr(), pred_x0.data_ptr(), current_stream_ptr(x.device)), "eod_dpmpp_step_obs")
        return x_next, pred_x0


    def project(self, i, p):
        """the projection of a given prediction p at evaluation number i (a link of a chain): eod_obs_project"""
        out = torch.empty_like(p)
        _lib.check(_lib.lib().eod_obs_project(p.data_ptr(), *self._tail(p, i), out.data_ptr(), current_stream_ptr(p.device)), "eod_obs_project")
        return out


class SpectralObservation:
    """K observed bands that are known linear mixes of the state's C channels, on a grid `factor` times coarser.  values [B or 1, K, H, W]
    fp32: what the other sensor saw, replicated onto the full-resolution grid; response: array-like [K, C], K <= min(C, 8), C <= 32, finite,
    of full row rank with sigma_min >= 1e-3 sigma_max (float64 SVD of the fp32 entries the kernels use); factor: the block edge, 1 .. 8;
    mask None or [B or 1, 1, H, W] fp32 (ONE mask for all K bands: per-band masks change the pseudo-inverse); weight as for Observation.
    `pinv` [C, K] is the float64 pseudo-inverse rounded once to fp32."""

    def __init__(self, values, response, factor=1, mask=None, weight=1.0):
        what = "SpectralObservation"
        self.response, self.pinv = _conditioned(what, response)
        K, C = self.response.shape
        self.factor = _factor(what, factor)
        v = torch.as_tensor(values)
        if v.dtype != torch.float32:
            raise _lib.EodError(f"{what}: `values` must be float32, got {v.dtype}")
        if v.dim() != 4 or v.shape[1] != K:
            raise _lib.EodError(f"{what}: `values` must be [B or 1, {K}, H, W] (`response` has {K} rows), got {tuple(v.shape)}")
        H, W = int(v.shape[2]), int(v.shape[3])
        if H % self.factor or W % self.factor:
            raise _lib.EodError(f"{what}: factor = {self.factor} does not divide {H} x {W}")
        if mask is not None:
            mask = torch.as_tensor(mask)
            if mask.dtype != torch.float32:
                raise _lib.EodError(f"{what}: `mask` must be float32, got {mask.dtype}")
            if mask.dim() != 4 or mask.shape[1] != 1 or tuple(mask.shape[2:]) != (H, W):
                raise _lib.EodError(f"{what}: `mask` must be [B or 1, 1, {H}, {W}] (one mask for all {K} bands), got {tuple(mask.shape)}")
            if 1 not in (v.shape[0], mask.shape[0]) and v.shape[0] != mask.shape[0]:
                raise _lib.EodError(f"{what}: `values` is for {v.shape[0]} samples, `mask` for {mask.shape[0]}")
        self.weights, self.per_evaluation = _weights(what, weight)
        self.values, self.mask = v, mask

    def bind(self, what, shape, n_evaluations, device):
        B, C, H, W = (int(s) for s in shape)
        if self.response.shape[1] != C:
            raise _lib.EodError(f"{what}: the observation's `response` mixes {self.response.shape[1]} channels, the state has {C}")
        if tuple(self.values.shape[2:]) != (H, W):
            raise _lib.EodError(f"{what}: the observation is {tuple(self.values.shape[2:])}, the state is {(H, W)}")
        for name, t in (("values", self.values), ("mask", self.mask)):
            if t is not None and t.shape[0] not in (1, B):
                raise _lib.EodError(f"{what}: the observation's `{name}` has leading dimension {t.shape[0]}; the call needs {B} or 1")
        if self.per_evaluation and len(self.weights) != n_evaluations:
            raise _lib.EodError(f"{what}: the call evaluates the UNet {n_evaluations} times, the observation's `weight` has {len(self.weights)} entries")
        if device is None:                             # (check(): the refusals alone, nothing copied)
            return None
        return BoundSpectral(self, (B, C, H, W), n_evaluations, device)

    def shard(self, n_total, lo, hi):
        """the observation of samples [lo, hi) of a batch of n_total: tensors with leading dimension n_total cut, leading dimension 1 kept"""
        return _shard(self, n_total, lo, hi)


class BoundSpectral:
    def __init__(self, obs, shape, n_evaluations, device):
        self.shape, self.factor, self.K = shape, obs.factor, obs.response.shape[0]
        self.c_R, self.c_G = _c_floats(obs.response), _c_floats(obs.pinv)
        self.values = f32c(obs.values.to(device))
        self.mask = None if obs.mask is None else f32c(obs.mask.to(device))
        self.weights = obs.weights if obs.per_evaluation else obs.weights * n_evaluations

    def _tail(self, x, i):
        """the arguments the three entry points share, from `values` to the broadcast flags"""
        if tuple(x.shape) != self.shape:
            raise _lib.EodError(f"observation bound to a state of shape {self.shape}, the step got {tuple(x.shape)}")
        B, C, H, W = self.shape
        m = self.mask
        return (self.values.data_ptr(), _lib.ptr(m), self.weights[i], self.c_R, self.c_G, self.K, self.factor, B, C, H, W,
                int(self.values.shape[0] != B), int(m is not None and m.shape[0] != B))

    def ddim_step(self, i, x, e_t, noise, a_t, a_prev, sigma_t, sqrt_1m_at, temperature):
        """(x_prev, pred_x0) of evaluation number i: eod_ddim_step_spec"""
        x, e_t = f32c(x), f32c(e_t)
        x_prev, pred_x0 = torch.empty_like(x), torch.empty_like(x)
        _lib.check(_lib.lib().eod_ddim_step_spec(x.data_ptr(), e_t.data_ptr(), _lib.ptr(noise), float(a_t), float(a_prev), float(sigma_t),
                                                 float(sqrt_1m_at), float(temperature), *self._tail(x, i), x_prev.data_ptr(),
                                                 pred_x0.data_ptr(), current_stream_ptr(x.device)), "eod_ddim_step_spec")
        return x_prev, pred_x0

    def dpmpp_step(self, i, x, e_t, d_prev, a_s, sqrt_1m_as, c_x, c_d, w_cur, w_prev, clip):
        """(x_next, pred_x0) of evaluation number i: eod_dpmpp_step_spec"""
        x, e_t = f32c(x), f32c(e_t)
        x_next, pred_x0 = torch.empty_like(x), torch.empty_like(x)
        _lib.check(_lib.lib().eod_dpmpp_step_spec(x.data_ptr(), e_t.data_ptr(), _lib.ptr(d_prev), float(a_s), float(sqrt_1m_as), float(c_x),
                                                  float(c_d), float(w_cur), float(w_prev), int(bool(clip)), *self._tail(x, i),
                                                  x_next.data_ptr(), pred_x0.data_ptr(), current_stream_ptr(x.device)), "eod_dpmpp_step_spec")
        return x_next, pred_x0

    def project(self, i, p):
        """the projection of a given prediction p at evaluation number i (a link of a chain): eod_spec_project"""
        out = torch.empty_like(p)
        _lib.check(_lib.lib().eod_spec_project(p.data_ptr(), *self._tail(p, i), out.data_ptr(), current_stream_ptr(p.device)), "eod_spec_project")
        return out


def _taps(what, psf, symmetric=True):
    """the 1-D taps h[0 .. 2r] as the fp32 array the kernels use: finite, non-negative, bitwise symmetric (unless symmetric=False: one
    axis of a SeparablePsf), centre tap positive"""
    try:
        h = np.asarray(psf.detach().cpu().numpy() if torch.is_tensor(psf) else psf)
    except Exception:
        raise _lib.EodError(f"{what}: `psf` is array-like, the 1-D taps h[0 .. 2r], got {type(psf).__name__}") from None
    if h.dtype == np.bool_ or not (np.issubdtype(h.dtype, np.floating) or np.issubdtype(h.dtype, np.integer)):
        raise _lib.EodError(f"{what}: `psf` must hold real numbers, got dtype {h.dtype}")
    if h.ndim != 1 or h.size % 2 != 1 or h.size > 2 * MAX_RADIUS + 1:
        raise _lib.EodError(f"{what}: `psf` is the 1-D taps h[0 .. 2r] of a separable PSF, r = 0 .. {MAX_RADIUS} (an odd number of them, "
                            f"at most {2 * MAX_RADIUS + 1}), got shape {h.shape}")
    with np.errstate(over="ignore"):
        h = np.ascontiguousarray(h, dtype=np.float32)
    if not np.isfinite(h).all() or np.signbit(h).any():
        raise _lib.EodError(f"{what}: the taps of `psf` must be finite and non-negative (as float32)")
    if symmetric and not _bit_symmetric(h):
        raise _lib.EodError(f"{what}: the taps of `psf` must be symmetric bit for bit (as float32): A^T is computed with the same stencil")
    if not h[h.size // 2] > 0.0:
        raise _lib.EodError(f"{what}: the centre tap of `psf` must be positive")
    return h


def _bit_symmetric(h):
    return h.view(np.uint32).tolist() == h[::-1].view(np.uint32).tolist()


class SeparablePsf:
    """A separable PSF with one tap vector per axis: `x` along a row, `y` along a column (None: the same taps on
    both axes).  Each is array-like [2r + 1], r = 0 .. 12 (the two radii independent), finite, non-negative, centre tap positive, and NOT
    necessarily symmetric: h[t] weights the scene pixel at offset t - r, so mass at t > r means "this sample sees the scene to its right /
    below" (a band registered a fraction of a pixel off the grid; gaussian_psf(shift=...)).  taps_x / taps_y: float32 arrays.  Taken
    wherever a `psf` is: PsfObservation(values, SeparablePsf(...), factor, ...) and psf_observe(x, SeparablePsf(...), factor, ...), which
    then run the eod_psf_*_xy kernels.  A bare array keeps the symmetric rules and kernels."""

    def __init__(self, x, y=None):
        what = "SeparablePsf"
        if isinstance(x, SeparablePsf) or isinstance(y, SeparablePsf):
            raise _lib.EodError(f"{what}: `x` and `y` are 1-D tap vectors, got a SeparablePsf")
        self.taps_x = _taps(f"{what}: x", x, symmetric=False)
        self.taps_y = self.taps_x if y is None else _taps(f"{what}: y", y, symmetric=False)

    @property
    def radii(self):
        """(ry, rx)"""
        return self.taps_y.size // 2, self.taps_x.size // 2

    def __repr__(self):
        return f"SeparablePsf(x={self.taps_x.tolist()}, y={self.taps_y.tolist()})"


def _channels(what, channels):
    try:
        cs = list(channels)
    except TypeError:
        raise _lib.EodError(f"{what}: `channels` is None (all) or a sequence of channel numbers, got {channels!r}") from None
    if not 1 <= len(cs) <= MAX_CHANNELS:
        raise _lib.EodError(f"{what}: `channels` lists 1 .. {MAX_CHANNELS} channels, got {len(cs)}")
    for c in cs:
        if isinstance(c, bool) or not isinstance(c, numbers.Integral) or not 0 <= c < MAX_CHANNELS:
            raise _lib.EodError(f"{what}: a channel is an integer in 0 .. {MAX_CHANNELS - 1}, got {c!r}")
    if any(b <= a for a, b in zip(cs, cs[1:])):
        raise _lib.EodError(f"{what}: `channels` must be strictly increasing, got {cs}")
    return tuple(int(c) for c in cs)


def _c_ints(a):
    return (ctypes.c_int32 * len(a))(*a)


def psf_cmax(taps, L):
    """max_j sum_i h[i - j + r] / n_i over a line of length L, n = B0 1 (float64 of the fp32 taps): the largest column sum of the
    renormalised 1-D blur N^-1 B0"""
    h = np.asarray(taps, np.float32).astype(np.float64)
    r, idx = h.size // 2, np.arange(int(L))
    n, col = np.zeros(int(L)), np.zeros(int(L))
    for t in range(h.size):
        ok = (idx + t - r >= 0) & (idx + t - r < L)
        n[ok] += h[t]
    for t in range(h.size):
        ok = (idx + t - r >= 0) & (idx + t - r < L)          # row i, column i + t - r holds h[t]
        col[idx[ok] + t - r] += h[t] / n[ok]
    return float(col.max())


def psf_tau(taps, factor, H, W):
    """the Landweber step size f^2 / (cmax(H) cmax(W)) <= 1 / ||A||^2 (||A||^2 <= ||A||_1 ||A||_inf = cmax(H) cmax(W) / f^2), float64.
    taps: one vector for both axes, or a SeparablePsf: f^2 / (cmax(taps_y, H) cmax(taps_x, W))"""
    ty, tx = (taps.taps_y, taps.taps_x) if isinstance(taps, SeparablePsf) else (taps, taps)
    return float(factor * factor) / (psf_cmax(ty, H) * psf_cmax(tx, W))


def psf_gram(taps, factor, L, symmetric=True):
    """(bands, b): the 1-D Gram matrix G_L = A1(L) A1(L)^T of the operator A1 = D_f N^-1 B0 on a line of length L (renormalised zero padding,
    block mean) as its band: bands float32 [L / f, 2b + 1], bands[i][j] = G_L[i][i - b + j], zero where the column lies outside the line;
    b = ceil(2r / f).  float64 of the fp32 taps, band by band (no dense matrix: L may be a scene's width); the upper band is computed and
    mirrored, so G_L is symmetric bit for bit.  A A^T = G(H) (x) G(W).  symmetric=False: one axis of a SeparablePsf, the taps need not be
    symmetric (G_L still is: it is a Gram matrix); n is then summed tap by tap in the orientation of the contract."""
    what = "psf_gram"
    h = _taps(what, taps, symmetric=bool(symmetric)).astype(np.float64)
    f = _factor(what, factor)
    if isinstance(L, bool) or not isinstance(L, numbers.Integral) or L < 1 or L % f:
        raise _lib.EodError(f"{what}: L is a positive multiple of factor = {f}, got {L!r}")
    L = int(L)
    r, Lc = h.size // 2, L // f
    b = -((-2 * r) // f)
    if symmetric:
        n = np.convolve(np.ones(L), h)[r:r + L]              # N = diag(B0 1) (np.convolve flips the taps: symmetric ones only)
    else:
        n, idx = np.zeros(L), np.arange(L)
        for t in range(h.size):                              # n[y] = sum_t h[t] [0 <= y - r + t < L]
            n[(idx - r + t >= 0) & (idx - r + t < L)] += h[t]
    w = f + 2 * r                                            # row i of A1 lives on x = i f - r .. i f + f - 1 + r
    rows = np.zeros((Lc, w))
    for a in range(f):                                       # the block's pixel y = i f + a sees x = y - r + t through h[t] / n[y]
        inv = 1.0 / n[a::f]
        for t in range(h.size):
            rows[:, a + t] += h[t] * inv
    x = np.arange(Lc)[:, None] * f - r + np.arange(w)[None, :]
    rows[(x < 0) | (x >= L)] = 0.0
    rows /= f
    bands = np.zeros((Lc, 2 * b + 1))
    for k in range(min(b, Lc - 1) + 1):                      # G[i][i + k]: the two rows overlap on w - k f columns
        g = (rows[:Lc - k, k * f:] * rows[k:, :w - k * f]).sum(axis=1)
        bands[np.arange(Lc - k), b + k] = g
        bands[np.arange(k, Lc), b - k] = g
    return bands.astype(np.float32), b


def psf_gram_pair(psf, factor, H, W):
    """(gy, gx, b): the Gram tables of a SeparablePsf's two axes, psf_gram(taps_y, factor, H) and psf_gram(taps_x, factor, W), as eod_psf_cg
    takes them: ONE half-width b = max(ceil(2 ry / f), ceil(2 rx / f)), the narrower table padded with zero columns on both sides (those
    entries of G are zero: the rows do not overlap).  An axis with bitwise symmetric taps takes psf_gram's symmetric form, so with equal
    symmetric taps nothing is padded and the tables have the bits of the bare-taps link."""
    gy, by = psf_gram(psf.taps_y, factor, H, symmetric=_bit_symmetric(psf.taps_y))
    gx, bx = psf_gram(psf.taps_x, factor, W, symmetric=_bit_symmetric(psf.taps_x))
    b = max(by, bx)
    pad = lambda g, bb: np.ascontiguousarray(np.pad(g, ((0, 0), (b - bb, b - bb))))
    return pad(gy, by), pad(gx, bx), b


def _dampings(what, damping):
    """([fp32-rounded dampings], one per evaluation?) of a `damping` argument: a finite float >= 0 or a sequence of them"""
    if isinstance(damping, (numbers.Real, np.floating)) and not isinstance(damping, bool):
        ds, per_evaluation = [damping], False
    else:
        try:
            ds = list(damping)
        except TypeError:
            raise _lib.EodError(f"{what}: `damping` is a float or a sequence of floats, got {damping!r}") from None
        per_evaluation = True
    for d in ds:
        if isinstance(d, bool) or not isinstance(d, (numbers.Real, np.floating)) or not math.isfinite(float(d)):
            raise _lib.EodError(f"{what}: a damping is a finite float, got {d!r}")
        if not 0.0 <= float(d) or not math.isfinite(float(np.float32(d))):
            raise _lib.EodError(f"{what}: a damping is >= 0 (and finite as float32), got {d!r}")
    return [float(np.float32(d)) for d in ds], per_evaluation


def gaussian_sigma(factor, mtf_nyquist=0.3):
    """sigma in fine pixels of the Gaussian whose MTF exp(-2 pi^2 sigma^2 nu^2) is mtf_nyquist at the coarse grid's Nyquist frequency 1 / (2 f)"""
    what = "gaussian_psf"
    f = _factor(what, factor)
    if isinstance(mtf_nyquist, bool) or not isinstance(mtf_nyquist, (numbers.Real, np.floating)) or not 0.0 < float(mtf_nyquist) <= 1.0:
        raise _lib.EodError(f"{what}: `mtf_nyquist` is a float in (0, 1], got {mtf_nyquist!r}")
    return f * math.sqrt(-2.0 * math.log(float(mtf_nyquist))) / math.pi


def gaussian_psf(factor, mtf_nyquist=0.3, radius=None, shift=0.0):
    """The taps of a Gaussian PSF for a sensor `factor` times coarser whose MTF at its Nyquist frequency is mtf_nyquist: sigma =
    f sqrt(-2 ln mtf) / pi, taps on -r .. r with r = min(ceil(3 sigma), 12) (or `radius`), normalised in float64, rounded to fp32,
    symmetric bit for bit.  float32 [2r + 1].  shift (|shift| <= 0.5 factor, in fine pixels): the Gaussian is centred at `shift`, tap t
    weighing the scene pixel at offset t - r (shift > 0: the sample sees the scene to its right / below); r = min(ceil(3 sigma + |shift|),
    12), normalised in float64, rounded to fp32 and NOT symmetrised: one axis of a SeparablePsf; refused when mtf_nyquist is so close to 1 that every tap underflows to 0.  shift = 0.0: the bits above."""
    what = "gaussian_psf"
    sigma = gaussian_sigma(factor, mtf_nyquist)
    if isinstance(shift, bool) or not isinstance(shift, (numbers.Real, np.floating)) or not math.isfinite(float(shift)):
        raise _lib.EodError(f"{what}: `shift` is a finite float (fine pixels), got {shift!r}")
    shift = float(shift)
    if abs(shift) > 0.5 * factor:
        raise _lib.EodError(f"{what}: `shift` is at most half a coarse pixel, |shift| <= {0.5 * factor}, got {shift!r}")
    if shift != 0.0 and not sigma > 0.0:
        raise _lib.EodError(f"{what}: mtf_nyquist = 1 is a point: it has no taps at a sub-pixel `shift`")
    if radius is None:
        r = min(int(math.ceil(3.0 * sigma + abs(shift))), MAX_RADIUS)
    else:
        if isinstance(radius, bool) or not isinstance(radius, numbers.Integral) or not 0 <= radius <= MAX_RADIUS:
            raise _lib.EodError(f"{what}: `radius` is an integer in 0 .. {MAX_RADIUS}, got {radius!r}")
        r = int(radius)
    k = np.arange(-r, r + 1, dtype=np.float64)
    if shift != 0.0:
        with np.errstate(under="ignore"):
            g = np.exp(-((k - shift) * (k - shift)) / (2.0 * sigma * sigma))
        total = float(g.sum())
        if not (total > 0.0 and math.isfinite(total)):                  # sigma so small that every tap underflows: nothing to normalise
            raise _lib.EodError(f"{what}: mtf_nyquist = {mtf_nyquist!r} is too close to a point: every tap at shift = {shift!r} underflows to 0")
        return (g / total).astype(np.float32)
    g = np.exp(-(k * k) / (2.0 * sigma * sigma)) if sigma > 0.0 else (k == 0).astype(np.float64)
    h = (g / g.sum()).astype(np.float32)
    h[r + 1:] = h[:r][::-1]
    return h


class PsfObservation:
    """K channels seen through a sensor's PSF on a grid `factor` times coarser: A = D_f N^-1 B0 per observed channel (B0 the zero-padded
    separable convolution with the 1-D taps `psf`, horizontally then vertically; N = diag(B0 1); D_f the factor x factor block mean).
    values [B or 1, K, H / f, W / f] fp32 on the COARSE grid: what the sensor delivered; psf: array-like [2r + 1], r = 0 .. 12, finite,
    non-negative, symmetric bit for bit as float32, centre tap positive, or a SeparablePsf (one tap vector per axis, asymmetric ones
    allowed: an anisotropic or shifted PSF; the eod_psf_*_xy kernels); factor 1 .. 8; channels None (all C, C = K) or K strictly
    increasing channel numbers; mask None or [B or 1, K or 1, H / f, W / f] fp32; weight as for Observation.  solver "landweber" (the
    default): iters 1 .. 8 Landweber steps per evaluation, which approach the constraint set.  solver "cg": iters 1 .. 64 conjugate-gradient
    iterations of the exact projection per evaluation, p - weight * A^T (M A A^T M + damping I)^-1 mask (A p - values); the mask must then
    be 0 or 1 exactly, and damping (a float >= 0, or one per evaluation) is the Tikhonov term for noisy values.

    response: None, or array-like [K, C] under SpectralObservation's rules (K <= min(C, 8), C <= 32, finite, sigma_min >= 1e-3 sigma_max):
    the K observed bands are the mixes sum_c response[k][c] * channel c seen through the ONE operator above, A = R (x) A_s (a panchromatic
    band with its own MTF; another sensor's broad bands on its grid).  Not together with `channels`; values then has K planes and the mask
    is [B or 1, 1, H / f, W / f], one for all bands.  `pinv` [C, K] is the float64 pseudo-inverse rounded once to fp32.  solver "cg":
    M A A^T M = (R R^T) (x) (M_s G M_s), so the projection is p - weight * (pinv(R) (x) A_s^T (M_s G M_s + damping I)^-1) mask (A p - values),
    K independent plane solves.  The damped system is therefore (R R^T) (x) (M_s G M_s + damping I): the Tikhonov term is scaled by each
    band's response energy -- for orthonormal rows it is the unmixed form, for one band it is damping * |r|^2.  solver "landweber": the
    step size is psf_tau / sigma_max(R)^2 (float64 SVD of the fp32 entries), soft masks allowed as before."""

    def __init__(self, values, psf, factor, channels=None, mask=None, weight=1.0, iters=1, solver="landweber", damping=0.0, response=None):
        what = "PsfObservation"
        self.psf = psf if isinstance(psf, SeparablePsf) else None       # one tap vector per axis: `taps` is then None
        self.taps = None if self.psf is not None else _taps(what, psf)
        self.factor = _factor(what, factor)
        self.channels = None if channels is None else _channels(what, channels)
        self.response = self.pinv = None
        if response is not None:
            if channels is not None:
                raise _lib.EodError(f"{what}: `response` mixes all channels of the state; it cannot be given together with `channels`")
            self.response, self.pinv = _conditioned(what, response)
        if not isinstance(solver, str) or solver not in SOLVERS:
            raise _lib.EodError(f"{what}: `solver` is one of {SOLVERS}, got {solver!r}")
        self.solver = solver
        most = MAX_CG_ITERS if solver == "cg" else MAX_ITERS
        if isinstance(iters, bool) or not isinstance(iters, numbers.Integral) or not 1 <= iters <= most:
            raise _lib.EodError(f"{what}: `iters` is an integer in 1 .. {most} with solver={solver!r}, got {iters!r}")
        self.iters = int(iters)
        self.dampings, self.damping_per_evaluation = _dampings(what, damping)
        if solver != "cg" and any(d != 0.0 for d in self.dampings):
            raise _lib.EodError(f"{what}: `damping` belongs to solver=\"cg\" (the Landweber steps have no regularised form), got {damping!r}")
        v = torch.as_tensor(values)
        if v.dtype != torch.float32:
            raise _lib.EodError(f"{what}: `values` must be float32, got {v.dtype}")
        if self.response is not None and (v.dim() != 4 or 0 in v.shape or v.shape[1] != self.response.shape[0]):
            raise _lib.EodError(f"{what}: `values` must be [B or 1, {self.response.shape[0]}, H / f, W / f] (`response` has "
                                f"{self.response.shape[0]} rows), got {tuple(v.shape)}")
        if v.dim() != 4 or 0 in v.shape or v.shape[1] > MAX_CHANNELS or (self.channels is not None and v.shape[1] != len(self.channels)):
            want = "K <= 32" if self.channels is None else str(len(self.channels))
            raise _lib.EodError(f"{what}: `values` must be [B or 1, {want}, H / f, W / f] on the coarse grid, got {tuple(v.shape)}")
        K, Hc, Wc = (int(d) for d in v.shape[1:])
        if mask is not None:
            mask = torch.as_tensor(mask)
            if mask.dtype != torch.float32:
                raise _lib.EodError(f"{what}: `mask` must be float32, got {mask.dtype}")
            if mask.dim() != 4 or mask.shape[1] not in (1, K) or tuple(mask.shape[2:]) != (Hc, Wc):
                raise _lib.EodError(f"{what}: `mask` must be [B or 1, {K} or 1, {Hc}, {Wc}] on the coarse grid, got {tuple(mask.shape)}")
            if self.response is not None and mask.shape[1] != 1:
                raise _lib.EodError(f"{what}: with `response` the `mask` must be [B or 1, 1, {Hc}, {Wc}] (one mask for all {K} bands: per-band "
                                    f"masks break the factorisation of A A^T), got {tuple(mask.shape)}")
            if 1 not in (v.shape[0], mask.shape[0]) and v.shape[0] != mask.shape[0]:
                raise _lib.EodError(f"{what}: `values` is for {v.shape[0]} samples, `mask` for {mask.shape[0]}")
            if solver == "cg" and not bool(((mask == 0.0) | (mask == 1.0)).all()):
                raise _lib.EodError(f"{what}: with solver=\"cg\" the `mask` must be 0 or 1 exactly (a soft mask inside M A A^T M destroys the "
                                    f"system's conditioning); express soft knowledge with `weight` and `damping`")
        self.weights, self.per_evaluation = _weights(what, weight)
        self.values, self.mask = v, mask

    def bind(self, what, shape, n_evaluations, device):
        B, C, H, W = (int(s) for s in shape)
        K, f = int(self.values.shape[1]), self.factor
        if C > MAX_CHANNELS:
            raise _lib.EodError(f"{what}: a PsfObservation takes a state of at most {MAX_CHANNELS} channels, got {C}")
        if self.response is not None:
            if self.response.shape[1] != C:
                raise _lib.EodError(f"{what}: the PsfObservation's `response` mixes {self.response.shape[1]} channels, the state has {C}")
            channels = None
        elif self.channels is None:
            if K != C:
                raise _lib.EodError(f"{what}: the PsfObservation observes all channels (`channels` is None) and has {K}, the state has {C}")
            channels = tuple(range(C))
        else:
            channels = self.channels
            if channels[-1] >= C:
                raise _lib.EodError(f"{what}: the PsfObservation observes channel {channels[-1]}, the state has {C}")
        if H % f or W % f or tuple(self.values.shape[2:]) != (H // f, W // f):
            raise _lib.EodError(f"{what}: the PsfObservation is {tuple(self.values.shape[2:])} at factor {f}, the state is {(H, W)}")
        for name, t in (("values", self.values), ("mask", self.mask)):
            if t is not None and t.shape[0] not in (1, B):
                raise _lib.EodError(f"{what}: the observation's `{name}` has leading dimension {t.shape[0]}; the call needs {B} or 1")
        if self.per_evaluation and len(self.weights) != n_evaluations:
            raise _lib.EodError(f"{what}: the call evaluates the UNet {n_evaluations} times, the observation's `weight` has {len(self.weights)} entries")
        if self.damping_per_evaluation and len(self.dampings) != n_evaluations:
            raise _lib.EodError(f"{what}: the call evaluates the UNet {n_evaluations} times, the observation's `damping` has {len(self.dampings)} entries")
        if device is None:                             # (check(): the refusals alone, nothing copied)
            return None
        return BoundPsf(self, (B, C, H, W), channels, n_evaluations, device)

    def shard(self, n_total, lo, hi):
        """the observation of samples [lo, hi) of a batch of n_total: tensors with leading dimension n_total cut, leading dimension 1 kept"""
        return _shard(self, n_total, lo, hi)


class BoundPsf:
    def __init__(self, obs, shape, channels, n_evaluations, device):
        B, C, H, W = shape
        self.shape, self.factor, self.iters, self.channels = shape, obs.factor, obs.iters, channels
        self.xy = obs.psf is not None                  # a SeparablePsf: the _xy entry points
        if self.xy:
            self.ry, self.rx = obs.psf.radii
            self.r = max(self.ry, self.rx)
            self.c_taps_y, self.c_taps_x = _c_floats(obs.psf.taps_y), _c_floats(obs.psf.taps_x)
        else:
            self.r = obs.taps.size // 2
            self.c_taps = _c_floats(obs.taps)
        self.tau = psf_tau(obs.psf if self.xy else obs.taps, obs.factor, H, W)
        self.mixed = obs.response is not None
        if self.mixed:                                 # A = R (x) A_s: ||A|| = sigma_max(R) ||A_s||; the Landweber adjoint mixes by R^T, cg by pinv(R)
            self.K = obs.response.shape[0]
            self.tau /= float(np.linalg.svd(obs.response.astype(np.float64), compute_uv=False)[0]) ** 2
            self.c_R = _c_floats(obs.response)
            self.c_G = _c_floats(obs.pinv if obs.solver == "cg" else np.ascontiguousarray(obs.response.T))
        else:
            self.K, self.c_channels = len(channels), _c_ints(channels)
        # the entry points (include/eodiff.h) and what each takes between the weight (the step) and K: taps, factor, channel list / matrix
        f = obs.factor
        if self.xy:                                    # eod_psf_{residual,update}_xy: both tap vectors, the channel list AND the matrix, one NULL
            cs, R, G = (None, self.c_R, self.c_G) if self.mixed else (self.c_channels, None, None)
            self.suffix, self.takes_mask_c1 = "_xy", True
            self.residual_args = (self.c_taps_y, self.ry, self.c_taps_x, self.rx, f, cs, R)
            self.update_args = (self.c_taps_y, self.ry, self.c_taps_x, self.rx, f, cs, G)
        elif self.mixed:                               # eod_psf_{residual,update}_mix: the matrix; one mask plane always, no mask_c1 argument
            self.suffix, self.takes_mask_c1 = "_mix", False
            self.residual_args = (self.c_taps, self.r, f, self.c_R)
            self.update_args = (self.c_taps, self.r, f, self.c_G)
        else:                                          # eod_psf_{residual,update}: the channel list
            self.suffix, self.takes_mask_c1 = "", True
            self.residual_args = self.update_args = (self.c_taps, self.r, f, self.c_channels)
        self.step = float(np.float32(self.tau / (obs.factor * obs.factor)))
        self.values = f32c(obs.values.to(device))
        self.mask = None if obs.mask is None else f32c(obs.mask.to(device))
        self.weights = obs.weights if obs.per_evaluation else obs.weights * n_evaluations
        self.solver = obs.solver
        if self.solver == "cg":                        # the two Gram tables beside `values`; workspace and coarse buffers at the first project
            self.dampings = obs.dampings if obs.damping_per_evaluation else obs.dampings * n_evaluations
            self.unit_step = float(np.float32(1.0 / (obs.factor * obs.factor)))
            if self.xy:
                gy, gx, self.band = psf_gram_pair(obs.psf, obs.factor, H, W)
            else:
                gy, self.band = psf_gram(obs.taps, obs.factor, H)
                gx, _ = psf_gram(obs.taps, obs.factor, W)
            self.gy, self.gx = torch.from_numpy(gy).to(device), torch.from_numpy(gx).to(device)
            self._cg = self._coarse = None

    def residual(self, i, p, q, weight=None):
        """q = weight_i * mask * (A p - values) on the coarse grid: eod_psf_residual"""
        if tuple(p.shape) != self.shape:
            raise _lib.EodError(f"observation bound to a state of shape {self.shape}, the step got {tuple(p.shape)}")
        B, C, H, W = self.shape
        m = self.mask
        name = "eod_psf_residual" + self.suffix
        mask_c1 = (int(self.mixed or (m is not None and m.shape[1] != self.K)),) if self.takes_mask_c1 else ()
        _lib.check(getattr(_lib.lib(), name)(p.data_ptr(), self.values.data_ptr(), _lib.ptr(m), self.weights[i] if weight is None else weight,
                                             *self.residual_args, self.K, B, C, H, W, int(self.values.shape[0] != B),
                                             int(m is not None and m.shape[0] != B), *mask_c1, q.data_ptr(), current_stream_ptr(p.device)), name)
        return q

    def update(self, p, q, out, step=None):
        """out = p - tau A^T q: eod_psf_update (with a response: eod_psf_update_mix, the coarse planes mixed by R^T or, under cg, pinv(R))"""
        B, C, H, W = self.shape
        name = "eod_psf_update" + self.suffix
        _lib.check(getattr(_lib.lib(), name)(p.data_ptr(), q.data_ptr(), self.step if step is None else step, *self.update_args, self.K, B, C, H, W,
                                             out.data_ptr(), current_stream_ptr(p.device)), name)
        return out

    def project(self, i, p):
        """`iters` Landweber steps from the prediction p at evaluation number i (a link of a chain): iters x (residual, update), ping-pong
        between two buffers (eod_psf_update's out must not be its p)"""
        if self.solver == "cg":
            return self.project_cg(i, p)
        B, C, H, W = self.shape
        p = f32c(p)
        q = torch.empty((B, self.K, H // self.factor, W // self.factor), device=p.device, dtype=torch.float32)
        bufs = [torch.empty_like(p) for _ in range(min(self.iters, 2))]
        for it in range(self.iters):
            p = self.update(p, self.residual(i, p, q), bufs[it % 2])
        return p


    def solve(self, i, c, q):
        """q = weight_i * mask * z, (M A A^T M + damping_i I) z = c by `iters` conjugate-gradient iterations on the coarse grid: eod_psf_cg.
        The workspace belongs to the link: allocated at the first call, reused by every later one."""
        B, C, H, W = self.shape
        Hc, Wc = H // self.factor, W // self.factor
        L = _lib.lib()
        if self._cg is None or self._cg.device != c.device:
            self._cg = torch.empty(int(L.eod_psf_cg_workspace_size(B, self.K, Hc, Wc)), device=c.device, dtype=torch.uint8)
        m = self.mask
        _lib.check(L.eod_psf_cg(c.data_ptr(), _lib.ptr(m), self.dampings[i], self.weights[i], self.gy.data_ptr(), self.gx.data_ptr(), self.band,
                                self.iters, B, self.K, Hc, Wc, int(m is not None and m.shape[0] != B),
                                int(m is not None and (self.mixed or m.shape[1] != self.K)), q.data_ptr(), self._cg.data_ptr(), self._cg.numel(),
                                current_stream_ptr(c.device)), "eod_psf_cg")
        return q

    def project_cg(self, i, p):
        """the exact projection of the prediction p at evaluation number i: eod_psf_residual (weight 1) -> eod_psf_cg -> eod_psf_update
        (step 1 / f^2).  The two coarse buffers belong to the link; the result is a fresh tensor (a sampler keeps it as its history)."""
        B, C, H, W = self.shape
        p = f32c(p)
        if self._coarse is None or self._coarse[0].device != p.device:
            self._coarse = [torch.empty((B, self.K, H // self.factor, W // self.factor), device=p.device, dtype=torch.float32) for _ in range(2)]
        c, q = self._coarse
        self.solve(i, self.residual(i, p, c, 1.0), q)
        return self.update(p, q, torch.empty_like(p), self.unit_step)


class BoundChain:
    """1 .. 4 bound observations (one: a PsfObservation, which has no fused kernel) applied in order to every evaluation's prediction, each link to the previous link's result and with its own
    weight: eod_pred_x0, one projection launch per link, eod_ddim_step_p0 / eod_dpmpp_step_p0.  The bits are those the fused kernel of
    every link would give on the same prediction.  pred_x0 (for DPM-Solver++: the next evaluation's history) is the last link's result.
    threshold: a diffusion/threshold.py BoundThreshold, or None.  It becomes link 0, in front of the observations (it does not count towards
    MAX_LINKS, and `links` may then be empty), and it REPLACES the static clamp: the prediction is formed with clip = 0 whatever the
    sampler asks for.
    parameterization: what the `e_t` handed to the steps is -- "eps": the noise estimate; "x0" / "v": the model's raw output, from which
    eod_param_pred (ancestral: eod_ddpm_param_pred) forms the prediction directly, and for DDIM the noise estimate its update needs.
    Every call of such a model runs a chain, with no links when it has neither an observation nor a threshold."""

    def __init__(self, links, threshold=None, parameterization="eps"):
        self.threshold = threshold
        self.links = list(links) if threshold is None else [threshold] + list(links)
        self.kind = parameterization_kind("BoundChain", parameterization)

    def _project(self, i, p):
        for link in self.links:
            p = link.project(i, p)
        return p

    def _pred_x0(self, x, e_t, a, sqrt_1m_a, clip, with_eps=False):
        """(the prediction, the noise estimate): e_t itself under "eps"; under "x0" / "v" eod_param_pred's, or None unless with_eps"""
        p0 = torch.empty_like(x)
        if self.kind == 0:
            _lib.check(_lib.lib().eod_pred_x0(x.data_ptr(), e_t.data_ptr(), float(a), float(sqrt_1m_a), int(bool(clip)), p0.data_ptr(), x.numel(),
                                              current_stream_ptr(x.device)), "eod_pred_x0")
            return p0, e_t
        eps = torch.empty_like(x) if with_eps else None
        _lib.check(_lib.lib().eod_param_pred(x.data_ptr(), e_t.data_ptr(), self.kind, float(a), float(sqrt_1m_a), int(bool(clip)), p0.data_ptr(),
                                             _lib.ptr(eps), x.numel(), current_stream_ptr(x.device)), "eod_param_pred")
        return p0, eps

    def ddim_step(self, i, x, e_t, noise, a_t, a_prev, sigma_t, sqrt_1m_at, temperature):
        x, e_t = f32c(x), f32c(e_t)
        pred_x0, e_t = self._pred_x0(x, e_t, a_t, sqrt_1m_at, False, with_eps=True)
        pred_x0 = self._project(i, pred_x0)
        x_prev = torch.empty_like(x)
        _lib.check(_lib.lib().eod_ddim_step_p0(e_t.data_ptr(), pred_x0.data_ptr(), _lib.ptr(noise), float(a_prev), float(sigma_t),
                                               float(temperature), x_prev.data_ptr(), x.numel(), current_stream_ptr(x.device)), "eod_ddim_step_p0")
        return x_prev, pred_x0

    def dpmpp_step(self, i, x, e_t, d_prev, a_s, sqrt_1m_as, c_x, c_d, w_cur, w_prev, clip):
        x, e_t = f32c(x), f32c(e_t)
        pred_x0 = self._project(i, self._pred_x0(x, e_t, a_s, sqrt_1m_as, clip and self.threshold is None)[0])
        x_next = torch.empty_like(x)
        _lib.check(_lib.lib().eod_dpmpp_step_p0(x.data_ptr(), pred_x0.data_ptr(), _lib.ptr(d_prev), float(c_x), float(c_d), float(w_cur),
                                                float(w_prev), x_next.data_ptr(), x.numel(), current_stream_ptr(x.device)), "eod_dpmpp_step_p0")
        return x_next, pred_x0


def bind(observation, what, shape, n_evaluations, device):
    """None, or the observation bound to the call (every refusal before anything is launched).  An Observation, a SpectralObservation or a
    PsfObservation, or a list / tuple of 1 .. 4 of them: one takes its fused step kernel (a PsfObservation has none: a BoundChain of
    one), more become a BoundChain."""
    if observation is None:
        return None
    kinds = (Observation, SpectralObservation, PsfObservation)
    if isinstance(observation, PsfObservation):
        link = observation.bind(what, shape, n_evaluations, device)
        return None if device is None else BoundChain([link])
    if isinstance(observation, kinds):
        return observation.bind(what, shape, n_evaluations, device)
    if not isinstance(observation, (list, tuple)):
        raise _lib.EodError(f"{what}: `observation` is an Observation, a SpectralObservation, a PsfObservation or a list of them, got "
                            f"{type(observation).__name__}")
    if not 1 <= len(observation) <= MAX_LINKS:
        raise _lib.EodError(f"{what}: a chain of observations has 1 .. {MAX_LINKS} links, got {len(observation)}")
    for link in observation:
        if not isinstance(link, kinds):
            raise _lib.EodError(f"{what}: a link of `observation` is an Observation, a SpectralObservation or a PsfObservation, got "
                                f"{type(link).__name__}")
    links = [link.bind(what, shape, n_evaluations, device) for link in observation]
    if device is None:
        return None
    return links[0] if len(links) == 1 and not isinstance(links[0], BoundPsf) else BoundChain(links)


def check(observation, what, shape, n_evaluations):
    """every refusal of bind() with nothing copied or launched (EODiffusion.check_scene_args)"""
    bind(observation, what, shape, n_evaluations, None)


def shard(observation, n_total, lo, hi):
    """None, an observation's shard(n_total, lo, hi), or every link's when it is a list / tuple (anything else: left for bind() to refuse)"""
    if isinstance(observation, (list, tuple)):
        return [link.shard(n_total, lo, hi) if hasattr(link, "shard") else link for link in observation]
    return observation.shard(n_total, lo, hi) if hasattr(observation, "shard") else observation


def ddpm_pred_x0(parameterization, x, o, t, acp, sqrt_acp, sqrt_1m_acp, clip):
    """the data prediction of the model output o [N, ...] at per-sample timesteps t (int64 [N] on the device): eod_ddpm_pred_x0 for "eps"
    (from the acp table), eod_ddpm_param_pred for "x0" / "v" (from the two square-root tables of eod_q_sample); contiguous fp32 tensors"""
    kind = parameterization_kind("ddpm_pred_x0", parameterization)
    n, T, stream = x.shape[0], acp.numel(), current_stream_ptr(x.device)
    p = torch.empty_like(x)
    if kind == 0:
        _lib.check(_lib.lib().eod_ddpm_pred_x0(x.data_ptr(), o.data_ptr(), t.data_ptr(), acp.data_ptr(), p.data_ptr(), n, x.numel() // n, T,
                                               int(bool(clip)), stream), "eod_ddpm_pred_x0")
    else:
        _lib.check(_lib.lib().eod_ddpm_param_pred(x.data_ptr(), o.data_ptr(), t.data_ptr(), sqrt_acp.data_ptr(), sqrt_1m_acp.data_ptr(), kind,
                                                  int(bool(clip)), p.data_ptr(), n, x.numel() // n, T, stream), "eod_ddpm_param_pred")
    return p


def ddpm_var_pred(parameterization, x, o, t, acp, sqrt_acp, sqrt_1m_acp, clip):
    """ddpm_pred_x0 on the mean half of a learned-variance output o [N, 2 C, ...], read in place (eod_ddpm_var_pred): the bits of
    ddpm_pred_x0 on a dense copy of that half"""
    kind = parameterization_kind("ddpm_var_pred", parameterization)
    n, T, stream = x.shape[0], acp.numel(), current_stream_ptr(x.device)
    if o.numel() != 2 * x.numel() or o.shape[0] != n:
        raise _lib.EodError(f"ddpm_var_pred: the output of a learned-variance model has twice the state's channels, got {tuple(o.shape)} "
                            f"for a state {tuple(x.shape)}")
    p = torch.empty_like(x)
    _lib.check(_lib.lib().eod_ddpm_var_pred(x.data_ptr(), o.data_ptr(), t.data_ptr(), acp.data_ptr(), _lib.ptr(sqrt_acp), _lib.ptr(sqrt_1m_acp),
                                            kind, int(bool(clip)), p.data_ptr(), n, x.numel() // n, T, stream), "eod_ddpm_var_pred")
    return p


def ddpm_step(bound, k, x_t, pred, noise, t, betas, alphas, acp, clip, sqrt_acp=None, sqrt_1m_acp=None, var=None):
    """One ancestral (DDPM) update with an observation: eod_ddpm_pred_x0 -> each link's project(k, p) in order -> eod_ddpm_step_p0.
    A BoundChain of an "x0" / "v" model forms the prediction with eod_ddpm_param_pred from `pred`, the model's raw output, and the tables
    sqrt_acp / sqrt_1m_acp [T] (the model's buffers); its `links` may be empty.
    bound: a BoundObservation, BoundSpectral, BoundPsf or BoundChain (a single link is a chain of one); k: the evaluation's number in the
    walk (what `weight` sequences are indexed by; not the timestep); t int64 [N] and the schedule tables [T] on the device.  clip False:
    the same posterior form without the clamp (algebraically the reference's epsilon form, not its bits).  A chain with a threshold
    (diffusion/threshold.py) forms its prediction without the clamp whatever `clip` says: the threshold, its link 0, replaces it.
    var: EODiffusion.variance_tables() of a learned-variance model, whose `pred` is [N, 2 C, ...] = [mean | v]: eod_ddpm_var_pred on the mean
    half -> the links -> eod_ddpm_step_p0_var, which takes every element's standard deviation from v."""
    x, e, z = f32c(x_t), f32c(pred), f32c(noise)
    clip = clip and getattr(bound, "threshold", None) is None
    n, T, stream = x.shape[0], acp.numel(), current_stream_ptr(x.device)
    parameterization = PARAMETERIZATIONS[getattr(bound, "kind", 0)]
    if var is None:
        p = ddpm_pred_x0(parameterization, x, e, t, acp, sqrt_acp, sqrt_1m_acp, clip)
    else:
        p = ddpm_var_pred(parameterization, x, e, t, acp, sqrt_acp, sqrt_1m_acp, clip)
    for link in (bound.links if isinstance(bound, BoundChain) else (bound,)):
        p = link.project(k, p)
    out = torch.empty_like(x)
    if var is not None:
        _lib.check(_lib.lib().eod_ddpm_step_p0_var(x.data_ptr(), p.data_ptr(), e.data_ptr(), z.data_ptr(), t.data_ptr(), betas.data_ptr(),
                                                   alphas.data_ptr(), acp.data_ptr(), var["sigma_min"].data_ptr(), var["half_gap"].data_ptr(),
                                                   out.data_ptr(), n, x.numel() // n, T, stream), "eod_ddpm_step_p0_var")
        return out
    _lib.check(_lib.lib().eod_ddpm_step_p0(x.data_ptr(), p.data_ptr(), z.data_ptr(), t.data_ptr(), betas.data_ptr(), alphas.data_ptr(),
                                           acp.data_ptr(), out.data_ptr(), n, x.numel() // n, T, stream), "eod_ddpm_step_p0")
    return out


def block_mean(x, factors):
    """A+ A x on the GPU (eod_block_mean): every pixel of x [B, C, H, W] replaced by the mean of its f_c x f_c block.  Makes an
    observation out of a full-resolution image, and measures how far a result is from one."""
    what = "block_mean"
    fs = _factors(what, factors)
    if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != len(fs):
        raise _lib.EodError(f"{what}: x must be a tensor [B, {len(fs)}, H, W] ({len(fs)} factors were given)")
    B, C, H, W = x.shape
    _divides(what, fs, H, W)
    require_gpu(x, what)
    x = f32c(x)
    out = torch.empty_like(x)
    _lib.check(_lib.lib().eod_block_mean(x.data_ptr(), _c_factors(fs), out.data_ptr(), B, C, H, W, current_stream_ptr(x.device)), "eod_block_mean")
    return out


def spectral_response(x, response, factor=1):
    """R (x) D_f of x on the GPU (eod_spec_apply): [B, K, H, W], band k = sum_c response[k][c] * (the factor x factor block mean of channel c),
    replicated onto the full-resolution grid.  Makes a SpectralObservation's `values` out of an image, and measures how far a result is
    from one."""
    what = "spectral_response"
    R = _response(what, response)
    f = _factor(what, factor)
    K, C = R.shape
    if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != C:
        raise _lib.EodError(f"{what}: x must be a tensor [B, {C}, H, W] (`response` mixes {C} channels)")
    B, _, H, W = x.shape
    if H % f or W % f:
        raise _lib.EodError(f"{what}: factor = {f} does not divide {H} x {W}")
    require_gpu(x, what)
    x = f32c(x)
    out = torch.empty((B, K, H, W), device=x.device, dtype=torch.float32)
    _lib.check(_lib.lib().eod_spec_apply(x.data_ptr(), _c_floats(R), K, f, out.data_ptr(), B, C, H, W, current_stream_ptr(x.device)), "eod_spec_apply")
    return out


def psf_observe(x, psf, factor, channels=None, response=None):
    """A x on the GPU (eod_psf_apply): [B, K, H / f, W / f], the channels `channels` (None: all) of x [B, C, H, W] blurred by the
    renormalised zero-padded separable PSF and averaged over factor x factor blocks.  Makes a PsfObservation's `values` out of an image,
    and measures how far a result is from one.  With `response` [K, C] (not together with `channels`): the K band mixes of x seen that
    way (eod_psf_apply_mix).  psf: the symmetric 1-D taps, or a SeparablePsf (eod_psf_apply_xy, either form)."""
    what = "psf_observe"
    xy = isinstance(psf, SeparablePsf)               # one tap vector per axis: eod_psf_apply_xy, either form
    h = None if xy else _taps(what, psf)
    f = _factor(what, factor)
    if not torch.is_tensor(x) or x.dim() != 4 or not 1 <= x.shape[1] <= MAX_CHANNELS:
        raise _lib.EodError(f"{what}: x must be a tensor [B, C <= {MAX_CHANNELS}, H, W]")
    B, C, H, W = (int(d) for d in x.shape)
    if response is not None:
        if channels is not None:
            raise _lib.EodError(f"{what}: `response` mixes all channels of x; it cannot be given together with `channels`")
        R = _response(what, response)
        if R.shape[1] != C:
            raise _lib.EodError(f"{what}: `response` mixes {R.shape[1]} channels, x has {C}")
        K, c_cs, c_R = R.shape[0], None, _c_floats(R)
    else:
        cs = tuple(range(C)) if channels is None else _channels(what, channels)
        if cs[-1] >= C:
            raise _lib.EodError(f"{what}: channel {cs[-1]} of an x with {C} channels")
        K, c_cs, c_R = len(cs), _c_ints(cs), None
    if H % f or W % f:
        raise _lib.EodError(f"{what}: factor = {f} does not divide {H} x {W}")
    require_gpu(x, what)
    x = f32c(x)
    out = torch.empty((B, K, H // f, W // f), device=x.device, dtype=torch.float32)
    if xy:
        name, args = "eod_psf_apply_xy", (_c_floats(psf.taps_y), psf.radii[0], _c_floats(psf.taps_x), psf.radii[1], f, c_cs, c_R)
    else:
        name, args = ("eod_psf_apply" if c_R is None else "eod_psf_apply_mix"), (_c_floats(h), h.size // 2, f, c_cs if c_R is None else c_R)
    _lib.check(getattr(_lib.lib(), name)(x.data_ptr(), *args, K, out.data_ptr(), B, C, H, W, current_stream_ptr(x.device)), name)
    return out
