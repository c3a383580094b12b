"""Observation-consistent sampling: the host-side description of a block-mean observation and the calls of the fused kernels that impose
it (eod_ddim_step_obs, eod_dpmpp_step_obs, eod_block_mean in csrc/sampler.hip).  No counterpart in the reference; DESIGN.md section 9.5.

What is known about channel c is its mean over every f_c x f_c block (f_c = 1: the channel at full resolution), where a mask says so.
With A = masked per-channel block mean and A+ = replication, every evaluation of DDIMSampler / DPMSolverSampler replaces its data
prediction p0 by p0 - weight * mask * (A+ A p0 - values) before the update uses it: the range / null-space projection of DDNM
(Wang et al. 2022) fused into the step kernel.  Per pixel, what the kernel computes for ANY values / mask is stated in include/eodiff.h;
it is the projection when values and mask are constant on every block and the mask is 0 or 1.
"""
import ctypes
import math
import numbers

import numpy as np
import torch

from .. import _lib
from ..engine import current_stream_ptr, f32c, require_gpu

MAX_FACTOR = 8
MAX_CHANNELS = 32


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
        if isinstance(weight, (numbers.Real, np.floating)) and not isinstance(weight, bool):
            ws, self.per_evaluation = [weight], False
        else:
            try:
                ws = list(weight)
            except TypeError:
                raise _lib.EodError(f"{what}: `weight` is a float or a sequence of floats, got {weight!r}") from None
            self.per_evaluation = True
        for w in ws:
            if isinstance(w, bool) or not isinstance(w, (numbers.Real, np.floating)) or not math.isfinite(float(w)):
                raise _lib.EodError(f"{what}: a weight is a finite float, got {w!r}")
            if not 0.0 <= float(np.float32(w)) <= 1.0:
                raise _lib.EodError(f"{what}: a weight lies in [0, 1], got {w!r}")
        self.weights = [float(np.float32(w)) for w in ws]
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
        return BoundObservation(self, (B, C, H, W), n_evaluations, device)


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


def bind(observation, what, shape, n_evaluations, device):
    """None, or the observation bound to the call (every refusal before anything is launched)"""
    if observation is None:
        return None
    if not isinstance(observation, Observation):
        raise _lib.EodError(f"{what}: `observation` is an Observation, got {type(observation).__name__}")
    return observation.bind(what, shape, n_evaluations, device)


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
