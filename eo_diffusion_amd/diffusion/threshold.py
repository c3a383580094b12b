"""Dynamic thresholding (Saharia et al. 2022, "Imagen"): every evaluation's data prediction is clamped to the sample's own q-quantile s of
|p0| (never below 1) and divided by s, where the static clamp fminf(fmaxf(p0, -1), 1) saturates whole regions once |p0| runs far beyond
1 -- under guidance, and in the early high-noise evaluations of a short DPM-Solver++ walk.  No counterpart in the reference; DESIGN.md
section 9.12.  The operator is eod_dyn_threshold (csrc/threshold.hip; include/eodiff.h states its operations): an exact order statistic by
radix selection, so a sample's bits depend on the sample alone -- not on the batch, the grid or the arrival order -- and n may be anything
up to 2^31 - 1 (torch.quantile stops at 16 M elements and computes the rank in fp32).

`threshold=DynamicThreshold(...)` on the six samplers: every evaluation runs prediction WITHOUT the static clamp (eod_pred_x0 /
eod_ddpm_pred_x0 with clip = 0) -> the threshold -> the observation's links in order, if any -> eod_ddim_step_p0 / eod_dpmpp_step_p0 /
eod_ddpm_step_p0.  The bound threshold is link 0 of a consistency.BoundChain (it does not count towards MAX_LINKS).  Where the quantile is
at most 1 the operator IS the static clamp, bit for bit, and the route has the bits of the clipped fused step.
"""
import math
import numbers

import torch

from .. import _lib
from ..engine import current_stream_ptr, f32c, quantile_rank, require_gpu
from . import consistency

MAX_N = 2 ** 31 - 1     # elements of one sample (eod_dyn_threshold)
PER = ("sample", "channel")


class DynamicThreshold:
    """quantile: q in [0, 1] of |p0| (0.995 in Imagen); max_value: None (no cap) or a float >= 1 the scale s is capped at;
    per="sample": one threshold per batch member / scene over C*H*W; per="channel": one per band over H*W (EO bands differ in range).
    s = min(max(quantile, 1), max_value); the prediction becomes clamp(p0, -s, s) / s."""

    def __init__(self, quantile=0.995, max_value=None, per="sample"):
        what = "DynamicThreshold"
        if isinstance(quantile, bool) or not isinstance(quantile, numbers.Real) or not 0.0 <= float(quantile) <= 1.0:  # (NaN fails the comparison)
            raise _lib.EodError(f"{what}: quantile is a number in [0, 1], got {quantile!r}")
        if max_value is not None and (isinstance(max_value, bool) or not isinstance(max_value, numbers.Real) or not float(max_value) >= 1.0):
            raise _lib.EodError(f"{what}: max_value is None or a number >= 1 (the scale is never below 1), got {max_value!r}")
        if per not in PER:
            raise _lib.EodError(f"{what}: per is 'sample' or 'channel', got {per!r}")
        self.quantile = float(quantile)
        self.max_value = None if max_value is None else float(max_value)
        self.cap = math.inf if max_value is None else float(max_value)
        self.per = per
        self.last_bound = None

    def __repr__(self):
        return f"DynamicThreshold(quantile={self.quantile!r}, max_value={self.max_value!r}, per={self.per!r})"

    def rank(self, n):
        """(k, frac) of eod_dyn_threshold for samples of n elements: pos = q * (n - 1) in float64, k = floor(pos), frac = fp32(pos - k)
        (returned as the Python float that holds the fp32 value); frac < 1 after the rounding, too"""
        return quantile_rank(self.quantile, n)

    def samples(self, shape):
        """(number of samples, elements of one) of a state [B, C, H, W]"""
        B, C, H, W = (int(s) for s in shape)
        return (B * C, H * W) if self.per == "channel" else (B, C * H * W)

    def bind(self, what, shape, device):
        """The threshold for a call on a state of `shape` = (B, C, H, W): every refusal first, then the workspace and the scale tensor,
        allocated once per call.  device None: the refusals alone.  Returns a BoundThreshold, which is also kept as `last_bound`: after a
        sampler call, threshold.last_bound.last_scale is the scale of that call's latest evaluation."""
        if len(tuple(shape)) != 4:
            raise _lib.EodError(f"{what}: the threshold takes a state [B, C, H, W], got {tuple(shape)}")
        S, n = self.samples(shape)
        if S < 1 or n < 1:
            raise _lib.EodError(f"{what}: the threshold takes a non-empty state, got {tuple(shape)}")
        if n > MAX_N:
            raise _lib.EodError(f"{what}: the threshold takes samples of at most 2^31 - 1 elements, a {self.per} of {tuple(shape)} has {n}")
        if S > MAX_N:
            raise _lib.EodError(f"{what}: the threshold takes at most 2^31 - 1 samples, {tuple(shape)} has {S}")
        if device is None:
            return None
        self.last_bound = BoundThreshold(self, tuple(int(s) for s in shape), device)
        return self.last_bound


class BoundThreshold:
    """A DynamicThreshold bound to a state shape: owns the workspace and the scale tensor of the call.  project(i, p) is the link interface
    of consistency.BoundChain; last_scale is the device tensor [B] (per="channel": [B, C]) of the latest evaluation -- reading it is the
    caller's synchronisation, not the sampler's."""

    def __init__(self, thr, shape, device):
        self.shape = shape
        self.S, self.n = thr.samples(shape)
        self.k, self.frac = thr.rank(self.n)
        self.cap = thr.cap
        self.ws = torch.empty(int(_lib.lib().eod_dyn_threshold_workspace_size(self.S, self.n)), dtype=torch.uint8, device=device)
        self.last_scale = torch.empty((shape[0], shape[1]) if thr.per == "channel" else (shape[0],), dtype=torch.float32, device=device)

    def project(self, i, p):
        """the thresholded prediction of evaluation number i (the threshold has no per-evaluation state: i is not used)"""
        if tuple(p.shape) != self.shape:
            raise _lib.EodError(f"threshold bound to a state of shape {self.shape}, the step got {tuple(p.shape)}")
        p = f32c(p)
        out = torch.empty_like(p)
        _lib.check(_lib.lib().eod_dyn_threshold(p.data_ptr(), self.k, self.frac, self.cap, out.data_ptr(), self.last_scale.data_ptr(), self.S,
                                                self.n, self.ws.data_ptr(), self.ws.numel(), current_stream_ptr(p.device)), "eod_dyn_threshold")
        return out


def check(threshold, what, shape):
    """every refusal of a sampler's `threshold=` from the arguments alone (nothing allocated or launched)"""
    if threshold is None:
        return
    if not isinstance(threshold, DynamicThreshold):
        raise _lib.EodError(f"{what}: `threshold` is a DynamicThreshold or None, got {type(threshold).__name__}")
    threshold.bind(what, shape, None)


def no_skip(what, skip_known, threshold):
    if skip_known and threshold is not None:
        raise _lib.EodError(f"{what}: skip_known=True cannot be combined with `threshold`: a skipped tile has no estimate, and the "
                            "prediction at non-estimated pixels would enter the quantile")


def bind(threshold, observation, what, shape, n_evaluations, device, parameterization="eps"):
    """consistency.bind(observation, ...) with the threshold in front: None when both are None, the bound observation as before when
    threshold is None, else a BoundChain whose link 0 is the BoundThreshold (the chain then forms its prediction without the static
    clamp).  Every refusal of either comes before anything is allocated or launched; device None: the refusals alone.
    parameterization: the model's.  "x0" / "v": ALWAYS a BoundChain that carries it -- a single observation as a chain of one (its fused
    step kernel starts from a noise estimate), neither observation nor threshold as a chain with no links."""
    check(threshold, what, shape)
    consistency.parameterization_kind(what, parameterization)
    if threshold is None and parameterization == "eps":
        return consistency.bind(observation, what, shape, n_evaluations, device)
    consistency.bind(observation, what, shape, n_evaluations, None)
    if device is None:
        return None
    obs = consistency.bind(observation, what, shape, n_evaluations, device)
    links = [] if obs is None else (obs.links if isinstance(obs, consistency.BoundChain) else [obs])
    return consistency.BoundChain(links, threshold=None if threshold is None else threshold.bind(what, shape, device),
                                  parameterization=parameterization)


def dynamic_threshold(x, quantile=0.995, max_value=None, per="sample"):
    """The operator alone on a GPU tensor x [B, C, H, W] (eod_dyn_threshold): returns (out, s), s [B] or, per="channel", [B, C]."""
    what = "dynamic_threshold"
    thr = DynamicThreshold(quantile, max_value, per)
    if not torch.is_tensor(x) or x.dim() != 4:
        raise _lib.EodError(f"{what}: x must be a tensor [B, C, H, W]")
    thr.bind(what, x.shape, None)
    require_gpu(x, what)
    bound = thr.bind(what, x.shape, x.device)
    out = bound.project(0, x)
    return out, bound.last_scale
