"""Fused optimizer side of the training step on the HIP path (train.py:70-75,119-124): `AdamW` and
`ExponentialMovingAverage` with the constructor signatures the reference uses, running as ONE kernel launch over flat fp32
buffers (csrc/train.hip: eod_adamw_step, eod_ema_update) instead of torch's per-tensor loops, and `mse_loss`.
Opt-in, for a learned-variance model: `hybrid_loss` / `HybridLoss` (L_simple + lambda L_vlb with both gradients, eod_hybrid_loss).
Opt-in, the objective beyond plain MSE: `diffusion_loss` / `DiffusionLoss` (masked, per-sample-weighted l1 / l2 / huber with its
gradient, eod_diffusion_loss) and `AdamW(max_grad_norm=...)` (gradient clipping to a global norm inside the guarded step).

    from eo_diffusion_amd.optim import AdamW, ExponentialMovingAverage        # instead of torch.optim / utils.py
    optimizer = AdamW(model.parameters(), lr=args.lr)
    model_ema = ExponentialMovingAverage(model, device=device, decay=1.0 - alpha)

`AdamW` moves the parameters into one flat buffer (each `p.data` becomes a view of it, values unchanged), so checkpoints,
`state_dict()` and the weight re-packing of the kernels keep working on the same Parameter objects."""
import copy

import torch

from . import _lib
from ._lib import check, ptr
from .engine import current_stream_ptr


def _flatten(tensors, device):
    """one flat fp32 buffer + views (16-byte aligned) holding `tensors`' values"""
    offs, off = [], 0
    for t in tensors:
        offs.append(off)
        off += (t.numel() + 3) // 4 * 4
    flat = torch.zeros((off,), dtype=torch.float32, device=device)
    views = []
    for t, o in zip(tensors, offs):
        v = flat[o:o + t.numel()].view(t.shape)
        v.copy_(t.detach())
        views.append(v)
    return flat, views


def mse_loss(pred, target, want_grad=True):
    """nn.MSELoss(reduction='mean') (train.py:86,117) on the GPU: returns (loss [1] fp32 tensor, dLoss/dpred or None)"""
    L = _lib.lib()
    if not pred.is_cuda:
        raise _lib.EodError("mse_loss: tensors must be on the HIP GPU")
    p, t = pred.detach().contiguous().float(), target.detach().contiguous().float()
    loss = torch.empty((1,), dtype=torch.float32, device=p.device)
    dp = torch.empty_like(p) if want_grad else None
    scratch = torch.empty((1024,), dtype=torch.float32, device=p.device)
    check(L.eod_mse_loss(ptr(p), ptr(t), p.numel(), ptr(loss), ptr(dp), ptr(scratch), 1024, current_stream_ptr(p.device)), "eod_mse_loss")
    return loss, dp


LOSS_KINDS = {"l2": 0, "l1": 1, "huber": 2}
SUMSQ_SLOTS = 4096  # workgroups of the clipped step's scan (eod_grad_sumsq): one float64 slot each, folded 64 at a time in two launches


def _loss_args(pred, target, mask, weight, kind, delta):
    """the refusals of diffusion_loss, host-side and before any launch; returns the kind's id"""
    what = "diffusion_loss"
    if kind not in LOSS_KINDS:
        raise _lib.EodError(f"{what}: kind must be one of {sorted(LOSS_KINDS)}, got {kind!r}")
    if isinstance(delta, bool) or not isinstance(delta, (int, float)) or not delta > 0:
        raise _lib.EodError(f"{what}: delta must be a number > 0, got {delta!r}")
    for name, t in (("pred", pred), ("target", target), ("mask", mask), ("weight", weight)):
        if t is None and name in ("mask", "weight"):
            continue
        if not isinstance(t, torch.Tensor):
            raise _lib.EodError(f"{what}: `{name}` must be a tensor, got {type(t).__name__}")
        if not t.is_cuda:
            raise _lib.EodError(f"{what}: `{name}` must be on the HIP GPU, it is on {t.device}")
        if t.device != pred.device:
            raise _lib.EodError(f"{what}: `{name}` is on {t.device}, pred on {pred.device}")
        if t.dtype != torch.float32:
            raise _lib.EodError(f"{what}: `{name}` must be float32, got {t.dtype}")
    if pred.dim() != 4 or pred.numel() == 0:
        raise _lib.EodError(f"{what}: pred must be [N, C, H, W], got {tuple(pred.shape)}")
    if target.shape != pred.shape:
        raise _lib.EodError(f"{what}: target {tuple(target.shape)} does not match pred {tuple(pred.shape)}")
    n, c, h, w = pred.shape
    if mask is not None and (mask.dim() != 4 or mask.shape[0] not in (1, n) or mask.shape[1] not in (1, c) or tuple(mask.shape[2:]) != (h, w)):
        raise _lib.EodError(f"{what}: mask must be [{n} or 1, {c} or 1, {h}, {w}], got {tuple(mask.shape)}")
    if weight is not None and tuple(weight.shape) != (n,):
        raise _lib.EodError(f"{what}: weight must be [{n}], got {tuple(weight.shape)}")
    return LOSS_KINDS[kind]


def diffusion_loss(pred, target, *, mask=None, weight=None, kind="l2", delta=1.0, want_grad=True, return_per_sample=False):
    """The objective of the reference's vendored trainers (denoising_diffusion_pytorch.py:662-706: loss_type, mean per sample, times a
    per-timestep weight, mean over the batch) with a pixel mask, in one C call (eod_diffusion_loss, csrc/train.hip):
        S_n = sum m,  L_n = sum m * l(pred - target) / S_n (0 where S_n = 0),  loss = mean_n weight_n * L_n
    kind: "l2" (d^2) | "l1" (|d|) | "huber" (torch's huber_loss with `delta`).  mask: fp32 [N or 1, 1 or C, H, W], finite and >= 0, 0 = no
    loss here (cloud, shadow, nodata); such an element is skipped, so pred / target may hold NaN there; a one-channel mask counts once
    per channel.  weight: fp32 [N], e.g. EODiffusion.loss_weights("min_snr", 5.0)[t].  All tensors fp32 on the GPU (no conversions here).
    Returns (loss [1], dLoss/dpred or None) like mse_loss; with return_per_sample=True also the L_n [N] (the loss by timestep bucket).
    No mask, no weight, "l2": nn.MSELoss(reduction="mean") up to rounding."""
    k = _loss_args(pred, target, mask, weight, kind, delta)
    L = _lib.lib()
    p, t = pred.detach().contiguous(), target.detach().contiguous()
    m = None if mask is None else mask.detach().contiguous()
    w = None if weight is None else weight.detach().contiguous()
    n, c, h, wd = p.shape
    loss = torch.empty((1,), dtype=torch.float32, device=p.device)
    per = torch.empty((n,), dtype=torch.float32, device=p.device)
    dp = torch.empty_like(p) if want_grad else None
    nbytes = L.eod_diffusion_loss_workspace_size(n, c, h, wd)
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=p.device)
    check(L.eod_diffusion_loss(ptr(p), ptr(t), ptr(m), 0 if m is None else m.shape[0], 0 if m is None else m.shape[1], ptr(w), n, c, h, wd, k,
                               float(delta), ptr(loss), ptr(per), ptr(dp), ptr(ws), nbytes, current_stream_ptr(p.device)), "eod_diffusion_loss")
    return (loss, dp, per) if return_per_sample else (loss, dp)


class _DiffusionLossFn(torch.autograd.Function):
    """the HIP-computed dpred kept for backward, times the incoming gradient"""

    @staticmethod
    def forward(ctx, pred, target, mask, weight, kind, delta, owner):
        loss, dp, per = diffusion_loss(pred, target, mask=mask, weight=weight, kind=kind, delta=delta, want_grad=True, return_per_sample=True)
        owner.per_sample = per
        ctx.save_for_backward(dp)
        return loss[0]

    @staticmethod
    def backward(ctx, gout):
        dp, = ctx.saved_tensors
        return dp * gout, None, None, None, None, None, None


class DiffusionLoss(torch.nn.Module):
    """diffusion_loss as a loss module: `loss = loss_fn(pred, noise, mask=.., weight=..); loss.backward()` -- the reference's loop shape
    (train.py:117-118) with nn.MSELoss replaced.  The scalar is connected to `pred` only (target, mask and weight get no gradient).
    `per_sample` holds the latest L_n [N]."""

    def __init__(self, kind="l2", delta=1.0):
        super().__init__()
        if kind not in LOSS_KINDS:
            raise _lib.EodError(f"DiffusionLoss: kind must be one of {sorted(LOSS_KINDS)}, got {kind!r}")
        if isinstance(delta, bool) or not isinstance(delta, (int, float)) or not delta > 0:
            raise _lib.EodError(f"DiffusionLoss: delta must be a number > 0, got {delta!r}")
        self.kind, self.delta = kind, float(delta)
        self.per_sample = None

    def forward(self, pred, target, mask=None, weight=None):
        return _DiffusionLossFn.apply(pred, target, mask, weight, self.kind, self.delta, self)


def _finite_number(what, name, v, positive=False):
    import math
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or (positive and not v > 0):
        raise _lib.EodError(f"{what}: {name} must be a finite number{' > 0' if positive else ''}, got {v!r}")
    return float(v)


def hybrid_loss(o, target, x_0, x_t, t, diffusion, *, mask=None, weight=None, kind="l2", delta=1.0, vlb_weight=1e-3, bin_halfwidth=1.0 / 255.0,
                want_grad=True, return_terms=False):
    """The hybrid objective of a learned-variance model (Nichol & Dhariwal 2021) in one C call (eod_hybrid_loss):
        loss = mean_n (weight_n * L_n + vlb_weight * V_n)
    o [N, 2 C, H, W] = [mean | v], target, x_0, x_t [N, C, H, W] and t int64 [N]: what diffusion.forward(x_0, noise, t=t, return_target=True,
    return_state=True) returned; diffusion: the EODiffusion (learned_variance=True), whose parameterization and variance_tables() are used.
    L_n: diffusion_loss's per-sample term of the mean half against target (kind, delta, mask, weight: as there, bit for bit).  V_n: the
    masked mean of the variational-bound term in bits per element, float64, with the mean detached -- the KL between the true posterior
    and N(mu_theta, exp(lv_theta)) at t > 0, the likelihood of x_0 under that Gaussian discretised to bins of half-width bin_halfwidth at
    t = 0 (per sample; the exact normal distribution function, not guided-diffusion's tanh approximation).  The weight applies to L_n only.
    Returns (loss [1], dLoss/do [N, 2 C, H, W] or None); with return_terms=True also (L_n fp32 [N], V_n float64 [N])."""
    what = "hybrid_loss"
    if not getattr(diffusion, "learned_variance", False):
        raise _lib.EodError(f"{what}: `diffusion` must be an EODiffusion with learned_variance=True")
    lam, h = _finite_number(what, "vlb_weight", vlb_weight), _finite_number(what, "bin_halfwidth", bin_halfwidth, positive=True)
    if not isinstance(o, torch.Tensor) or not isinstance(target, torch.Tensor) or o.dim() != 4 or target.dim() != 4 or \
            tuple(o.shape) != (target.shape[0], 2 * target.shape[1]) + tuple(target.shape[2:]):
        got = [tuple(v.shape) if isinstance(v, torch.Tensor) else type(v).__name__ for v in (o, target)]
        raise _lib.EodError(f"{what}: o must be [N, 2 C, H, W] for a target [N, C, H, W], got {got[0]} and {got[1]}")
    k = _loss_args(target, target, mask, weight, kind, delta)
    for name, v in (("o", o), ("x_0", x_0), ("x_t", x_t)):
        if not isinstance(v, torch.Tensor) or v.device != target.device or v.dtype != torch.float32:
            raise _lib.EodError(f"{what}: `{name}` must be a float32 tensor on {target.device}")
        if name != "o" and v.shape != target.shape:
            raise _lib.EodError(f"{what}: `{name}` {tuple(v.shape)} does not match target {tuple(target.shape)}")
    n, c, hh, wd = target.shape
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or tuple(t.shape) != (n,) or t.device != target.device:
        raise _lib.EodError(f"{what}: t must be an int64 tensor [{n}] on {target.device}")
    if c != diffusion.in_channels or diffusion.betas.device != target.device:
        raise _lib.EodError(f"{what}: the tensors have {c} channels on {target.device}, the model {diffusion.in_channels} on {diffusion.betas.device}")
    L = _lib.lib()
    tb = diffusion.variance_tables()
    od, tg, x0, xt, tt = (v.detach().contiguous() for v in (o, target, x_0, x_t, t))
    m = None if mask is None else mask.detach().contiguous()
    w = None if weight is None else weight.detach().contiguous()
    loss = torch.empty((1,), dtype=torch.float32, device=od.device)
    simple = torch.empty((n,), dtype=torch.float32, device=od.device)
    vlb = torch.empty((n,), dtype=torch.float64, device=od.device)
    grad = torch.empty_like(od) if want_grad else None
    nbytes = L.eod_hybrid_loss_workspace_size(n, c, hh, wd)
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=od.device)
    check(L.eod_hybrid_loss(ptr(od), ptr(tg), ptr(x0), ptr(xt), ptr(tt), ptr(m), 0 if m is None else m.shape[0], 0 if m is None else m.shape[1],
                            ptr(w), ptr(diffusion.sqrt_alphas_cumprod), ptr(diffusion.sqrt_one_minus_alphas_cumprod), ptr(tb["c1"]), ptr(tb["lmin"]),
                            ptr(tb["gap"]), n, c, hh, wd, diffusion.timesteps, _lib_param_kind(diffusion.parameterization), k, float(delta), lam, h,
                            ptr(loss), ptr(simple), ptr(vlb), ptr(grad), ptr(ws), nbytes, current_stream_ptr(od.device)), "eod_hybrid_loss")
    return (loss, grad, simple, vlb) if return_terms else (loss, grad)


def _lib_param_kind(parameterization):
    from .diffusion.consistency import parameterization_kind
    return parameterization_kind("hybrid_loss", parameterization)


class _HybridLossFn(torch.autograd.Function):
    """the HIP-computed gradient of both halves kept for backward, times the incoming gradient (a loss scale included)"""

    @staticmethod
    def forward(ctx, o, target, x_0, x_t, t, mask, weight, owner):
        loss, grad, simple, vlb = hybrid_loss(o, target, x_0, x_t, t, owner.diffusion, mask=mask, weight=weight, kind=owner.kind, delta=owner.delta,
                                              vlb_weight=owner.vlb_weight, bin_halfwidth=owner.bin_halfwidth, want_grad=True, return_terms=True)
        owner.per_sample, owner.per_sample_vlb = simple, vlb
        ctx.save_for_backward(grad)
        return loss[0]

    @staticmethod
    def backward(ctx, gout):
        grad, = ctx.saved_tensors
        return grad * gout, None, None, None, None, None, None, None


class HybridLoss(torch.nn.Module):
    """hybrid_loss as a loss module, built like DiffusionLoss:
        o, target, x_t, t = diffusion(x, noise, t=t, return_target=True, return_state=True)
        loss = loss_fn(o, target, x, x_t, t, mask=.., weight=..); loss.backward()
    The scalar is connected to `o` only.  `per_sample` holds the latest L_n [N], `per_sample_vlb` the latest V_n [N] (float64, bits per
    element).  The diffusion model is referred to, not registered: it is no sub-module of the loss."""

    def __init__(self, diffusion, kind="l2", delta=1.0, vlb_weight=1e-3, bin_halfwidth=1.0 / 255.0):
        super().__init__()
        if not getattr(diffusion, "learned_variance", False):
            raise _lib.EodError("HybridLoss: `diffusion` must be an EODiffusion with learned_variance=True")
        if kind not in LOSS_KINDS:
            raise _lib.EodError(f"HybridLoss: kind must be one of {sorted(LOSS_KINDS)}, got {kind!r}")
        if isinstance(delta, bool) or not isinstance(delta, (int, float)) or not delta > 0:
            raise _lib.EodError(f"HybridLoss: delta must be a number > 0, got {delta!r}")
        object.__setattr__(self, "diffusion", diffusion)
        self.kind, self.delta = kind, float(delta)
        self.vlb_weight = _finite_number("HybridLoss", "vlb_weight", vlb_weight)
        self.bin_halfwidth = _finite_number("HybridLoss", "bin_halfwidth", bin_halfwidth, positive=True)
        self.per_sample = self.per_sample_vlb = None

    def forward(self, o, target, x_0, x_t, t, mask=None, weight=None):
        return _HybridLossFn.apply(o, target, x_0, x_t, t, mask, weight, self)


class AdamW(torch.optim.Optimizer):
    """torch.optim.AdamW semantics (decoupled weight decay, no amsgrad), one fused launch per parameter group."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, *, skip_nonfinite=True, max_grad_norm=None):
        """skip_nonfinite (default on): a step whose gradients contain inf / NaN (fp16 training overflowing its static loss scale)
        is skipped on the device -- parameters and moments stay untouched; `skipped_steps()` reads the count (one host sync).
        max_grad_norm (a positive float; needs skip_nonfinite): every step clips the gradients to this GLOBAL norm over all parameter
        groups by torch.nn.utils.clip_grad_norm_'s rule (the reference's trainer: denoising_diffusion_pytorch.py:877), on the device and
        inside the step -- the scan that looks for inf / NaN forms the squared norm (eod_grad_sumsq), the update reads g * coef
        (eod_adamw_step_clipped).  Unlike torch's in-place clip, `p.grad` keeps the RAW gradient.  `last_grad_norm()` and
        `clipped_steps()` read the state (one host sync each).  None (default): today's calls."""
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.skip_nonfinite = bool(skip_nonfinite)
        if max_grad_norm is not None:
            if isinstance(max_grad_norm, bool) or not isinstance(max_grad_norm, (int, float)) or not max_grad_norm > 0:
                raise _lib.EodError(f"AdamW: max_grad_norm must be a positive number or None, got {max_grad_norm!r}")
            if not self.skip_nonfinite:
                raise _lib.EodError("AdamW: max_grad_norm needs skip_nonfinite=True (the norm comes out of the guarded step's scan)")
            max_grad_norm = float(max_grad_norm)
        self.max_grad_norm = max_grad_norm
        self._sumsq = None
        self._flat = []
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.requires_grad]
            if not ps:
                self._flat.append(None)
                continue
            dev = ps[0].device
            if dev.type != "cuda" or any(p.dtype != torch.float32 for p in ps):
                raise _lib.EodError("AdamW: parameters must be fp32 tensors on the HIP GPU")
            flat_p, views = _flatten(ps, dev)
            for p, v in zip(ps, views):
                p.data = v  # same values, now contiguous in one buffer
            st = dict(params=ps, p=flat_p, g=torch.zeros_like(flat_p), m=torch.zeros_like(flat_p), v=torch.zeros_like(flat_p), step=0,
                      gviews=[None] * len(ps), guard=torch.zeros((4,), dtype=torch.int32, device=dev),
                      scratch=torch.zeros((8192,), dtype=torch.int32, device=dev))
            if self.max_grad_norm is not None:  # the clipped step's state (10 ints, include/eodiff.h) and the scan's float64 slots
                st["clip"] = torch.zeros((10,), dtype=torch.int32, device=dev)
                st["slots"] = torch.zeros((_lib.lib().eod_grad_sumsq_workspace_size(SUMSQ_SLOTS) // 8,), dtype=torch.float64, device=dev)
            off = 0
            for k, p in enumerate(ps):
                st["gviews"][k] = st["g"][off:off + p.numel()].view(p.shape)
                off += (p.numel() + 3) // 4 * 4
            self._flat.append(st)

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        L = _lib.lib()
        live = [(group, st) for group, st in zip(self.param_groups, self._flat) if st is not None]
        if self.max_grad_norm is not None:
            return self._step_clipped(L, live, loss)
        for group, st in live:
            gptr, untouched = self._gradients(st)
            st["step"] += 1
            b1, b2 = group["betas"]
            if self.skip_nonfinite:
                check(L.eod_adamw_step_guarded(ptr(st["p"]), gptr, ptr(st["m"]), ptr(st["v"]), st["p"].numel(), float(group["lr"]),
                                               float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]), st["step"],
                                               ptr(st["guard"]), ptr(st["scratch"]), 8192, current_stream_ptr(st["p"].device)),
                      "eod_adamw_step_guarded")
            else:
                check(L.eod_adamw_step(ptr(st["p"]), gptr, ptr(st["m"]), ptr(st["v"]), st["p"].numel(), float(group["lr"]), float(b1),
                                       float(b2), float(group["eps"]), float(group["weight_decay"]), st["step"], current_stream_ptr(st["p"].device)),
                      "eod_adamw_step")
            self._after(st, untouched)
        return loss

    def _step_clipped(self, L, live, loss):
        """the norm is global: every group's scan first (one double each), then every group's step folds all of them in group order"""
        if not live:
            return loss
        dev = live[0][1]["p"].device
        if any(st["p"].device != dev for _, st in live):
            raise _lib.EodError("AdamW: max_grad_norm needs every parameter group on one device")
        if self._sumsq is None:
            self._sumsq = torch.zeros((len(live),), dtype=torch.float64, device=dev)
        stream = current_stream_ptr(dev)
        prepared = [self._gradients(st) for _, st in live]
        for k, ((_, st), (gptr, _)) in enumerate(zip(live, prepared)):
            check(L.eod_grad_sumsq(gptr, st["p"].numel(), ptr(self._sumsq) + 8 * k, ptr(st["slots"]), st["slots"].numel() * 8, SUMSQ_SLOTS, stream),
                  "eod_grad_sumsq")
        for (group, st), (gptr, untouched) in zip(live, prepared):
            st["step"] += 1
            b1, b2 = group["betas"]
            check(L.eod_adamw_step_clipped(ptr(st["p"]), gptr, ptr(st["m"]), ptr(st["v"]), st["p"].numel(), float(group["lr"]), float(b1),
                                           float(b2), float(group["eps"]), float(group["weight_decay"]), st["step"], self.max_grad_norm,
                                           ptr(self._sumsq), len(live), ptr(st["clip"]), stream), "eod_adamw_step_clipped")
            self._after(st, untouched)
        return loss

    def _gradients(self, st):
        """(pointer to the group's flat gradient, [(parameter without a gradient, its value, slice, m, v)])"""
        untouched = []  # torch.optim.AdamW skips parameters without a gradient (no decay, no state update): keep their values
        # Fast path: the gradients already lie in ONE flat buffer with this optimizer's own layout (UNetTrainer.flat_grad: same
        # parameter order, same 16-byte-aligned offsets) -> the kernel reads it in place, no per-tensor copies.
        gptr, base, off = ptr(st["g"]), None, 0
        in_place = True
        for p in st["params"]:
            if p.grad is not None:
                b = p.grad.data_ptr() - 4 * off
                if base is None:
                    base = b
                in_place = in_place and b == base and p.grad.dtype == torch.float32 and p.grad.is_contiguous()
            off += (p.numel() + 3) // 4 * 4
        if in_place and base is not None and base % 16 == 0:
            owner = next(p.grad for p in st["params"] if p.grad is not None)
            in_place = owner.untyped_storage().data_ptr() <= base and \
                base + 4 * st["p"].numel() <= owner.untyped_storage().data_ptr() + owner.untyped_storage().nbytes()
        else:
            in_place = False
        def keep(p, o):  # value AND moments of a parameter without a gradient: torch.optim.AdamW leaves all three alone
            sl = slice(o, o + p.numel())
            untouched.append((p, p.detach().clone(), sl, st["m"][sl].clone(), st["v"][sl].clone()))
        off = 0
        if in_place:
            gptr = base
            for p in st["params"]:
                if p.grad is None:  # (its slice of the flat buffer is never written by the backward: zeros)
                    keep(p, off)
                off += (p.numel() + 3) // 4 * 4
        else:
            for p, gv in zip(st["params"], st["gviews"]):
                if p.grad is None:
                    gv.zero_()
                    keep(p, off)
                elif p.grad.data_ptr() != gv.data_ptr():
                    gv.copy_(p.grad)
                off += (p.numel() + 3) // 4 * 4
        return gptr, untouched

    @staticmethod
    def _after(st, untouched):
        for p, val, sl, m0, v0 in untouched:  # undo the weight decay and the moment decay a zero gradient went through
            p.detach().copy_(val)
            st["m"][sl].copy_(m0)
            st["v"][sl].copy_(v0)
        for p in st["params"]:  # written through the flat buffer: advance torch's version counters (the packed-weight
            torch.autograd.graph.increment_version(p)  # caches of the kernels key on them); no kernel is launched

    def _clip_state(self):
        """the clipped step's state of the first live group (the norm, and with it every counter, is the same in all of them)"""
        st = next((st for st in self._flat if st is not None and "clip" in st), None)
        if st is None:
            raise _lib.EodError("AdamW: built without max_grad_norm: there is no clipping state")
        return st["clip"]

    def skipped_steps(self):
        """number of steps skipped because of non-finite gradients (host synchronisation)"""
        if self.max_grad_norm is not None:  # (one global decision per step)
            return int(self._clip_state()[1])
        return sum(int(st["guard"][1]) for st in self._flat if st is not None)

    def clipped_steps(self):
        """number of applied steps whose gradient was scaled down (host synchronisation)"""
        return int(self._clip_state()[3])

    def last_grad_norm(self):
        """the global gradient norm the latest step saw, before clipping; inf / NaN on a skipped step (host synchronisation)"""
        return float(self._clip_state()[8:10].view(torch.float64)[0])

    def last_clip_coef(self):
        """the factor the latest step's gradients were multiplied by (host synchronisation)"""
        return float(self._clip_state()[6:7].view(torch.float32)[0])


class ExponentialMovingAverage(torch.nn.Module):
    """script_utils/utils.py:56-67 (torchvision-style EMA on AveragedModel, use_buffers=True): `module` is a deep copy of the
    model whose float parameters AND buffers follow avg = decay*avg + (1-decay)*value; the first update copies."""

    def __init__(self, model, decay, device="cpu"):
        super().__init__()
        self.module = copy.deepcopy(model)
        if device is not None:
            self.module = self.module.to(device)
        self.decay = float(decay)
        self.register_buffer("n_averaged", torch.tensor(0, dtype=torch.long, device=device))
        self._flat = None

    def forward(self, *args, **kwargs):
        return self.module(*args, **kwargs)

    def _pairs(self, model):
        a = list(self.module.parameters()) + list(self.module.buffers())
        b = list(model.parameters()) + list(model.buffers())
        return [(x, y) for x, y in zip(a, b)]

    @torch.no_grad()
    def update_parameters(self, model):
        L = _lib.lib()
        pairs = self._pairs(model)
        if int(self.n_averaged) == 0:
            for a, b in pairs:
                a.copy_(b.detach().to(a.device))
        else:
            npar = len(list(self.module.parameters()))
            par = [(a, b) for a, b in pairs[:npar] if a.dtype == torch.float32 and a.is_cuda]
            rest = [(a, b) for a, b in pairs if not any(a is x for x, _ in par)]
            st = current_stream_ptr(par[0][0].device)
            if self._flat is None:  # the EMA parameters live in one flat buffer with the same layout as optim.AdamW's
                flat, views = _flatten([a for a, _ in par], par[0][0].device)
                for (a, _), v in zip(par, views):
                    a.data = v
                self._flat = flat
            src = [b for _, b in par]
            contiguous = all(src[k].data_ptr() + ((src[k].numel() + 3) // 4 * 4) * 4 == src[k + 1].data_ptr() for k in range(len(src) - 1))
            if contiguous:  # one launch over all parameters
                check(L.eod_ema_update(ptr(self._flat), src[0].data_ptr(), self._flat.numel(), self.decay, st), "eod_ema_update")
            else:
                for a, b in par:
                    check(L.eod_ema_update(ptr(a), ptr(b.detach().contiguous()), a.numel(), self.decay, st), "eod_ema_update")
            for a, b in rest:  # buffers (use_buffers=True): the schedule tables etc.
                if a.dtype == torch.float32 and a.is_cuda and b.is_cuda:
                    check(L.eod_ema_update(ptr(a), ptr(b.detach().contiguous()), a.numel(), self.decay, st), "eod_ema_update")
                else:
                    a.copy_(b.detach().to(a.device))
            # the kernels wrote through raw pointers: advance torch's version counters so that the EMA copy's cached launch
            # program (packed conv / qkv / proj weights, keyed on (data_ptr, _version)) is rebuilt before its next forward
            for a, _ in pairs:
                if a.is_cuda and a.dtype == torch.float32:
                    torch.autograd.graph.increment_version(a)
        self.n_averaged += 1
