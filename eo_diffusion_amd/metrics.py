"""Image-quality metrics on the GPU: what a sampled, inpainted or sharpened multi-band scene is scored with against
a truth, at the size it is produced.  The reference evaluates torchmetrics' PSNR and SSIM on the GPU inside its sampling script
(inference.py:136-138); harness.ssim / harness.psnr restate them for one saved batch (a host-side numpy SSIM, one pooled PSNR).  This module
adds the per-band view and the measures of the sharpening literature, from two operators (csrc/metrics.hip; include/eodiff.h states their
operations):

    eod_band_stats   one pass over both tensors: per (sample, band) n, the five raw moments, the squared error and max |p - t| in float64,
                     per sample the sum of the spectral angles atan2(sqrt(max(pp tt - dot^2, 0)), dot)
    eod_ssim         the SSIM map over the valid region (no padding: torchmetrics crops its reflect pad away again) in float64, and its
                     per-(sample, band) sum

pred [B, C, H, W]; ref [B or 1, C, H, W] (one truth against a stack of draws); where: None or [B or 1, 1, H, W], a pixel counts iff its
value is not 0 (hole_of(mask) for an inpainting); affine (a, b): both images become a * x + b on load ((0.5, 0.5) takes [-1, 1] samples to
[0, 1]: ERGAS and SAM need a reflectance-like range).  quality() makes one call of each operator and ONE device-to-host copy of the small
tables; everything after that is float64 numpy on the host.  A region without a counted pixel gives NaN, not an error.
"""
import ctypes
import math
import numbers

import numpy as np
import torch

from . import _lib
from ._lib import EodError
from .engine import current_stream_ptr, f32c, require_gpu

MAX_C = 32          # bands (the limit the PSF code has)
MAX_KERNEL = 25     # taps of the SSIM window (r <= 12)
NB, NS = 8, 3       # float64 values per (sample, band) and per sample of eod_band_stats


def gauss_window(kernel_size=11, sigma=1.5):
    """torchmetrics' 1-D Gaussian, exactly as harness._gauss_kernel builds it (float64)"""
    d = np.arange((1 - kernel_size) / 2.0, (1 + kernel_size) / 2.0, 1.0)
    g = np.exp(-((d / sigma) ** 2) / 2.0)
    return g / g.sum()


def _real(what, name, v, positive=False):
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(float(v)) or (positive and not float(v) > 0.0):
        raise EodError(f"{what}: {name} is a {'positive ' if positive else ''}finite number, got {v!r}")
    return float(v)


def _affine(what, affine):
    try:
        a, b = affine
    except (TypeError, ValueError):
        raise EodError(f"{what}: affine is a pair (a, b), got {affine!r}") from None
    return _real(what, "affine[0]", a), _real(what, "affine[1]", b)


def _window(what, kernel_size, sigma):
    if isinstance(kernel_size, bool) or not isinstance(kernel_size, numbers.Integral) or kernel_size < 1 or kernel_size % 2 == 0 or kernel_size > MAX_KERNEL:
        raise EodError(f"{what}: kernel_size is an odd integer in 1 .. {MAX_KERNEL}, got {kernel_size!r}")
    _real(what, "sigma", sigma, positive=True)
    return np.ascontiguousarray(gauss_window(int(kernel_size), float(sigma)), dtype=np.float64)


def _shapes(what, pred, ref, where, kernel_size=1):
    """every refusal that needs no GPU; returns (B, C, H, W)"""
    for name, t in (("pred", pred), ("ref", ref)):
        if not torch.is_tensor(t) or t.dim() != 4:
            raise EodError(f"{what}: {name} must be a tensor [B, C, H, W]")
    B, C, H, W = (int(s) for s in pred.shape)
    if B < 1 or H < 1 or W < 1:
        raise EodError(f"{what}: pred must not be empty, got {tuple(pred.shape)}")
    if not 1 <= C <= MAX_C:
        raise EodError(f"{what}: 1 .. {MAX_C} bands, pred has {C}")
    if tuple(ref.shape[1:]) != (C, H, W) or int(ref.shape[0]) not in (1, B):
        raise EodError(f"{what}: ref must be [{B} or 1, {C}, {H}, {W}], got {tuple(ref.shape)}")
    if where is not None:
        if not torch.is_tensor(where) or where.dim() != 4 or tuple(where.shape[1:]) != (1, H, W) or int(where.shape[0]) not in (1, B):
            raise EodError(f"{what}: where must be None or a tensor [{B} or 1, 1, {H}, {W}], got {tuple(getattr(where, 'shape', ()))}")
    if H < kernel_size or W < kernel_size:
        raise EodError(f"{what}: a {H} x {W} image is smaller than the {kernel_size}-tap window")
    return B, C, H, W


def _gpu(what, pred, ref, where):
    require_gpu(pred, what)
    require_gpu(ref, what)
    if where is not None:
        require_gpu(where, what)
    if ref.device != pred.device or (where is not None and where.device != pred.device):
        raise EodError(f"{what}: pred, ref and where must be on one device")
    return f32c(pred), f32c(ref), None if where is None else f32c(where)


def hole_of(mask):
    """The `where` of an inpainting: 1.0 where the RePaint mask is not exactly 1 (the rule of skip_known: NaN and soft values are painted),
    0.0 where the pixel is known.  mask [B, 1, H, W] (or [B, H, W] / [H, W]) -> float32 [B, 1, H, W] on the mask's device."""
    if not torch.is_tensor(mask) or mask.dim() not in (2, 3, 4):
        raise EodError("hole_of: mask must be a tensor [B, 1, H, W], [B, H, W] or [H, W]")
    m = mask if mask.dim() == 4 else (mask[:, None] if mask.dim() == 3 else mask[None, None])
    if m.shape[1] != 1:
        raise EodError(f"hole_of: the mask has one channel, got {tuple(mask.shape)}")
    return (m != 1).to(torch.float32)


def _band_stats(what, p, t, w, a, b, out):
    """out: float64 device tensor of B * (C * NB + NS) values: the band table, then the sample table"""
    B, C, H, W = p.shape
    L = _lib.lib()
    ws = torch.empty(int(L.eod_band_stats_workspace_size(B, C, H, W)), dtype=torch.uint8, device=p.device)
    band, sample = out[:B * C * NB], out[B * C * NB:]
    _lib.check(L.eod_band_stats(p.data_ptr(), t.data_ptr(), _lib.ptr(w), B, t.shape[0], 1 if w is None else w.shape[0], C, H, W, a, b,
                                band.data_ptr(), sample.data_ptr(), ws.data_ptr(), ws.numel(), current_stream_ptr(p.device)), "eod_band_stats")
    return band.view(B, C, NB), sample.view(B, NS)


def _ssim(what, p, t, w, a, b, taps, c1, c2, sums, want_map):
    B, C, H, W = p.shape
    r = (taps.size - 1) // 2
    L = _lib.lib()
    ws = torch.empty(int(L.eod_ssim_workspace_size(B, C, H, W, r)), dtype=torch.uint8, device=p.device)
    full = torch.full((B, C, H, W), float("nan"), dtype=torch.float32, device=p.device) if want_map else None
    _lib.check(L.eod_ssim(p.data_ptr(), t.data_ptr(), _lib.ptr(w), B, t.shape[0], 1 if w is None else w.shape[0], C, H, W,
                          taps.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), r, a, b, c1, c2, _lib.ptr(full), sums.data_ptr(), ws.data_ptr(),
                          ws.numel(), current_stream_ptr(p.device)), "eod_ssim")
    return None if full is None else full[:, :, r:H - r, r:W - r]


def band_stats(pred, ref, where=None, affine=(1.0, 0.0)):
    """The device tables of eod_band_stats: (band [B, C, 8], sample [B, 3]), float64.  band[b, c] = n, sum p, sum t, sum p^2, sum t^2,
    sum p t, sum (p - t)^2, max |p - t| over the counted pixels; sample[b] = sum of the spectral angles (radians), pixels that have one,
    pixels that have none (a zero spectrum on either side).  Reading them is the caller's synchronisation."""
    what = "band_stats"
    B, C, H, W = _shapes(what, pred, ref, where)
    a, b = _affine(what, affine)
    p, t, w = _gpu(what, pred, ref, where)
    out = torch.empty(B * (C * NB + NS), dtype=torch.float64, device=p.device)
    return _band_stats(what, p, t, w, a, b, out)


class Quality:
    """What quality() returns: numpy arrays (float64), see the table in DESIGN.md section 9.13.  ergas is None without `ratio`, ssim and
    ssim_all are None with ssim=False."""
    FIELDS = ("n", "rmse", "bias", "max_abs", "psnr", "psnr_all", "cc", "uiqi", "sam_deg", "sam_undefined", "ergas", "ssim", "ssim_all")

    def __init__(self, **kw):
        for f in self.FIELDS:
            setattr(self, f, kw[f])

    def __repr__(self):
        return "Quality(" + ", ".join(f"{f}={getattr(self, f)!r}" for f in self.FIELDS) + ")"


def _derive(band, sample, ssim_sums, data_range, ratio):
    """the float64 host arithmetic of quality(): band [B, C, 8], sample [B, 3], ssim_sums [B, C, 2] or None (numpy)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        n, sp, st, spp, stt, spt, sdd, mx = (band[..., i] for i in range(NB))
        mse = sdd / n
        mp, mt = sp / n, st / n
        vp, vt, cov = spp / n - mp * mp, stt / n - mt * mt, spt / n - mp * mt
        psnr = np.where(mse == 0.0, np.inf, 10.0 * np.log10(data_range * data_range / mse))
        mse_all = sdd.sum(1) / n.sum(1)
        psnr_all = np.where(mse_all == 0.0, np.inf, 10.0 * np.log10(data_range * data_range / mse_all))
        ergas = None if ratio is None else 100.0 / ratio * np.sqrt((mse / (mt * mt)).mean(1))
        ssim = None if ssim_sums is None else ssim_sums[..., 0] / ssim_sums[..., 1]
        return Quality(n=n[:, 0].copy(), rmse=np.sqrt(mse), bias=(sp - st) / n, max_abs=np.where(n == 0.0, np.nan, mx), psnr=psnr, psnr_all=psnr_all,
                       cc=cov / np.sqrt(vp * vt), uiqi=4.0 * cov * mp * mt / ((vp + vt) * (mp * mp + mt * mt)),
                       sam_deg=np.degrees(sample[:, 0] / sample[:, 1]), sam_undefined=sample[:, 2].copy(), ergas=ergas,
                       ssim=ssim, ssim_all=None if ssim is None else ssim.mean(1))


def describe(q, title="quality", member=0):
    """member `member` of a Quality as a few lines of text (what the examples print under --metrics)"""
    row = lambda a, fmt: ", ".join(format(float(v), fmt) for v in a)
    lines = [f"{title}: {int(q.n[member])} pixels; PSNR {q.psnr_all[member]:.2f} dB over all bands"
             + (f", SSIM {q.ssim_all[member]:.4f}" if q.ssim_all is not None else "") + f", SAM {q.sam_deg[member]:.3f} deg"
             + (f" ({int(q.sam_undefined[member])} pixels without an angle)" if q.sam_undefined[member] else "")
             + (f", ERGAS {q.ergas[member]:.3f}" if q.ergas is not None else ""),
             f"  per band: RMSE {row(q.rmse[member], '.4f')}", f"            bias {row(q.bias[member], '+.4f')}",
             f"            PSNR {row(q.psnr[member], '.2f')}", f"            CC   {row(q.cc[member], '.4f')}",
             f"            UIQI {row(q.uiqi[member], '.4f')}"]
    if q.ssim is not None:
        lines.append(f"            SSIM {row(q.ssim[member], '.4f')}")
    return "\n".join(lines)


def quality(pred, ref, *, where=None, data_range=1.0, affine=(1.0, 0.0), ratio=None, ssim=True, kernel_size=11, sigma=1.5, k1=0.01, k2=0.03):
    """Every metric of one prediction (or a stack) against a truth, per band where that means something: a Quality of numpy arrays.
    data_range is the range AFTER the affine; ratio the resolution ratio of ERGAS (2 for 20 m bands against 10 m), None: no ERGAS."""
    what = "quality"
    taps = _window(what, kernel_size, sigma) if ssim else None
    B, C, H, W = _shapes(what, pred, ref, where, kernel_size if ssim else 1)
    a, b = _affine(what, affine)
    data_range = _real(what, "data_range", data_range, positive=True)
    if ratio is not None:
        ratio = _real(what, "ratio", ratio, positive=True)
    k1, k2 = _real(what, "k1", k1), _real(what, "k2", k2)
    p, t, w = _gpu(what, pred, ref, where)
    nb = B * (C * NB + NS)
    out = torch.empty(nb + (B * C * 2 if ssim else 0), dtype=torch.float64, device=p.device)
    _band_stats(what, p, t, w, a, b, out[:nb])
    if ssim:
        _ssim(what, p, t, w, a, b, taps, (k1 * data_range) ** 2, (k2 * data_range) ** 2, out[nb:], False)
    host = out.cpu().numpy()      # the one device-to-host copy (and the synchronisation)
    return _derive(host[:B * C * NB].reshape(B, C, NB), host[B * C * NB:nb].reshape(B, NS), host[nb:].reshape(B, C, 2) if ssim else None, data_range, ratio)


def ssim(pred, ref, data_range=1.0, kernel_size=11, sigma=1.5, k1=0.01, k2=0.03, *, where=None, affine=(1.0, 0.0), return_map=False):
    """harness.ssim on the GPU (positionally compatible): the mean over pixels, then bands, then batch.  return_map=True: (mean, map), the
    map [B, C, H - 2r, W - 2r] fp32 on the device."""
    what = "ssim"
    taps = _window(what, kernel_size, sigma)
    B, C, H, W = _shapes(what, pred, ref, where, kernel_size)
    a, b = _affine(what, affine)
    data_range = _real(what, "data_range", data_range, positive=True)
    k1, k2 = _real(what, "k1", k1), _real(what, "k2", k2)
    p, t, w = _gpu(what, pred, ref, where)
    sums = torch.empty(B * C * 2, dtype=torch.float64, device=p.device)
    smap = _ssim(what, p, t, w, a, b, taps, (k1 * data_range) ** 2, (k2 * data_range) ** 2, sums, bool(return_map))
    s = sums.cpu().numpy().reshape(B, C, 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = float((s[..., 0] / s[..., 1]).mean(1).mean())
    return (mean, smap) if return_map else mean


def psnr(pred, ref, data_range=1.0, *, where=None, affine=(1.0, 0.0)):
    """harness.psnr from float64 sums: 10 log10(data_range^2 / mse), the squared error pooled over all bands and all members, like
    torchmetrics' default.  inf at mse 0, NaN where nothing is counted."""
    what = "psnr"
    data_range = _real(what, "data_range", data_range, positive=True)
    band, _ = band_stats(pred, ref, where, affine)
    s = band.cpu().numpy()
    n, sdd = s[..., 0].sum(), s[..., 6].sum()
    if n == 0.0:
        return float("nan")
    mse = sdd / n
    return float("inf") if mse == 0.0 else float(10.0 * np.log10(data_range * data_range / mse))


# ---------------------------------------------------------------------------------------------------------------- the ensemble as a whole
MAX_MEMBERS = 64    # members of a stack (csrc/ensemble_body.h: ENS_MAXB)
MAX_LEVELS = 4      # central intervals of one eod_ensemble_stats call
ENS_NV = 5          # float64 sums per band of eod_ensemble_stats


class Ensemble:
    """What ensemble() returns: numpy arrays (float64), per band [C] unless noted; see the table in DESIGN.md section 9.14.  rank_hist is
    [C, B + 1] (counts), coverage [C, L] (fractions), levels [L]."""
    FIELDS = ("n", "crps", "crps_fair", "mae_members", "rmse_mean", "bias_mean", "spread", "spread_skill", "rank_hist", "reliability_index",
              "ties", "coverage", "levels")

    def __init__(self, **kw):
        for f in self.FIELDS:
            setattr(self, f, kw[f])

    def __repr__(self):
        return "Ensemble(" + ", ".join(f"{f}={getattr(self, f)!r}" for f in self.FIELDS) + ")"


def _levels(what, levels, members):
    """the central intervals as ranks: level p -> the quantiles (1 - p) / 2 and (1 + p) / 2 by tiling.quantile_ranks"""
    from .tiling import quantile_ranks
    try:
        lv = list(levels)
    except TypeError:
        raise EodError(f"{what}: levels is a sequence of numbers in [0, 1], got {levels!r}") from None
    if len(lv) > MAX_LEVELS:
        raise EodError(f"{what}: at most {MAX_LEVELS} levels per call, got {len(lv)}")
    for p in lv:
        if isinstance(p, bool) or not isinstance(p, numbers.Real) or not 0.0 <= float(p) <= 1.0:
            raise EodError(f"{what}: every level is a number in [0, 1], got {p!r}")
    lv = [float(p) for p in lv]
    lo = quantile_ranks(what, [(1.0 - p) / 2.0 for p in lv], members)
    hi = quantile_ranks(what, [(1.0 + p) / 2.0 for p in lv], members)
    return lv, lo, hi


def _derive_ensemble(sums, counts, B, levels):
    """the float64 host arithmetic of ensemble(): sums [C, 5], counts [C, 2 + (B + 1) + L] (numpy)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        cnt = counts.astype(np.float64)
        n = cnt[:, 0]
        hist = cnt[:, 2:2 + B + 1]
        a, g, se, s2, e = (sums[:, i] / n for i in range(ENS_NV))
        rmse, spread = np.sqrt(se), np.sqrt(s2)
        fair = a - g * (B / (B - 1.0)) if B > 1 else np.full_like(a, np.nan)
        return Ensemble(n=n.copy(), crps=a - g, crps_fair=fair, mae_members=a, rmse_mean=rmse, bias_mean=e, spread=spread,
                        spread_skill=math.sqrt((B + 1.0) / B) * spread / rmse, rank_hist=hist.copy(),
                        reliability_index=np.abs(hist / n[:, None] - 1.0 / (B + 1)).sum(1), ties=cnt[:, 1].copy(),
                        coverage=cnt[:, 2 + B + 1:] / n[:, None], levels=np.asarray(levels, dtype=np.float64))


def ensemble(draws, ref, *, where=None, levels=(0.5, 0.9), return_map=False):
    """The verification of an ensemble against a truth: draws [B, C, H, W] (B <= 64 draws of one scene), ref [1, C, H, W], where None or
    [1, 1, H, W] (a pixel counts iff its value is not 0: hole_of(mask) for an inpainting) -> an Ensemble of numpy arrays per band, after one
    call of eod_ensemble_stats and ONE device-to-host copy; with return_map=True: (Ensemble, CRPS map [1, C, H, W] fp32 on the device, NaN
    where the pixel is not counted).  quality() scores members one at a time; whether their SPREAD is calibrated needs the sorted members
    of every pixel:

        crps               mean over the pixels of  E|X - y| - 1/2 E|X - X'|  over the B members (both expectations with divisor B resp. B^2)
        crps_fair          the same with E|X - X'| over the B (B - 1) pairs of different members (Ferro 2014); NaN at B = 1
        mae_members        mean of E|X - y|: the first term alone, so crps <= mae_members
        rmse_mean, bias_mean   of the ensemble mean
        spread             sqrt(mean of the per-pixel sample variance, divisor B - 1)
        spread_skill       sqrt((B + 1) / B) * spread / rmse_mean: 1 for a calibrated ensemble
        rank_hist          [C, B + 1]: how many pixels have exactly r members below the truth (Talagrand); flat when calibrated
        reliability_index  sum over r of |rank_hist_r / n - 1 / (B + 1)|
        ties               pixels at which some member equals the truth
        coverage           [C, L]: the fraction of pixels with q_((1-p)/2) <= y <= q_((1+p)/2), the quantiles of scene_quantiles, per level p

    Ties: the rank counts STRICT inequalities (members below the truth, in the total order -0.0 < +0.0 < .. < NaN) and ties are reported,
    not randomised.  The known pixels of an inpainting are all ties -- every draw equals the truth there -- and pile up in rank 0: exclude
    them with where=hole_of(mask).  There is no `affine`: every float measure is positively homogeneous (crps(a x + b, a y + b) = a crps(x, y)
    for a > 0; bias likewise) and the counts do not change, so rescale the result.  A region without a counted pixel gives NaN, not an
    error."""
    what = "ensemble"
    B, C, H, W = _shapes(what, draws, ref, where)
    if B > MAX_MEMBERS:
        raise EodError(f"{what}: at most {MAX_MEMBERS} members are sorted per pixel, draws has {B}")
    if int(ref.shape[0]) != 1 or (where is not None and int(where.shape[0]) != 1):
        raise EodError(f"{what}: one truth [1, {C}, {H}, {W}] and one where [1, 1, {H}, {W}] for the whole ensemble, got {tuple(ref.shape)}"
                       + ("" if where is None else f" and {tuple(where.shape)}"))
    lv, lo, hi = _levels(what, levels, B)
    p, t, w = _gpu(what, draws, ref, where)
    L, nl = _lib.lib(), len(lv)
    nc = 2 + B + 1 + nl
    ws = torch.empty(int(L.eod_ensemble_stats_workspace_size(B, C, H, W)), dtype=torch.uint8, device=p.device)
    out = torch.empty(C * (ENS_NV + nc), dtype=torch.float64, device=p.device)      # the sums, then the counts (int64 in the same buffer)
    sums, counts = out[:C * ENS_NV], out[C * ENS_NV:].view(torch.int64)
    cmap = torch.empty((1, C, H, W), dtype=torch.float32, device=p.device) if return_map else None
    lk = (ctypes.c_int32 * max(2 * nl, 1))(*[k for pair in zip(lo, hi) for k, _ in pair])
    lf = (ctypes.c_float * max(2 * nl, 1))(*[f for pair in zip(lo, hi) for _, f in pair])
    _lib.check(L.eod_ensemble_stats(p.data_ptr(), t.data_ptr(), _lib.ptr(w), B, C, H, W, lk, lf, nl, sums.data_ptr(), counts.data_ptr(),
                                    _lib.ptr(cmap), ws.data_ptr(), ws.numel(), current_stream_ptr(p.device)), "eod_ensemble_stats")
    host = out.cpu().numpy()      # the one device-to-host copy (and the synchronisation)
    e = _derive_ensemble(host[:C * ENS_NV].reshape(C, ENS_NV), host[C * ENS_NV:].view(np.int64).reshape(C, nc), B, lv)
    return (e, cmap) if return_map else e


def describe_ensemble(e, title="ensemble"):
    """an Ensemble as a few lines of text (what examples/inpaint_scene.py prints under --metrics with --draws K)"""
    row = lambda a, fmt: ", ".join(format(float(v), fmt) for v in a)
    B = e.rank_hist.shape[1] - 1
    lines = [f"{title}: {B} members, {int(e.n[0]) if len(e.n) else 0} pixels per band",
             f"  per band: CRPS {row(e.crps, '.4f')} (fair {row(e.crps_fair, '.4f')}; members' MAE {row(e.mae_members, '.4f')})",
             f"            RMSE of the mean {row(e.rmse_mean, '.4f')}, bias {row(e.bias_mean, '+.4f')}",
             f"            spread {row(e.spread, '.4f')}, spread / skill {row(e.spread_skill, '.3f')}",
             f"            rank histogram off flat by {row(e.reliability_index, '.3f')}, ties {row(e.ties, '.0f')}"]
    for i, p in enumerate(e.levels):
        lines.append(f"            {100 * p:.0f} % interval covers {row(100 * e.coverage[:, i], '.1f')} %")
    return "\n".join(lines)
