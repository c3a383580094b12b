"""Host-only torch emulation of eod_dyn_threshold (include/eodiff.h): abs, torch.sort and the fp32 formula, every operation rounded once
in fp32, fmaxf / fminf NaN semantics (a NaN operand loses; torch.maximum would propagate it).  No GPU, no libeodiff.so."""
import math

import torch

MAX_N = 2 ** 31 - 1


def rank(q, n):
    """(k, frac): pos = q * (n - 1) in float64, k = floor(pos), frac = fp32(pos - k) as a Python float; where the fp32 rounding of
    pos - k reaches 1 the rank is k + 1 with frac 0 (frac lies in [0, 1))"""
    pos = float(q) * (n - 1)
    k = min(int(math.floor(pos)), n - 1)
    frac = float(torch.tensor(pos - k, dtype=torch.float64).to(torch.float32)) if pos > k else 0.0
    if frac >= 1.0:
        k, frac = k + 1, 0.0
    return k, frac


def fmaxf(a, b):
    return torch.where(torch.isnan(a), b, torch.where(torch.isnan(b), a, torch.maximum(a, b)))


def fminf(a, b):
    return torch.where(torch.isnan(a), b, torch.where(torch.isnan(b), a, torch.minimum(a, b)))


def keys(p):
    """bits(x) & 0x7fffffff as int64: |x| in the order the kernel ranks it (NaNs above +inf, by payload)"""
    return p.contiguous().view(torch.int32).to(torch.int64) & 0x7FFFFFFF


def quantile_value(p, k, frac):
    """v [B] of p [B, n] (fp32): lo + frac * (hi - lo) of the k-th and (k + 1)-th smallest keys"""
    B, n = p.shape
    srt = keys(p).sort(dim=1).values
    as_f32 = lambda z: z.to(torch.int32).view(torch.float32)
    lo, hi = as_f32(srt[:, k].contiguous()), as_f32(srt[:, min(k + 1, n - 1)].contiguous())
    if frac == 0.0:
        return lo
    return lo + torch.tensor(frac, dtype=torch.float32) * (hi - lo)


def threshold_kf(p, k, frac, cap=math.inf):
    """(out [B, n], s [B], v [B]) of p [B, n] fp32 on the CPU, from a given rank"""
    assert p.dtype == torch.float32 and p.dim() == 2 and p.device.type == "cpu"
    v = quantile_value(p, k, frac)
    s = fminf(fmaxf(v, torch.ones_like(v)), torch.full_like(v, cap))
    sh = s[:, None]
    out = fminf(fmaxf(p, -sh), sh) / sh
    return out, s, v


def threshold(p, q, cap=math.inf):
    """(out, s, v) of p [B, n] for the quantile q"""
    k, frac = rank(q, p.shape[1])
    return threshold_kf(p, k, frac, cap)


def threshold_image(x, q, cap=math.inf, per="sample"):
    """(out [B, C, H, W], s [B] or [B, C]) of a state on the CPU: per sample over C*H*W, or per channel over H*W"""
    B, C, H, W = x.shape
    flat = x.reshape(B * C, H * W) if per == "channel" else x.reshape(B, C * H * W)
    out, s, _ = threshold(flat.contiguous().float(), q, cap)
    return out.reshape(B, C, H, W), (s.reshape(B, C) if per == "channel" else s)
