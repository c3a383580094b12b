"""The emulation of csrc/metrics.hip (eod_band_stats, eod_ssim) in torch float64 on the CPU, operation by operation in the order
include/eodiff.h documents: the affine (one multiply, one add), the products formed in double, the taps in ascending order with one rounded
multiply and one rounded add each, horizontal before vertical, the association of the map formula, the atan2 form of the spectral angle.
Element values are therefore bit-exact; only the ORDER of the big sums (pixels of a band, tiles of a plane) is not emulated -- the tests bound
a reordered float64 sum of n terms by n * 2^-53 * sum |terms|.  (torch's CPU float64 kernels round every elementwise operation once and
never contract a multiply into an add.)

quality_ref() holds the host formulas of metrics.quality written independently: straight from the definitions (centred moments, np.mean)
in numpy, not from raw sums."""
import math

import numpy as np
import torch

U = 2.0 ** -53


def gauss(kernel_size=11, sigma=1.5):
    d = np.arange((1 - kernel_size) / 2.0, (1 + kernel_size) / 2.0, 1.0)
    g = np.exp(-((d / sigma) ** 2) / 2.0)
    return g / g.sum()


def affine(x, a=1.0, b=0.0):
    return (a * x.double()) + b


def _pair(pred, ref, a, b):
    p = affine(pred, a, b)
    t = affine(ref, a, b).expand_as(p)
    return p, t


def counted(where, B, H, W):
    """bool [B, H, W]"""
    if where is None:
        return torch.ones(B, H, W, dtype=torch.bool)
    return (where != 0).expand(B, 1, H, W)[:, 0]


def blur(q, taps):
    """valid-region separable window sum of q [..., H, W]: horizontal, then vertical, taps ascending"""
    L = len(taps)
    Hv, Wv = q.shape[-2] - L + 1, q.shape[-1] - L + 1
    h = float(taps[0]) * q[..., :, 0:Wv]
    for k in range(1, L):
        h = h + float(taps[k]) * q[..., :, k:k + Wv]
    v = float(taps[0]) * h[..., 0:Hv, :]
    for k in range(1, L):
        v = v + float(taps[k]) * h[..., k:k + Hv, :]
    return v


def ssim_map(pred, ref, taps, c1, c2, a=1.0, b=0.0):
    """float64 [B, C, H - 2r, W - 2r]"""
    p, t = _pair(pred, ref, a, b)
    Ep, Et, Epp, Ett, Ept = blur(p, taps), blur(t, taps), blur(p * p, taps), blur(t * t, taps), blur(p * t, taps)
    mpp, mtt, mpt = Ep * Ep, Et * Et, Ep * Et
    spp, stt, spt = Epp - mpp, Ett - mtt, Ept - mpt
    return (((2.0 * mpt) + c1) * ((2.0 * spt) + c2)) / (((mpp + mtt) + c1) * ((spp + stt) + c2))


def ssim_sums(smap, where, r):
    """(sum [B, C], n [B, C], sum |ssim| [B, C]) over the positions whose centre is counted"""
    B, C, Hv, Wv = smap.shape
    on = counted(where, B, Hv + 2 * r, Wv + 2 * r)[:, r:r + Hv, r:r + Wv][:, None].expand(B, C, Hv, Wv)
    z = torch.where(on, smap, torch.zeros((), dtype=torch.float64))
    return z.sum((2, 3)), on.sum((2, 3)).double(), z.abs().sum((2, 3))


def ssim_mean(pred, ref, data_range=1.0, kernel_size=11, sigma=1.5, k1=0.01, k2=0.03, a=1.0, b=0.0):
    m = ssim_map(pred, ref, gauss(kernel_size, sigma), (k1 * data_range) ** 2, (k2 * data_range) ** 2, a, b)
    return float(m.reshape(m.shape[0], -1).mean(-1).mean())


def band_terms(pred, ref, a=1.0, b=0.0):
    """the seven per-pixel terms of the band sums, float64 [7, B, C, H, W]: 1, p, t, p*p, t*t, p*t, (p-t)*(p-t)"""
    p, t = _pair(pred, ref, a, b)
    d = p - t
    return torch.stack((torch.ones_like(p), p, t, p * p, t * t, p * t, d * d))


def band_stats(pred, ref, where=None, a=1.0, b=0.0):
    """(band [B, C, 8], bound [B, C, 8]): the float64 sums (torch's order) and max |p - t|; bound = n * 2^-53 * sum |terms| (0 for n and the max)"""
    B, C, H, W = pred.shape
    terms = band_terms(pred, ref, a, b)
    on = counted(where, B, H, W)[None, :, None].expand_as(terms)
    z = torch.where(on, terms, torch.zeros((), dtype=torch.float64))
    sums, mags = z.sum((3, 4)), z.abs().sum((3, 4))
    p, t = _pair(pred, ref, a, b)
    ad = torch.where(on[0], (p - t).abs(), torch.zeros((), dtype=torch.float64))
    nan = torch.isnan(ad).any(3).any(2)
    mx = torch.where(nan, torch.full((), math.nan, dtype=torch.float64), torch.nan_to_num(ad, nan=0.0).amax((2, 3)))
    band = torch.cat((sums.permute(1, 2, 0), mx[..., None]), 2)
    bound = torch.cat((sums[0][None] * U * mags, torch.zeros(1, B, C, dtype=torch.float64))).permute(1, 2, 0).clone()
    bound[..., 0] = 0.0
    return band, bound


def angles(pred, ref, a=1.0, b=0.0):
    """(theta [B, H, W] float64, defined [B, H, W] bool): the products summed over the bands in ascending order"""
    p, t = _pair(pred, ref, a, b)
    pp = torch.zeros_like(p[:, 0])
    tt, dot = pp.clone(), pp.clone()
    for c in range(p.shape[1]):
        pp = pp + p[:, c] * p[:, c]
        tt = tt + t[:, c] * t[:, c]
        dot = dot + p[:, c] * t[:, c]
    w = (pp * tt) - (dot * dot)
    w = torch.where(w > 0, w, torch.zeros((), dtype=torch.float64))
    return torch.atan2(torch.sqrt(w), dot), ~((pp == 0) | (tt == 0))


def sample_stats(pred, ref, where=None, a=1.0, b=0.0):
    """(sample [B, 3], bound [B]) -- bound of the angle sum: the reordering allowance plus 4 ulp per term for the device's atan2 / sqrt"""
    B, C, H, W = pred.shape
    th, ok = angles(pred, ref, a, b)
    on = counted(where, B, H, W)
    use = on & ok
    z = torch.where(use, th, torch.zeros((), dtype=torch.float64))
    n = use.sum((1, 2)).double()
    sample = torch.stack((z.sum((1, 2)), n, (on & ~ok).sum((1, 2)).double()), 1)
    return sample, (n * U + 8 * U) * z.abs().sum((1, 2))


def quality_ref(pred, ref, where=None, data_range=1.0, aff=(1.0, 0.0), ratio=None, kernel_size=11, sigma=1.5, k1=0.01, k2=0.03):
    """dict of numpy arrays with the fields of metrics.Quality, from the definitions"""
    B, C, H, W = pred.shape
    p, t = (x.numpy() for x in _pair(pred, ref, *aff))
    on = counted(where, B, H, W).numpy()
    th, ok = (x.numpy() for x in angles(pred, ref, *aff))
    out = {k: np.full((B, C), np.nan) for k in ("rmse", "bias", "max_abs", "psnr", "cc", "uiqi", "ssim")}
    out.update({k: np.full(B, np.nan) for k in ("n", "psnr_all", "sam_deg", "sam_undefined", "ssim_all")})
    out["ergas"] = None if ratio is None else np.full(B, np.nan)
    r = (kernel_size - 1) // 2
    smap = ssim_map(pred, ref, gauss(kernel_size, sigma), (k1 * data_range) ** 2, (k2 * data_range) ** 2, *aff).numpy()
    with np.errstate(divide="ignore", invalid="ignore"):
        for b in range(B):
            m = on[b]
            out["n"][b] = m.sum()
            out["sam_undefined"][b] = (m & ~ok[b]).sum()
            if not m.any():
                continue
            out["sam_deg"][b] = np.degrees(th[b][m & ok[b]].mean()) if (m & ok[b]).any() else np.nan
            mses, rel = [], []
            for c in range(C):
                x, y = p[b, c][m], t[b, c][m]
                d = x - y
                mse = np.mean(d * d)
                mses.append(mse)
                rel.append(mse / np.mean(y) ** 2)
                out["rmse"][b, c], out["bias"][b, c], out["max_abs"][b, c] = np.sqrt(mse), np.mean(d), np.abs(d).max()
                out["psnr"][b, c] = np.inf if mse == 0 else 10 * np.log10(data_range ** 2 / mse)
                xc, yc = x - x.mean(), y - y.mean()
                cov, vx, vy = np.mean(xc * yc), np.mean(xc * xc), np.mean(yc * yc)
                out["cc"][b, c] = cov / np.sqrt(vx * vy)
                out["uiqi"][b, c] = 4 * cov * x.mean() * y.mean() / ((vx + vy) * (x.mean() ** 2 + y.mean() ** 2))
                sm = smap[b, c][m[r:H - r, r:W - r]]
                out["ssim"][b, c] = sm.mean() if sm.size else np.nan
            mse_all = np.mean(mses)      # (every band counts the same pixels)
            out["psnr_all"][b] = np.inf if mse_all == 0 else 10 * np.log10(data_range ** 2 / mse_all)
            out["ssim_all"][b] = out["ssim"][b].mean()
            if ratio is not None:
                out["ergas"][b] = 100.0 / ratio * np.sqrt(np.mean(rel))
    return out
