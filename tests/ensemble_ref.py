"""Emulations of the ensemble statistics (csrc/ensemble.hip; include/eodiff.h states the operations): the order-preserving keys and their
sort by numpy on the integers, the quantile in numpy fp32 operation by operation, the per-pixel float64 quantities in the stated order
(vectorised over the pixels, sequential over the members), and the band sums by math.fsum together with sum |terms| for the bound of a
reordered sum.  Arrays are numpy; the tests convert."""
import math

import numpy as np

TOP = np.uint32(0xFFFFFFFF)
NV = 5


def keys(x):
    """float32 array -> uint32 keys: -inf < .. < -0.0 < +0.0 < .. < +inf < NaN (every NaN the top key)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32)
    k = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(x), TOP, k).astype(np.uint32)


def unkeys(k):
    """uint32 keys -> the floats they came from; the top key gives the quiet NaN 0x7fc00000"""
    k = np.ascontiguousarray(k, dtype=np.uint32)
    u = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    u = np.where(k == TOP, np.uint32(0x7FC00000), u).astype(np.uint32)
    return u.view(np.float32)


def sorted_keys(x):
    """x [B, ...] float32 -> the keys sorted along axis 0"""
    return np.sort(keys(x), axis=0)


def quantile_of_sorted(xs, k, frac):
    """xs [B, ...] float32, sorted along axis 0 -> the quantile (k, frac): x_(k) itself at frac == 0, else d = hi - lo, m = frac * d,
    v = lo + m, each a float32 operation"""
    lo = xs[k]
    if frac == 0.0:
        return lo.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        hi = xs[k + 1]
        d = (hi - lo).astype(np.float32)
        m = (np.float32(frac) * d).astype(np.float32)
        return (lo + m).astype(np.float32)


def scene_quantiles(x, ranks):
    """x [B, n] float32, ranks [(k, frac)] -> [Q, n] float32"""
    xs = unkeys(sorted_keys(x))
    return np.stack([quantile_of_sorted(xs, k, f) for k, f in ranks])


def pixel_terms(x, y, levels=()):
    """x [B, n] float32 (one band's members), y [n] float32, levels [((k_lo, f_lo), (k_hi, f_hi))] -> dict of per-pixel arrays:
    terms [n, 5] float64 (a / B, g / (B B), (m - y)^2, s2, m - y), crps [n] float64, rank [n], tie [n], covered [L, n]"""
    B, n = x.shape
    ks = sorted_keys(x)
    xs32 = unkeys(ks)
    xs = xs32.astype(np.float64)
    yd = np.asarray(y, dtype=np.float32).astype(np.float64)
    yk = keys(y)
    with np.errstate(invalid="ignore", over="ignore"):
        a, g, s = np.zeros(n), np.zeros(n), np.zeros(n)
        for i in range(B):
            ad = np.abs(xs[i] - yd)
            gx = float(2 * i - B + 1) * xs[i]
            a = a + ad
            g = g + gx
            s = s + xs[i]
        m = s / float(B)
        ss = np.zeros(n)
        for i in range(B):
            d = xs[i] - m
            ss = ss + d * d
        s2 = ss / float(B - 1) if B > 1 else np.zeros(n)
        t1, t2 = a / float(B), g / (float(B) * float(B))
        e = m - yd
        y32 = np.asarray(y, dtype=np.float32)
        cov = [(quantile_of_sorted(xs32, *lo) <= y32) & (y32 <= quantile_of_sorted(xs32, *hi)) for lo, hi in levels]
        return dict(terms=np.stack([t1, t2, e * e, s2, e], axis=1), crps=t1 - t2, rank=(ks < yk[None]).sum(0), tie=(ks == yk[None]).any(0),
                    covered=np.stack(cov) if cov else np.zeros((0, n), dtype=bool))


def ensemble_stats(x, y, where=None, levels=()):
    """x [B, C, H, W], y [C, H, W], where [H, W] or None (float32 numpy) -> (sums [C, 5] by fsum, mag [C, 5] = sum |terms|,
    counts [C, 2 + B + 1 + L] int64, crps_map [C, H, W] float32 with NaN at pixels that are not counted)"""
    B, C, H, W = x.shape
    L = len(levels)
    on = np.ones(H * W, dtype=bool) if where is None else (np.asarray(where, dtype=np.float32).reshape(-1) != 0)
    sums, mag = np.zeros((C, NV)), np.zeros((C, NV))
    counts = np.zeros((C, 2 + B + 1 + L), dtype=np.int64)
    cmap = np.full((C, H * W), np.nan, dtype=np.float32)
    for c in range(C):
        if not on.any():
            continue
        p = pixel_terms(x[:, c].reshape(B, -1)[:, on], y[c].reshape(-1)[on], levels)
        for v in range(NV):
            col = p["terms"][:, v]
            sums[c, v] = math.fsum(col) if np.isfinite(col).all() else col.sum()
            mag[c, v] = math.fsum(np.abs(col)) if np.isfinite(col).all() else np.abs(col).sum()
        counts[c, 0] = int(on.sum())
        counts[c, 1] = int(p["tie"].sum())
        counts[c, 2:2 + B + 1] = np.bincount(p["rank"], minlength=B + 1)
        counts[c, 2 + B + 1:] = p["covered"].sum(1)
        with np.errstate(invalid="ignore", over="ignore"):
            cmap[c, on] = p["crps"].astype(np.float32)
    return sums, mag, counts, cmap.reshape(C, H, W)


def crps_brute(x, y):
    """E|X - y| - 1/2 E|X - X'| over the members of one pixel by the double loop (x [B], y scalar; float64)"""
    x = [float(v) for v in x]
    B = len(x)
    first = math.fsum(abs(v - float(y)) for v in x) / B
    second = math.fsum(abs(u - v) for u in x for v in x) / (B * B)
    return first - 0.5 * second
