"""Host side of tests/test_gpu_big_index.py (test infrastructure, numpy only: no GPU, no libeodiff.so): where the reference windows of a
tensor of more than 2^31 elements lie, how such a tensor is cut into the views of the whole-tensor comparison, the constructed multiset
of the threshold's order statistic, and the blend of a band of scene rows from the tiles that cover it.

  OFFSETS             the element offsets a narrow index breaks at: 2^29 (a signed 32-bit BYTE offset), 2^30 (an unsigned one), 2^31 (a
                      signed 32-bit ELEMENT index)
  windows             [lo, hi) element ranges: the first and the last 64 Ki, +-32 Ki around each offset inside the tensor, and +-32 Ki
                      around the multiples of each `unit` (sample, scene, plane) on both sides of each of those (the nearest is one of them)
  cut_at              the same ranges cut at the multiples of a unit, so that a piece lies in one sample / plane
  chunks              [lo, hi) ranges of at most 2^26 elements that tile [0, numel)
  row_bands           the same scheme for plane operators: bands of whole rows [ya, yb) of plane (b, c) of a [B][C][H][W] tensor
  multiset_x          x_i = +-((i a mod M) + 1) 2^-22 scale: every magnitude occurs n / M times, so the order statistics have a closed form
  multiset_order_stat a_(k) of it
  blend_band          tests/test_gpu_scene.py blend_emulated restricted to a band of rows: w = wy * wx, p = w * e, left to right over the
                      covering tiles in ascending (iy, ix), every operation one fp32 rounding
tests/test_big_index_ref.py checks each of them on the CPU."""
import numpy as np

OFFSETS = (2 ** 29, 2 ** 30, 2 ** 31)
EDGE, HALF = 65536, 32768
CHUNK = 2 ** 26
F = np.float32


def _merge(spans):
    out = []
    for lo, hi in sorted(s for s in spans if s[1] > s[0]):
        if out and lo <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], hi))
        else:
            out.append((lo, hi))
    return out


def anchors(numel):
    """the element offsets the windows are placed at: the start, each of OFFSETS inside the tensor, the end"""
    return [0] + [o for o in OFFSETS if o < numel] + [numel]


def windows(numel, units=()):
    numel = int(numel)
    spans = [(0, min(EDGE, numel)), (max(0, numel - EDGE), numel)]
    at = [o for o in OFFSETS if o < numel]
    for u in units:
        u = int(u)
        for a in anchors(numel):
            at += [b for b in ((a // u) * u, -(-a // u) * u) if 0 < b < numel]       # the multiples of u on both sides of a
    spans += [(max(0, o - HALF), min(numel, o + HALF)) for o in at]
    return _merge(spans)


def cut_at(spans, unit):
    unit = int(unit)
    out = []
    for lo, hi in spans:
        while lo < hi:
            nxt = min(hi, (lo // unit + 1) * unit)
            out.append((lo, nxt))
            lo = nxt
    return out


def chunks(numel, size=CHUNK, unit=None):
    """[lo, hi) of at most `size` elements tiling [0, numel); with a unit, no chunk crosses a multiple of it"""
    spans = [(lo, min(lo + size, int(numel))) for lo in range(0, int(numel), int(size))]
    return cut_at(spans, unit) if unit else spans


def row_bands(B, C, H, W, rows=4, align=None):
    """(b, c, ya, yb): bands of `rows` whole rows of one plane, at the first and the last rows of the tensor, on both sides of each of
    OFFSETS, and on both sides of the plane and the scene boundaries below and above each of those.  align: the bands start at multiples
    of it (block operators: rows and H are multiples of the block size)"""
    hw, numel = H * W, B * C * H * W
    rows_of = set()
    at = list(anchors(numel))
    for u in (hw, C * hw):
        at += [b for a in anchors(numel) for b in ((a // u) * u, -(-a // u) * u)]
    for a in at:
        for e in (a - 1, a):                                 # the element before and the element at the offset
            if 0 <= e < numel:
                r = e // W                                   # the global row (b * C + c) * H + y
                p, y = divmod(r, H)
                ya = (y // align) * align if align else min(max(y - rows // 2, 0), H - rows)
                rows_of.add((p // C, p % C, ya, ya + rows))
    return sorted(rows_of)


# ------------------------------------------------------------------------------------------------ the threshold's multiset
def multiset_x(i, a, M, scale=1.0):
    """x_i of the constructed multiset for the int64 element numbers i: |x_i| = ((i a mod M) + 1) 2^-22 scale, the sign alternating per
    block of M elements.  a odd and M a power of two: i -> i a mod M is a bijection of every block of M, so with n = M R every magnitude
    occurs exactly R times.  Exact in fp32 for M <= 2^24 and a scale that is a power of two"""
    i = np.asarray(i, np.int64)
    mag = (((i * np.int64(a)) % np.int64(M)) + 1).astype(F) * F(2.0 ** -22) * F(scale)
    return np.where((i // np.int64(M)) % 2 == 0, mag, -mag).astype(F)


def multiset_order_stat(k, R, scale=1.0):
    """a_(k), k from 0, of the n = M R magnitudes: each of 1 .. M (times 2^-22 scale) occurs R times"""
    return F(int(k) // int(R) + 1) * F(2.0 ** -22) * F(scale)


def multiset_scale(k, frac, R, M, scale=1.0, cap=np.inf):
    """(s, v) of eod_dyn_threshold on the multiset: v = lo + frac * (hi - lo) in fp32, s = min(max(v, 1), cap)"""
    n = int(M) * int(R)
    lo, hi = multiset_order_stat(k, R, scale), multiset_order_stat(min(k + 1, n - 1), R, scale)
    v = lo if frac == 0.0 else F(lo + F(F(frac) * F(hi - lo)))
    return F(min(max(v, F(1.0)), F(cap))), v


def threshold_apply(x, s):
    """out = clamp(x, -s, s) / s, fp32 (finite x)"""
    s = F(s)
    return (np.minimum(np.maximum(np.asarray(x, F), -s), s) / s).astype(F)


# ------------------------------------------------------------------------------------------------ the blend of a band of rows
def blend_band(rows_of, oy, ox, wy, wx, s, W, ya, yb):
    """rows [ya, yb) x [0, W) of one plane of the blended scene.  rows_of(iy, ix, d0, d1) -> float32 [d1 - d0][s]: rows d0 .. d1 of the
    tile (iy, ix) of that plane.  A pixel no tile covers stays NaN (the full plan's kernel writes NaN there)"""
    acc = np.full((yb - ya, W), np.nan, F)
    seen = np.zeros((yb - ya, W), bool)
    for iy in range(len(oy)):
        y0 = max(ya, int(oy[iy])), min(yb, int(oy[iy]) + s)
        if y0[0] >= y0[1]:
            continue
        d0, d1 = y0[0] - int(oy[iy]), y0[1] - int(oy[iy])
        for ix in range(len(ox)):
            x0 = int(ox[ix])
            w = np.asarray(wy[iy], F)[d0:d1, None] * np.asarray(wx[ix], F)[None, :]
            p = w * np.asarray(rows_of(iy, ix, d0, d1), F)
            reg = (slice(y0[0] - ya, y0[1] - ya), slice(x0, x0 + s))
            acc[reg] = np.where(seen[reg], acc[reg] + p, p)
            seen[reg] = True
    return acc


def tiles_covering(o, s, lo, hi):
    """the indices i of an axis whose window [o[i], o[i] + s) meets [lo, hi)"""
    return [i for i in range(len(o)) if int(o[i]) < hi and int(o[i]) + s > lo]


# ------------------------------------------------------------------------------------------------ Philox on a window of quads
def philox_uniforms_at(q_lo, q_hi, seed, sample, step, stream_id):
    """(u_r, u_a) [1, q_hi - q_lo, 2] float32 of the quads q_lo .. q_hi - 1 of one sample: tests/sampler_edge_ref.py philox_uniforms for a
    range of quads that need not start at 0 (oracle/philox_ref.py's own rounds; the quad number is 64-bit, its high word goes to c3)"""
    from oracle import philox_ref as PR
    q = np.arange(int(q_lo), int(q_hi), dtype=np.uint64)
    n = q.size
    c0, c1, c2, c3 = PR._philox(q.astype(np.uint32), np.full(n, sample & 0xFFFFFFFF, np.uint32), np.full(n, step & 0xFFFFFFFF, np.uint32),
                                np.uint32(stream_id & 0xFFFFFFFF) ^ (q >> np.uint64(32)).astype(np.uint32),
                                seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    ur, ua = np.zeros((1, n, 2), F), np.zeros((1, n, 2), F)
    ur[0, :, 0], ur[0, :, 1], ua[0, :, 0], ua[0, :, 1] = PR._u01(c0), PR._u01(c2), PR._u01(c1), PR._u01(c3)
    return ur, ua
