// The tile phases of eod_ssim (include/eodiff.h states the operations), free of HIP headers: csrc/metrics.hip
// instantiates them as device code, tests/ssim_host_check.cc walks them on the host, thread number by thread number, under the sanitizers.
//
// One workgroup of SSIM_THREADS threads owns SSIM_TILE x SSIM_TILE window positions of one (sample, band) plane.  The window at position
// (y, x) covers rows y .. y + 2r and columns x .. x + 2r of the plane and has its centre at (y + r, x + r); the positions of a plane are
// 0 .. H - 2r - 1 by 0 .. W - 2r - 1 (the valid region: no padding exists).  The tile therefore reads E x E elements, E = SSIM_TILE + 2r:
// the halo is 2r, on the far side only.  Phases, separated by workgroup barriers:
//   ssim_load     the E x E elements of both images, converted to double and put through the affine once: P and T (row pitch E);
//                 an element outside the plane is 0.0 and reaches only positions outside the valid region, which store nothing
//   for q = 0 .. 4 (p, t, p*p, t*t, p*t -- the products formed in double from P and T):
//     ssim_hpass  E rows x SSIM_TILE columns of the horizontal sums into the ONE line buffer hb (row pitch SSIM_TILE)
//     ssim_vpass  the vertical sums of the thread's SSIM_PER positions from hb, kept in its registers m[q][]
//   ssim_finish   the map value of each position, the fp32 store, and the thread's sum over its counted positions
// LDS, sized by the launch: P and T 2 x E x E x 8 B, hb E x 32 x 8 B -- 39 KiB at r = 5 (four workgroups per CU), 64512 B at r = 12.  Banks:
// the 32 lanes of a half-wave read 32 consecutive doubles of one row in every phase (ds_read_b64 banks by (a / 4) mod 64: 32 x 8 B is
// exactly one bank row whatever the row's offset), so neither pitch needs padding.
// A thread's window sums advance together, tap by tap (SSIM_HPER row sums, SSIM_PER column sums): each sum still takes its taps in
// ascending order, and the LDS reads of one tap are independent of each other.
#pragma once
#include <stdint.h>

#ifndef SSIM_FN
#define SSIM_FN static inline
#endif

#define SSIM_MAXR 12                          // window radius
#define SSIM_MAXC 32                          // bands
#define SSIM_THREADS 256
#define SSIM_TILE 32                          // window positions per tile edge (tests/test_gpu_metrics.py: SSIM_TILE and its edge list)
#define SSIM_ROWS (SSIM_TILE + 2 * SSIM_MAXR)  // 56: the largest tile with its halo
#define SSIM_HPER ((SSIM_ROWS * SSIM_TILE + SSIM_THREADS - 1) / SSIM_THREADS)  // 7 row sums per thread at the most: t + SSIM_THREADS * e
#define SSIM_PER (SSIM_TILE * SSIM_TILE / SSIM_THREADS)  // 4 positions per thread: t + SSIM_THREADS * j

struct SsimTaps {
    double g[2 * SSIM_MAXR + 1];
};

struct SsimArgs {
    const float* pred;
    const float* ref;
    const float* where;  // or null
    float* map;          // or null
    double* part;        // [B * C][tiles]{sum, n}
    int B, C, H, W, r, ref_B, where_B;
    int tiles_x, tiles_y;
    double a, b, c1, c2;
};

SSIM_FN void ssim_load(const SsimArgs& g, int t, long long plane_p, long long plane_t, int y0, int x0, double* P, double* T) {
    const int E = SSIM_TILE + 2 * g.r;
    for (int i = t; i < E * E; i += SSIM_THREADS) {
        const int ly = i / E, lx = i - ly * E;
        const long long y = (long long)y0 + ly, x = (long long)x0 + lx;
        double p = 0.0, q = 0.0;
        if (y < g.H && x < g.W) {
            const long long o = y * g.W + x;
            const double mp = g.a * (double)g.pred[plane_p + o];
            const double mt = g.a * (double)g.ref[plane_t + o];
            p = mp + g.b;
            q = mt + g.b;
        }
        P[i] = p;
        T[i] = q;
    }
}

SSIM_FN double ssim_quantity(int q, double p, double t) {
    return q == 0 ? p : q == 1 ? t : q == 2 ? p * p : q == 3 ? t * t : p * t;
}

SSIM_FN void ssim_hpass(const SsimArgs& g, const SsimTaps& k, int q, int t, const double* P, const double* T, double* hb) {
    const int E = SSIM_TILE + 2 * g.r, L = 2 * g.r + 1;
    const int row0 = t / SSIM_TILE, col = t - row0 * SSIM_TILE;
    double s[SSIM_HPER];
    int off[SSIM_HPER];
#pragma unroll
    for (int e = 0; e < SSIM_HPER; ++e) {
        const int row = row0 + (SSIM_THREADS / SSIM_TILE) * e;
        off[e] = (row < E ? row : row0) * E + col;  // (a row the tile does not have: row0's sum once more, not stored)
        s[e] = k.g[0] * ssim_quantity(q, P[off[e]], T[off[e]]);
    }
    for (int j = 1; j < L; ++j) {
#pragma unroll
        for (int e = 0; e < SSIM_HPER; ++e) {
            const double m = k.g[j] * ssim_quantity(q, P[off[e] + j], T[off[e] + j]);
            s[e] = s[e] + m;
        }
    }
#pragma unroll
    for (int e = 0; e < SSIM_HPER; ++e) {
        const int row = row0 + (SSIM_THREADS / SSIM_TILE) * e;
        if (row < E) hb[row * SSIM_TILE + col] = s[e];
    }
}

SSIM_FN void ssim_vpass(const SsimArgs& g, const SsimTaps& k, int t, const double* hb, double* m) {
    const int L = 2 * g.r + 1;
    double s[SSIM_PER];
#pragma unroll
    for (int j = 0; j < SSIM_PER; ++j) s[j] = k.g[0] * hb[t + SSIM_THREADS * j];  // position (oy, ox) = ((t + 256 j) / 32, t % 32): hb[oy * 32 + ox]
    for (int u = 1; u < L; ++u) {
#pragma unroll
        for (int j = 0; j < SSIM_PER; ++j) {
            const double v = k.g[u] * hb[t + SSIM_THREADS * j + u * SSIM_TILE];
            s[j] = s[j] + v;
        }
    }
#pragma unroll
    for (int j = 0; j < SSIM_PER; ++j) m[j] = s[j];
}

SSIM_FN double ssim_value(double mp, double mt, double epp, double ett, double ept, double c1, double c2) {
    const double mpp = mp * mp, mtt = mt * mt, mpt = mp * mt;
    const double spp = epp - mpp, stt = ett - mtt, spt = ept - mpt;
    const double n1 = 2.0 * mpt + c1, n2 = 2.0 * spt + c2;
    const double d1 = (mpp + mtt) + c1, d2 = (spp + stt) + c2;
    return (n1 * n2) / (d1 * d2);
}

// m[q * SSIM_PER + j]; plane_o: the map's plane; plane_w: the plane of `where` (not read when g.where is null)
SSIM_FN void ssim_finish(const SsimArgs& g, int t, long long plane_o, long long plane_w, int y0, int x0, const double* m, double* sum, double* cnt) {
    double s = 0.0, n = 0.0;
    for (int j = 0; j < SSIM_PER; ++j) {
        const int i = t + SSIM_THREADS * j, oy = i / SSIM_TILE, ox = i - oy * SSIM_TILE;
        const long long cy = (long long)y0 + oy + g.r, cx = (long long)x0 + ox + g.r;  // the window's centre
        if (cy >= g.H - g.r || cx >= g.W - g.r) continue;
        const double v = ssim_value(m[0 * SSIM_PER + j], m[1 * SSIM_PER + j], m[2 * SSIM_PER + j], m[3 * SSIM_PER + j], m[4 * SSIM_PER + j], g.c1, g.c2);
        const long long o = cy * g.W + cx;
        if (g.map) g.map[plane_o + o] = (float)v;
        if (!g.where || g.where[plane_w + o] != 0.0f) {
            s = s + v;
            n = n + 1.0;
        }
    }
    *sum = s;
    *cnt = n;
}
