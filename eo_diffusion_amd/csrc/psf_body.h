// The bodies of the two PSF kernels (csrc/psf.hip), one phase of one tile for one thread at a time.  The kernels call
// the phases in order with a barrier after each; a host program can do the same with a loop over the 256 thread numbers per phase
// (tests/psf_host_check.cc does, under the address and undefined-behaviour sanitizers).  Nothing here needs the HIP headers.
#pragma once
#include <stdint.h>

#ifndef PSF_FN
#define PSF_FN static inline
#endif

#define PSF_MAXR 12                        // tap radius
#define PSF_MAXC 32                        // channels
#define PSF_THREADS 256
#define PSF_MAXT 32                        // the largest tile edge in full-resolution pixels
#define PSF_ROWS (PSF_MAXT + 2 * PSF_MAXR)  // 56: a tile with its halo
#define PSF_MAXK 8                         // observed bands of a mixed observation (EOD_SPEC_MAXK of csrc/sampler.hip)
#define PSF_PITCH 64                       // row pitch of a buffer filled by aligned quads: 56 + up to 3 leading columns, rounded up to a quad

typedef float psf_f4 __attribute__((ext_vector_type(4)));

struct PsfTaps {
    float h[2 * PSF_MAXR + 1];
};

struct PsfArgs {
    const float* p;       // [B][C][H][W]
    const float* values;  // residual: [B or 1][K][H/f][W/f], NULL: the operator alone
    const float* mask;    // residual: NULL or [B or 1][K or 1][H/f][W/f]
    const float* q;       // update: [B][K][H/f][W/f]
    float* out;           // residual: [B][K][H/f][W/f]; update: [B][C][H][W]
    float lambda, step;
    int r, f, K, B, C, H, W;
    int values_b1, mask_b1, mask_c1;
    int tc, tiles_x, tiles_y;          // coarse outputs per tile edge (the tile is tc * f pixels: psf_tile_coarse), tiles per plane
    signed char kof[PSF_MAXC];         // update: the row k of channel c, -1: not observed (copied)
    unsigned char ch[PSF_MAXC];        // residual: the channel of row k
};

// coarse outputs per tile edge for f = 1 .. 8: a multiple of 4 (coarse rows go by quads) with tc * f <= 32 -> tiles of 32, 32, 24, 32, 20, 24, 28, 32
PSF_FN int psf_tile_coarse(int f) { return f == 1 ? 32 : f == 2 ? 16 : f <= 4 ? 8 : 4; }

struct PsfResLds {
    float patch[PSF_ROWS * PSF_PITCH];  // p over the tile and its halo, out-of-plane 0; afterwards b (pitch PSF_MAXT)
    float hbuf[PSF_ROWS * PSF_MAXT];    // the horizontal pass
    float nh[PSF_MAXT], nv[PSF_MAXT];
};

struct PsfUpdLds {
    float qs[PSF_ROWS * PSF_PITCH];     // q over the tile's coarse pixels and their halo
    float w[PSF_ROWS * PSF_ROWS];       // w over the tile and its halo, out-of-plane 0
    float hbuf[PSF_ROWS * PSF_MAXT];
    float nh[PSF_ROWS], nv[PSF_ROWS];
};

// the mixing matrix of eod_psf_*_mix, by value: R[k][c] at m[k * PSF_MAXC + c] (residual), G[c][k] at m[c * PSF_MAXK + k] (update)
struct PsfMix {
    float m[PSF_MAXK * PSF_MAXC];
};

// conv of a line of ones of length L at position x: the contract's nh / nv
PSF_FN float psf_norm(const PsfTaps& t, int r, int x, int L) {
    float acc = t.h[0] * ((x - r >= 0 && x - r < L) ? 1.0f : 0.0f);
    for (int i = 1; i <= 2 * r; ++i) {
        const int xi = x - r + i;
        const float pr = t.h[i] * ((xi >= 0 && xi < L) ? 1.0f : 0.0f);
        acc = acc + pr;
    }
    return acc;
}

// taps in ascending order over u[0], u[stride], ...: the contract's conv_h / conv_v
// The loop is unrolled over groups of four taps with one wave-uniform test per group (2r is even: a group holds four taps or its first
// two), so the taps are scalar registers, the offsets are immediates and a group's loads are in flight together; the adds stay sequential.
PSF_FN float psf_conv(const PsfTaps& t, int r, const float* u, int stride) {
    float acc = t.h[0] * u[0];
    const int last = 2 * r;
#pragma unroll
    for (int i = 1; i <= 2 * PSF_MAXR; i += 4) {
        if (i > last) break;
        const float u0 = u[i * stride], u1 = u[(i + 1) * stride];
        const float p0 = t.h[i] * u0, p1 = t.h[i + 1] * u1;
        if (i + 3 <= last) {
            const float u2 = u[(i + 2) * stride], u3 = u[(i + 3) * stride];
            const float p2 = t.h[i + 2] * u2, p3 = t.h[i + 3] * u3;
            acc = acc + p0;
            acc = acc + p1;
            acc = acc + p2;
            acc = acc + p3;
        } else {
            acc = acc + p0;
            acc = acc + p1;
        }
    }
    return acc;
}

// the same operations as a plain loop: eod_psf_update, whose five phases leave no scalar registers for 25 resident taps
PSF_FN float psf_conv_loop(const PsfTaps& t, int r, const float* u, int stride) {
    float acc = t.h[0] * u[0];
    for (int i = 1; i <= 2 * r; ++i) {
        const float pr = t.h[i] * u[i * stride];
        acc = acc + pr;
    }
    return acc;
}

struct PsfTile {
    long long plane;  // b * K + k (residual), b * C + c (update)
    int y0, x0, ft;
};
PSF_FN PsfTile psf_tile_of(const PsfArgs& g, long long item) {
    const long long tiles = (long long)g.tiles_x * g.tiles_y;
    const int tile = (int)(item % tiles);
    PsfTile t;
    t.plane = item / tiles;
    t.ft = g.tc * g.f;
    t.y0 = (tile / g.tiles_x) * t.ft;
    t.x0 = (tile % g.tiles_x) * t.ft;
    return t;
}

// ------------------------------------------------------------------------------------------------ q = lm * (D_f (blur(p) / n) - values)
// phase 0: the patch and nh / nv;  1: horizontal;  2: vertical and / n;  3: block sums, residual, store
template <bool VEC, bool VECQ>
PSF_FN void psf_residual_phase(int phase, const PsfArgs& g, const PsfTaps& t, PsfResLds& s, long long item, int tid) {
    const PsfTile tl = psf_tile_of(g, item);
    const int r = g.r, f = g.f, ft = tl.ft, y0 = tl.y0, x0 = tl.x0;
    const int b = (int)(tl.plane / g.K), k = (int)(tl.plane % g.K);
    const int rows = ft + 2 * r;
    const int xs = (x0 - r) & ~3;          // the patch starts at a quad boundary at or left of x0 - r (negative: still a multiple of 4)
    const int lead = x0 - r - xs;
    if (phase == 0) {
        const float* src = g.p + ((long long)b * g.C + g.ch[k]) * g.H * g.W;
        const int nq = (lead + ft + 2 * r + 3) / 4;
        for (int idx = tid; idx < rows * nq; idx += PSF_THREADS) {
            const int row = idx / nq, qd = idx % nq;
            const int gy = y0 - r + row, gx = xs + 4 * qd;
            psf_f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (gy >= 0 && gy < g.H) {
                if (VEC) {
                    if (gx >= 0 && gx < g.W) v = *reinterpret_cast<const psf_f4*>(src + (long long)gy * g.W + gx);   // W % 4 == 0: a whole quad
                } else {
                    for (int j = 0; j < 4; ++j)
                        if (gx + j >= 0 && gx + j < g.W) v[j] = src[(long long)gy * g.W + gx + j];
                }
            }
            *reinterpret_cast<psf_f4*>(s.patch + row * PSF_PITCH + 4 * qd) = v;
        }
        if (tid < ft) s.nh[tid] = psf_norm(t, r, x0 + tid, g.W);
        else if (tid >= 64 && tid < 64 + ft) s.nv[tid - 64] = psf_norm(t, r, y0 + tid - 64, g.H);
    } else if (phase == 1) {
        for (int idx = tid; idx < rows * ft; idx += PSF_THREADS) {
            const int row = idx / ft, x = idx % ft;
            s.hbuf[row * PSF_MAXT + x] = psf_conv(t, r, s.patch + row * PSF_PITCH + lead + x, 1);
        }
    } else if (phase == 2) {
        for (int idx = tid; idx < ft * ft; idx += PSF_THREADS) {
            const int y = idx / ft, x = idx % ft;
            float bv = 0.0f;
            if (y0 + y < g.H && x0 + x < g.W) {
                const float acc = psf_conv(t, r, s.hbuf + y * PSF_MAXT + x, PSF_MAXT);
                const float n = s.nv[y] * s.nh[x];
                bv = acc / n;
            }
            s.patch[y * PSF_MAXT + x] = bv;
        }
    } else {
        const int Hc = g.H / f, Wc = g.W / f, tc = g.tc;
        const long long chw = (long long)Hc * Wc;
        const float* val = g.values ? g.values + ((long long)(g.values_b1 ? 0 : b) * g.K + k) * chw : nullptr;
        const float* msk = (g.values && g.mask) ? g.mask + ((long long)(g.mask_b1 ? 0 : b) * (g.mask_c1 ? 1 : g.K) + (g.mask_c1 ? 0 : k)) * chw : nullptr;
        float* dst = g.out + tl.plane * chw;
        const float ff = (float)(f * f);
        const int per = VECQ ? 4 : 1, nx = tc / per;
        for (int idx = tid; idx < tc * nx; idx += PSF_THREADS) {
            const int cy = idx / nx, cx = (idx % nx) * per;
            const int gy = (y0 / f) + cy, gx = (x0 / f) + cx;
            if (gy >= Hc || gx >= Wc) continue;              // VECQ: Wc % 4 == 0 and gx % 4 == 0, the quad is inside or outside as a whole
            const long long at = (long long)gy * Wc + gx;
            float vv[4] = {0.0f, 0.0f, 0.0f, 0.0f}, mv[4] = {1.0f, 1.0f, 1.0f, 1.0f}, o[4];
            if (VECQ) {
                if (val) { const psf_f4 q4 = *reinterpret_cast<const psf_f4*>(val + at); vv[0] = q4[0]; vv[1] = q4[1]; vv[2] = q4[2]; vv[3] = q4[3]; }
                if (msk) { const psf_f4 q4 = *reinterpret_cast<const psf_f4*>(msk + at); mv[0] = q4[0]; mv[1] = q4[1]; mv[2] = q4[2]; mv[3] = q4[3]; }
            } else {
                if (val) vv[0] = val[at];
                if (msk) mv[0] = msk[at];
            }
            for (int j = 0; j < per; ++j) {
                const float* blk = s.patch + (cy * f) * PSF_MAXT + (cx + j) * f;
                float sum = blk[0];
                for (int i = 1; i < f * f; ++i) sum = sum + blk[(i / f) * PSF_MAXT + i % f];   // row by row, left to right
                const float mean = sum / ff;
                if (val) {
                    const float lm = g.lambda * mv[j];
                    const float df = mean - vv[j];
                    o[j] = lm * df;
                } else {
                    o[j] = mean;
                }
            }
            if (VECQ) { const psf_f4 q4 = {o[0], o[1], o[2], o[3]}; *reinterpret_cast<psf_f4*>(dst + at) = q4; }
            else dst[at] = o[0];
        }
    }
}

// ------------------------------------------------------------------------------------------------ out = p - blur((replicate(q) * step) / n)
// a plane that is not observed: out = p over the tile
template <bool VEC>
PSF_FN void psf_copy_tile(const PsfArgs& g, const PsfTile& tl, int tid) {
    const float* src = g.p + tl.plane * g.H * g.W;
    float* dst = g.out + tl.plane * g.H * g.W;
    const int ft = tl.ft, per = VEC ? 4 : 1, nx = ft / per;
    for (int idx = tid; idx < ft * nx; idx += PSF_THREADS) {
        const int gy = tl.y0 + idx / nx, gx = tl.x0 + (idx % nx) * per;
        if (gy >= g.H || gx >= g.W) continue;
        const long long at = (long long)gy * g.W + gx;
        if (VEC) *reinterpret_cast<psf_f4*>(dst + at) = *reinterpret_cast<const psf_f4*>(src + at);
        else dst[at] = src[at];
    }
}

// phase 0: q and nh / nv over the tile and its halo;  1: w;  2: horizontal;  3: vertical;  4: out = p - blur(w)
template <bool VEC, bool VECQ>
PSF_FN void psf_update_phase(int phase, const PsfArgs& g, const PsfTaps& t, PsfUpdLds& s, long long item, int tid) {
    const PsfTile tl = psf_tile_of(g, item);
    const int c = (int)(tl.plane % g.C), b = (int)(tl.plane / g.C);
    const int k = g.kof[c];
    if (k < 0) {
        if (phase == 4) psf_copy_tile<VEC>(g, tl, tid);
        return;
    }
    const int r = g.r, f = g.f, ft = tl.ft, y0 = tl.y0, x0 = tl.x0;
    const int rows = ft + 2 * r;           // w is rows x rows from (y0 - r, x0 - r)
    const int Hc = g.H / f, Wc = g.W / f;
    const int ylo = y0 - r < 0 ? 0 : y0 - r, xlo = x0 - r < 0 ? 0 : x0 - r;
    const int yhi = y0 + ft + r > g.H ? g.H : y0 + ft + r, xhi = x0 + ft + r > g.W ? g.W : x0 + ft + r;   // in-plane part of the w region (never empty)
    const int cy0 = ylo / f, cx0 = xlo / f, cy1 = (yhi - 1) / f, cx1 = (xhi - 1) / f;
    const int cxs = cx0 & ~3;
    if (phase == 0) {
        const float* src = g.q + ((long long)b * g.K + k) * Hc * Wc;
        const int nq = (cx1 - cxs) / 4 + 1, qrows = cy1 - cy0 + 1;
        for (int idx = tid; idx < qrows * nq; idx += PSF_THREADS) {
            const int row = idx / nq, qd = idx % nq;
            const int gy = cy0 + row, gx = cxs + 4 * qd;
            psf_f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (VECQ) {
                v = *reinterpret_cast<const psf_f4*>(src + (long long)gy * Wc + gx);    // gx <= cx1 < Wc, Wc % 4 == 0: a whole quad
            } else {
                for (int j = 0; j < 4; ++j)
                    if (gx + j < Wc) v[j] = src[(long long)gy * Wc + gx + j];
            }
            *reinterpret_cast<psf_f4*>(s.qs + row * PSF_PITCH + 4 * qd) = v;
        }
        if (tid < rows) s.nh[tid] = psf_norm(t, r, x0 - r + tid, g.W);
        else if (tid >= 64 && tid < 64 + rows) s.nv[tid - 64] = psf_norm(t, r, y0 - r + tid - 64, g.H);
    } else if (phase == 1) {
        for (int idx = tid; idx < rows * rows; idx += PSF_THREADS) {
            const int wy = idx / rows, wx = idx % rows;
            const int gy = y0 - r + wy, gx = x0 - r + wx;
            float wv = 0.0f;
            if (gy >= 0 && gy < g.H && gx >= 0 && gx < g.W) {
                const float qv = s.qs[(gy / f - cy0) * PSF_PITCH + (gx / f - cxs)];
                const float ts = qv * g.step;
                const float n = s.nv[wy] * s.nh[wx];
                wv = ts / n;
            }
            s.w[wy * PSF_ROWS + wx] = wv;
        }
    } else if (phase == 2) {
        for (int idx = tid; idx < rows * ft; idx += PSF_THREADS) {
            const int row = idx / ft, x = idx % ft;
            s.hbuf[row * PSF_MAXT + x] = psf_conv_loop(t, r, s.w + row * PSF_ROWS + x, 1);
        }
    } else if (phase == 3) {
        for (int idx = tid; idx < ft * ft; idx += PSF_THREADS) {          // (w is dead: the blur goes where it was, pitch PSF_MAXT)
            const int y = idx / ft, x = idx % ft;
            s.w[y * PSF_MAXT + x] = psf_conv_loop(t, r, s.hbuf + y * PSF_MAXT + x, PSF_MAXT);
        }
    } else {
        const float* src = g.p + tl.plane * g.H * g.W;
        float* dst = g.out + tl.plane * g.H * g.W;
        const int per = VEC ? 4 : 1, nx = ft / per;
        for (int idx = tid; idx < ft * nx; idx += PSF_THREADS) {
            const int y = idx / nx, x = (idx % nx) * per;
            const int gy = y0 + y, gx = x0 + x;
            if (gy >= g.H || gx >= g.W) continue;            // VEC: W % 4 == 0 and gx % 4 == 0, the quad is inside or outside as a whole
            const long long at = (long long)gy * g.W + gx;
            if (VEC) {
                const psf_f4 pv = *reinterpret_cast<const psf_f4*>(src + at);
                const psf_f4 bl = *reinterpret_cast<const psf_f4*>(s.w + y * PSF_MAXT + x);
                const psf_f4 o = {pv[0] - bl[0], pv[1] - bl[1], pv[2] - bl[2], pv[3] - bl[3]};
                *reinterpret_cast<psf_f4*>(dst + at) = o;
            } else {
                dst[at] = src[at] - s.w[y * PSF_MAXT + x];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ the same through a band mix (section 9.10)
// (m[0] * x_0) + (m[1] * x_1) + ... over n planes `stride` apart, a quad at a time, the adds in index order.  The planes are taken four
// at a time with the four loads issued before the first of them is used (the tests on n are wave-uniform): one plane per trip leaves a
// single load in flight per thread, and the staging loop is then bound by the latency of n dependent round trips.
PSF_FN psf_f4 psf_mix_quads(const float* base, long long stride, const float* m, int n) {
    psf_f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int i = 0; i < n; i += 4) {
        const int left = n - i;
        const psf_f4 z = {0.0f, 0.0f, 0.0f, 0.0f};
        const psf_f4 a = *reinterpret_cast<const psf_f4*>(base + i * stride);
        const psf_f4 b = left > 1 ? *reinterpret_cast<const psf_f4*>(base + (i + 1) * stride) : z;
        const psf_f4 c = left > 2 ? *reinterpret_cast<const psf_f4*>(base + (i + 2) * stride) : z;
        const psf_f4 d = left > 3 ? *reinterpret_cast<const psf_f4*>(base + (i + 3) * stride) : z;
        const float ma = m[i];
        const psf_f4 pa = {ma * a[0], ma * a[1], ma * a[2], ma * a[3]};
        if (i == 0) v = pa;
        else { v[0] = v[0] + pa[0]; v[1] = v[1] + pa[1]; v[2] = v[2] + pa[2]; v[3] = v[3] + pa[3]; }
        if (left > 1) { const float mb = m[i + 1]; const psf_f4 pb = {mb * b[0], mb * b[1], mb * b[2], mb * b[3]};
                        v[0] = v[0] + pb[0]; v[1] = v[1] + pb[1]; v[2] = v[2] + pb[2]; v[3] = v[3] + pb[3]; }
        if (left > 2) { const float mc = m[i + 2]; const psf_f4 pc = {mc * c[0], mc * c[1], mc * c[2], mc * c[3]};
                        v[0] = v[0] + pc[0]; v[1] = v[1] + pc[1]; v[2] = v[2] + pc[2]; v[3] = v[3] + pc[3]; }
        if (left > 3) { const float md = m[i + 3]; const psf_f4 pd = {md * d[0], md * d[1], md * d[2], md * d[3]};
                        v[0] = v[0] + pd[0]; v[1] = v[1] + pd[1]; v[2] = v[2] + pd[2]; v[3] = v[3] + pd[3]; }
    }
    return v;
}

// q_k = lm * (D_f (blur(u_k) / n) - values_k), u_k = sum_c R[k][c] * p_c: phase 0 stages u_k (the channel planes quad by quad, the running
// sum in registers, LDS written once); phases 1 .. 3 are psf_residual_phase's on the staged patch.  g.K bands, g.mask_c1 = 1.
template <bool VEC, bool VECQ>
PSF_FN void psf_residual_mix_phase(int phase, const PsfArgs& g, const PsfTaps& t, const PsfMix& mx, PsfResLds& s, long long item, int tid) {
    if (phase != 0) {
        psf_residual_phase<VEC, VECQ>(phase, g, t, s, item, tid);
        return;
    }
    const PsfTile tl = psf_tile_of(g, item);
    const int r = g.r, ft = tl.ft, y0 = tl.y0, x0 = tl.x0;
    const int b = (int)(tl.plane / g.K), k = (int)(tl.plane % g.K);
    const int rows = ft + 2 * r;
    const int xs = (x0 - r) & ~3;
    const int lead = x0 - r - xs;
    const long long hw = (long long)g.H * g.W;
    const float* src = g.p + (long long)b * g.C * hw;
    const float* R = mx.m + k * PSF_MAXC;
    const int nq = (lead + ft + 2 * r + 3) / 4;
    for (int idx = tid; idx < rows * nq; idx += PSF_THREADS) {
        const int row = idx / nq, qd = idx % nq;
        const int gy = y0 - r + row, gx = xs + 4 * qd;
        psf_f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (gy >= 0 && gy < g.H) {
            const long long at = (long long)gy * g.W + gx;
            if (VEC) {
                if (gx >= 0 && gx < g.W) v = psf_mix_quads(src + at, hw, R, g.C);   // W % 4 == 0: a whole quad
            } else {
                for (int j = 0; j < 4; ++j)
                    if (gx + j >= 0 && gx + j < g.W) {
                        float u = R[0] * src[at + j];
                        for (int c = 1; c < g.C; ++c) {
                            const float pr = R[c] * src[c * hw + at + j];
                            u = u + pr;
                        }
                        v[j] = u;
                    }
            }
        }
        *reinterpret_cast<psf_f4*>(s.patch + row * PSF_PITCH + 4 * qd) = v;
    }
    if (tid < ft) s.nh[tid] = psf_norm(t, r, x0 + tid, g.W);
    else if (tid >= 64 && tid < 64 + ft) s.nv[tid - 64] = psf_norm(t, r, y0 + tid - 64, g.H);
}

// out_c = p_c - blur((replicate(s_c) * step) / n), s_c = sum_k G[c][k] * q_k: phase 0 stages s_c over the tile's coarse pixels and their
// halo; phases 1 .. 4 are psf_update_phase's.  Every channel is written (g.kof[c] = 0 for all c: no copied plane).
template <bool VEC, bool VECQ>
PSF_FN void psf_update_mix_phase(int phase, const PsfArgs& g, const PsfTaps& t, const PsfMix& mx, PsfUpdLds& s, long long item, int tid) {
    if (phase != 0) {
        psf_update_phase<VEC, VECQ>(phase, g, t, s, item, tid);
        return;
    }
    const PsfTile tl = psf_tile_of(g, item);
    const int c = (int)(tl.plane % g.C), b = (int)(tl.plane / g.C);
    const int r = g.r, f = g.f, ft = tl.ft, y0 = tl.y0, x0 = tl.x0;
    const int rows = ft + 2 * r;
    const int Hc = g.H / f, Wc = g.W / f;
    const int ylo = y0 - r < 0 ? 0 : y0 - r, xlo = x0 - r < 0 ? 0 : x0 - r;
    const int yhi = y0 + ft + r > g.H ? g.H : y0 + ft + r, xhi = x0 + ft + r > g.W ? g.W : x0 + ft + r;
    const int cy0 = ylo / f, cx0 = xlo / f, cy1 = (yhi - 1) / f, cx1 = (xhi - 1) / f;
    const int cxs = cx0 & ~3;
    const long long chw = (long long)Hc * Wc;
    const float* src = g.q + (long long)b * g.K * chw;
    const float* G = mx.m + c * PSF_MAXK;
    const int nq = (cx1 - cxs) / 4 + 1, qrows = cy1 - cy0 + 1;
    for (int idx = tid; idx < qrows * nq; idx += PSF_THREADS) {
        const int row = idx / nq, qd = idx % nq;
        const int gy = cy0 + row, gx = cxs + 4 * qd;
        const long long at = (long long)gy * Wc + gx;
        psf_f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (VECQ) {                                             // gx <= cx1 < Wc, Wc % 4 == 0: a whole quad
            v = psf_mix_quads(src + at, chw, G, g.K);
        } else {
            for (int j = 0; j < 4; ++j)
                if (gx + j < Wc) {
                    float u = G[0] * src[at + j];
                    for (int k = 1; k < g.K; ++k) {
                        const float pr = G[k] * src[k * chw + at + j];
                        u = u + pr;
                    }
                    v[j] = u;
                }
        }
        *reinterpret_cast<psf_f4*>(s.qs + row * PSF_PITCH + 4 * qd) = v;
    }
    if (tid < rows) s.nh[tid] = psf_norm(t, r, x0 - r + tid, g.W);
    else if (tid >= 64 && tid < 64 + rows) s.nv[tid - 64] = psf_norm(t, r, y0 - r + tid - 64, g.H);
}

// ------------------------------------------------------------------------------------------------ one tap vector per axis (section 9.11)
// hx[0 .. 2 rx] along x and hy[0 .. 2 ry] along y, not necessarily symmetric, the radii independent.  The residual carries the forward
// taps; the update carries them REVERSED (h~[t] = h[2r - t]: B0^T is the correlation with the reversed taps), so both run the one
// convolution routine.  n is the conv of a line of ones with the FORWARD taps in both: psf_norm_rev reads a reversed array backwards.
struct PsfTapsXy {
    PsfTaps y, x;
    int ry, rx;
};

PSF_FN float psf_norm_rev(const PsfTaps& t, int r, int x, int L) {
    float acc = t.h[2 * r] * ((x - r >= 0 && x - r < L) ? 1.0f : 0.0f);
    for (int i = 1; i <= 2 * r; ++i) {
        const int xi = x - r + i;
        const float pr = t.h[2 * r - i] * ((xi >= 0 && xi < L) ? 1.0f : 0.0f);
        acc = acc + pr;
    }
    return acc;
}

// The residual of a tile: ft + 2 ry rows of lead + ft + 2 rx columns are staged (PSF_PITCH holds 3 + 32 + 24 columns rounded up to a
// quad, PsfResLds 56 rows: the maxima; the loops run over the real extents, no zero tap is ever multiplied).  phase 0: the patch (MIX: the
// band mix of section 9.10, mx->m = R) and nh / nv;  1: horizontal with hx;  2: vertical with hy and / n;  3: psf_residual_phase's.
template <bool VEC, bool VECQ, bool MIX>
PSF_FN void psf_residual_xy_phase(int phase, const PsfArgs& g, const PsfTapsXy& tt, const PsfMix* mx, PsfResLds& s, long long item, int tid) {
    if (phase == 3) {
        psf_residual_phase<VEC, VECQ>(3, g, tt.x, s, item, tid);
        return;
    }
    const PsfTile tl = psf_tile_of(g, item);
    const int ry = tt.ry, rx = tt.rx, ft = tl.ft, y0 = tl.y0, x0 = tl.x0;
    const int b = (int)(tl.plane / g.K), k = (int)(tl.plane % g.K);
    const int rows = ft + 2 * ry;
    const int xs = (x0 - rx) & ~3;         // the patch starts at a quad boundary at or left of x0 - rx
    const int lead = x0 - rx - xs;
    if (phase == 0) {
        const long long hw = (long long)g.H * g.W;
        const float* src = g.p + ((long long)b * g.C + (MIX ? 0 : g.ch[k])) * hw;
        const float* R = MIX ? mx->m + k * PSF_MAXC : nullptr;
        const int nq = (lead + ft + 2 * rx + 3) / 4;
        for (int idx = tid; idx < rows * nq; idx += PSF_THREADS) {
            const int row = idx / nq, qd = idx % nq;
            const int gy = y0 - ry + row, gx = xs + 4 * qd;
            psf_f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (gy >= 0 && gy < g.H) {
                const long long at = (long long)gy * g.W + gx;
                if (VEC) {
                    if (gx >= 0 && gx < g.W) {                                    // W % 4 == 0: a whole quad
                        if (MIX) v = psf_mix_quads(src + at, hw, R, g.C);
                        else v = *reinterpret_cast<const psf_f4*>(src + at);
                    }
                } else {
                    for (int j = 0; j < 4; ++j)
                        if (gx + j >= 0 && gx + j < g.W) {
                            if (MIX) {
                                float u = R[0] * src[at + j];
                                for (int c = 1; c < g.C; ++c) {
                                    const float pr = R[c] * src[c * hw + at + j];
                                    u = u + pr;
                                }
                                v[j] = u;
                            } else {
                                v[j] = src[at + j];
                            }
                        }
                }
            }
            *reinterpret_cast<psf_f4*>(s.patch + row * PSF_PITCH + 4 * qd) = v;
        }
        if (tid < ft) s.nh[tid] = psf_norm(tt.x, rx, x0 + tid, g.W);
        else if (tid >= 64 && tid < 64 + ft) s.nv[tid - 64] = psf_norm(tt.y, ry, y0 + tid - 64, g.H);
    } else if (phase == 1) {
        for (int idx = tid; idx < rows * ft; idx += PSF_THREADS) {
            const int row = idx / ft, x = idx % ft;
            s.hbuf[row * PSF_MAXT + x] = psf_conv(tt.x, rx, s.patch + row * PSF_PITCH + lead + x, 1);
        }
    } else {
        for (int idx = tid; idx < ft * ft; idx += PSF_THREADS) {
            const int y = idx / ft, x = idx % ft;
            float bv = 0.0f;
            if (y0 + y < g.H && x0 + x < g.W) {
                const float acc = psf_conv(tt.y, ry, s.hbuf + y * PSF_MAXT + x, PSF_MAXT);
                const float n = s.nv[y] * s.nh[x];
                bv = acc / n;
            }
            s.patch[y * PSF_MAXT + x] = bv;
        }
    }
}

// The update of a tile: w over (ft + 2 ry) x (ft + 2 rx) pixels from (y0 - ry, x0 - rx), row pitch PSF_ROWS; the coarse pixels under it
// reach ceil(ry / f) rows and ceil(rx / f) columns beyond the tile's own.  tt holds the REVERSED taps.  phase 0: q (MIX: s_c = sum_k
// G[c][k] q_k, mx->m = G) and nh / nv;  1: w;  2: horizontal with hx~;  3: vertical with hy~;  4: psf_update_phase's (the copied planes too).
template <bool VEC, bool VECQ, bool MIX>
PSF_FN void psf_update_xy_phase(int phase, const PsfArgs& g, const PsfTapsXy& tt, const PsfMix* mx, PsfUpdLds& s, long long item, int tid) {
    if (phase == 4) {
        psf_update_phase<VEC, VECQ>(4, g, tt.x, s, item, tid);
        return;
    }
    const PsfTile tl = psf_tile_of(g, item);
    const int c = (int)(tl.plane % g.C), b = (int)(tl.plane / g.C);
    const int k = g.kof[c];
    if (k < 0) return;
    const int ry = tt.ry, rx = tt.rx, f = g.f, ft = tl.ft, y0 = tl.y0, x0 = tl.x0;
    const int rows = ft + 2 * ry, cols = ft + 2 * rx;
    const int Hc = g.H / f, Wc = g.W / f;
    const int ylo = y0 - ry < 0 ? 0 : y0 - ry, xlo = x0 - rx < 0 ? 0 : x0 - rx;
    const int yhi = y0 + ft + ry > g.H ? g.H : y0 + ft + ry, xhi = x0 + ft + rx > g.W ? g.W : x0 + ft + rx;   // in-plane part of the w region (never empty)
    const int cy0 = ylo / f, cx0 = xlo / f, cy1 = (yhi - 1) / f, cx1 = (xhi - 1) / f;
    const int cxs = cx0 & ~3;
    if (phase == 0) {
        const long long chw = (long long)Hc * Wc;
        const float* src = g.q + ((long long)b * g.K + (MIX ? 0 : k)) * chw;
        const float* G = MIX ? mx->m + c * PSF_MAXK : nullptr;
        const int nq = (cx1 - cxs) / 4 + 1, qrows = cy1 - cy0 + 1;
        for (int idx = tid; idx < qrows * nq; idx += PSF_THREADS) {
            const int row = idx / nq, qd = idx % nq;
            const int gy = cy0 + row, gx = cxs + 4 * qd;
            const long long at = (long long)gy * Wc + gx;
            psf_f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (VECQ) {                                             // gx <= cx1 < Wc, Wc % 4 == 0: a whole quad
                if (MIX) v = psf_mix_quads(src + at, chw, G, g.K);
                else v = *reinterpret_cast<const psf_f4*>(src + at);
            } else {
                for (int j = 0; j < 4; ++j)
                    if (gx + j < Wc) {
                        if (MIX) {
                            float u = G[0] * src[at + j];
                            for (int kk = 1; kk < g.K; ++kk) {
                                const float pr = G[kk] * src[kk * chw + at + j];
                                u = u + pr;
                            }
                            v[j] = u;
                        } else {
                            v[j] = src[at + j];
                        }
                    }
            }
            *reinterpret_cast<psf_f4*>(s.qs + row * PSF_PITCH + 4 * qd) = v;
        }
        if (tid < cols) s.nh[tid] = psf_norm_rev(tt.x, rx, x0 - rx + tid, g.W);
        else if (tid >= 64 && tid < 64 + rows) s.nv[tid - 64] = psf_norm_rev(tt.y, ry, y0 - ry + tid - 64, g.H);
    } else if (phase == 1) {
        for (int idx = tid; idx < rows * cols; idx += PSF_THREADS) {
            const int wy = idx / cols, wx = idx % cols;
            const int gy = y0 - ry + wy, gx = x0 - rx + wx;
            float wv = 0.0f;
            if (gy >= 0 && gy < g.H && gx >= 0 && gx < g.W) {
                const float qv = s.qs[(gy / f - cy0) * PSF_PITCH + (gx / f - cxs)];
                const float ts = qv * g.step;
                const float n = s.nv[wy] * s.nh[wx];
                wv = ts / n;
            }
            s.w[wy * PSF_ROWS + wx] = wv;
        }
    } else if (phase == 2) {
        for (int idx = tid; idx < rows * ft; idx += PSF_THREADS) {
            const int row = idx / ft, x = idx % ft;
            s.hbuf[row * PSF_MAXT + x] = psf_conv_loop(tt.x, rx, s.w + row * PSF_ROWS + x, 1);
        }
    } else {
        for (int idx = tid; idx < ft * ft; idx += PSF_THREADS) {          // (w is dead: the blur goes where it was, pitch PSF_MAXT)
            const int y = idx / ft, x = idx % ft;
            s.w[y * PSF_MAXT + x] = psf_conv_loop(tt.y, ry, s.hbuf + y * PSF_MAXT + x, PSF_MAXT);
        }
    }
}
