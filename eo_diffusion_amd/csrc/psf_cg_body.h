// The bodies of the coarse-grid conjugate-gradient kernels (csrc/psf_cg.hip), one phase of one tile for one thread at a
// time, in the manner of psf_body.h: the kernels call the phases in order with a barrier after each, a host program does the same with a loop
// over the 256 thread numbers (tests/psf_cg_host_check.cc, under the address and undefined-behaviour sanitizers).  Nothing here needs the HIP
// headers.
//
// A workgroup of 256 threads owns a tile of 32 x 32 coarse pixels of one plane (sample b, observed channel k).  In every kernel thread tid owns
// the four pixels (row tid / 8, columns 4 (tid % 8) .. + 3) of the tile, in BOTH access forms: VECQ moves them as one 16-byte quad, the
// element-wise form one by one, so a tile's partial sum has one order whatever the alignment.
#pragma once
#include <stdint.h>

#ifndef PSF_FN
#define PSF_FN static inline
#endif

#define CG_THREADS 256
#define CG_T 32                            // tile edge in coarse pixels
#define CG_MAXB 24                         // half-width of a Gram table: ceil(2 r / f) at f = 1, r = 12
#define CG_NB (2 * CG_MAXB + 1)            // 49 entries of a Gram row (an odd LDS pitch: no bank conflicts across a tile's columns)
#define CG_ROWS (CG_T + 2 * CG_MAXB)       // 80: a tile with its halo
#define CG_PITCH 84                        // 80 + up to 3 leading columns (the patch is filled by aligned quads), rounded up to a quad
#define CG_MAX_ITERS 64

typedef float cg_f4 __attribute__((ext_vector_type(4)));

struct CgArgs {
    const float* d;       // gram: d, or the previous d when r is given; update: d
    const float* r;       // gram: NULL, or r: the tile is staged as d_new = r + beta * d and its interior written to d_out
    const float* mask;    // NULL or [B or 1][K or 1][Hc][Wc], entries 0 or 1
    const float* gy;      // [Hc][2b + 1]
    const float* gx;      // [Wc][2b + 1]
    const float* c;       // init: the right-hand side
    float* q;             // gram: out; update: in
    float* d_out;         // gram with r
    float* z;             // init / update: in and out; final: in
    float* rr;            // init / update: r, in and out
    float* q_out;         // final
    double* slots;        // one partial per (plane, tile)
    double* rho;          // per plane
    float* alpha;         // per plane
    float* beta;          // per plane
    int* ok;              // per plane: this iteration's alpha was formed (not guarded)
    double* sigma_out;    // eod_psf_gram: per plane
    float mu, lambda;
    int b, B, K, Hc, Wc, mask_b1, mask_c1;
    int tiles_x, tiles_y;
};

struct CgLds {
    float patch[CG_ROWS * CG_PITCH];  // u = m * d over the tile and its halo, out-of-plane 0
    float tbuf[CG_ROWS * CG_T];       // the row pass
    float dn[CG_T * CG_T];            // d over the tile
    float sgx[CG_T * CG_NB];          // the tile's rows of gx and gy
    float sgy[CG_T * CG_NB];
};

struct CgSumLds {
    double part[CG_THREADS];
};

struct CgTile {
    long long plane;
    int tile, y0, x0;
};
PSF_FN CgTile cg_tile_of(const CgArgs& g, long long item) {
    const long long tiles = (long long)g.tiles_x * g.tiles_y;
    CgTile t;
    t.plane = item / tiles;
    t.tile = (int)(item % tiles);
    t.y0 = (t.tile / g.tiles_x) * CG_T;
    t.x0 = (t.tile % g.tiles_x) * CG_T;
    return t;
}
PSF_FN const float* cg_mask_plane(const CgArgs& g, long long plane) {
    if (!g.mask) return nullptr;
    const long long bb = plane / g.K, k = plane % g.K;
    return g.mask + ((g.mask_b1 ? 0 : bb) * (g.mask_c1 ? 1 : g.K) + (g.mask_c1 ? 0 : k)) * ((long long)g.Hc * g.Wc);
}
PSF_FN bool cg_finite(double v) { return v - v == 0.0; }

// entries in ascending order over u[0], u[stride], ...: the contract's row and column pass
PSF_FN float cg_band(const float* gr, int n, const float* u, int stride) {
    float acc = gr[0] * u[0];
    for (int j = 1; j < n; ++j) {
        const float pr = gr[j] * u[j * stride];
        acc = acc + pr;
    }
    return acc;
}

// ------------------------------------------------------------------------------------------------ q = m * G(m * d) + mu * d, <d, q>
// phase 0: the patch (with r: d_new = r + beta * d first, its interior to d_out), dn and the Gram rows;  1: the row pass;
// phase 2: the column pass, q, the store; returns the thread's share of <d, q> in float64 (0.0 in the other phases)
template <bool VECQ, bool FUSE>
PSF_FN double psf_cg_gram_phase(int phase, const CgArgs& g, CgLds& s, long long item, int tid) {
    const CgTile tl = cg_tile_of(g, item);
    const int b = g.b, nb = 2 * b + 1, y0 = tl.y0, x0 = tl.x0;
    const int rows = CG_T + 2 * b;
    const int xs = (x0 - b) & ~3;            // the patch starts at a quad boundary at or left of x0 - b (negative: still a multiple of 4)
    const int lead = x0 - b - xs;
    const long long chw = (long long)g.Hc * g.Wc;
    const float* msk = cg_mask_plane(g, tl.plane);
    if (phase == 0) {
        const float* dsrc = g.d + tl.plane * chw;
        const float* rsrc = FUSE ? g.r + tl.plane * chw : nullptr;
        float* dout = FUSE ? g.d_out + tl.plane * chw : nullptr;
        const float beta = FUSE ? g.beta[tl.plane] : 0.0f;
        const int nq = (lead + CG_T + 2 * b + 3) / 4;
        for (int idx = tid; idx < rows * nq; idx += CG_THREADS) {
            const int row = idx / nq, qd = idx % nq;
            const int gy = y0 - b + row, gx = xs + 4 * qd;
            float dv[4] = {0.0f, 0.0f, 0.0f, 0.0f}, rv[4] = {0.0f, 0.0f, 0.0f, 0.0f}, mv[4] = {1.0f, 1.0f, 1.0f, 1.0f};
            bool in[4] = {false, false, false, false};
            const long long at = (long long)gy * g.Wc + gx;
            if (gy >= 0 && gy < g.Hc) {
                if (VECQ) {
                    if (gx >= 0 && gx < g.Wc) {                  // Wc % 4 == 0: a whole quad
                        const cg_f4 d4 = *reinterpret_cast<const cg_f4*>(dsrc + at);
                        dv[0] = d4[0]; dv[1] = d4[1]; dv[2] = d4[2]; dv[3] = d4[3];
                        if (FUSE) { const cg_f4 r4 = *reinterpret_cast<const cg_f4*>(rsrc + at); rv[0] = r4[0]; rv[1] = r4[1]; rv[2] = r4[2]; rv[3] = r4[3]; }
                        if (msk) { const cg_f4 m4 = *reinterpret_cast<const cg_f4*>(msk + at); mv[0] = m4[0]; mv[1] = m4[1]; mv[2] = m4[2]; mv[3] = m4[3]; }
                        in[0] = in[1] = in[2] = in[3] = true;
                    }
                } else {
                    for (int j = 0; j < 4; ++j)
                        if (gx + j >= 0 && gx + j < g.Wc) {
                            in[j] = true;
                            dv[j] = dsrc[at + j];
                            if (FUSE) rv[j] = rsrc[at + j];
                            if (msk) mv[j] = msk[at + j];
                        }
                }
            }
            float dn[4];
            cg_f4 u4 = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int j = 0; j < 4; ++j) {
                dn[j] = 0.0f;
                if (!in[j]) continue;
                if (FUSE) {
                    const float bd = beta * dv[j];
                    dn[j] = rv[j] + bd;
                } else {
                    dn[j] = dv[j];
                }
                u4[j] = msk ? mv[j] * dn[j] : dn[j];
            }
            *reinterpret_cast<cg_f4*>(s.patch + row * CG_PITCH + 4 * qd) = u4;
            const int ty = gy - y0, tx = gx - x0;                // tx is a multiple of 4: a quad lies in the tile or in its halo as a whole
            if (ty >= 0 && ty < CG_T && tx >= 0 && tx < CG_T) {
                for (int j = 0; j < 4; ++j) s.dn[ty * CG_T + tx + j] = dn[j];
                if (FUSE) {
                    if (VECQ) {
                        if (in[0]) { const cg_f4 o = {dn[0], dn[1], dn[2], dn[3]}; *reinterpret_cast<cg_f4*>(dout + at) = o; }
                    } else {
                        for (int j = 0; j < 4; ++j)
                            if (in[j]) dout[at + j] = dn[j];
                    }
                }
            }
        }
        for (int idx = tid; idx < CG_T * nb; idx += CG_THREADS) {
            const int l = idx / nb, j = idx % nb;
            s.sgx[l * CG_NB + j] = x0 + l < g.Wc ? g.gx[(long long)(x0 + l) * nb + j] : 0.0f;
            s.sgy[l * CG_NB + j] = y0 + l < g.Hc ? g.gy[(long long)(y0 + l) * nb + j] : 0.0f;
        }
        return 0.0;
    }
    if (phase == 1) {
        for (int idx = tid; idx < rows * CG_T; idx += CG_THREADS) {
            const int row = idx / CG_T, xl = idx % CG_T;
            s.tbuf[row * CG_T + xl] = cg_band(s.sgx + xl * CG_NB, nb, s.patch + row * CG_PITCH + lead + xl, 1);
        }
        return 0.0;
    }
    const int ty = tid / 8, tx = (tid % 8) * 4;
    const int gy = y0 + ty, gx = x0 + tx;
    if (gy >= g.Hc || gx >= g.Wc) return 0.0;
    const long long at = (long long)gy * g.Wc + gx;
    float* dst = g.q + tl.plane * chw;
    float o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    double part = 0.0;
    for (int j = 0; j < 4; ++j) {
        if (gx + j >= g.Wc) break;                               // (VECQ: never)
        const float col = cg_band(s.sgy + ty * CG_NB, nb, s.tbuf + ty * CG_T + tx + j, CG_T);
        const float dj = s.dn[ty * CG_T + tx + j];
        const float mq = msk ? msk[at + j] * col : col;
        const float md = g.mu * dj;
        o[j] = mq + md;
        part += (double)dj * (double)o[j];
    }
    if (VECQ) {
        const cg_f4 o4 = {o[0], o[1], o[2], o[3]};
        *reinterpret_cast<cg_f4*>(dst + at) = o4;
    } else {
        for (int j = 0; j < 4 && gx + j < g.Wc; ++j) dst[at + j] = o[j];
    }
    return part;
}

// ------------------------------------------------------------------------------------------------ the elementwise kernels
// mode 0: z = 0, r = c, returns the share of <c, c>;  1: z += alpha d, r -= alpha q, returns the share of <r, r>;  2: q_out = lambda * (m * z)
template <bool VECQ>
PSF_FN double psf_cg_elem(int mode, const CgArgs& g, long long item, int tid) {
    const CgTile tl = cg_tile_of(g, item);
    const int ty = tid / 8, tx = (tid % 8) * 4;
    const int gy = tl.y0 + ty, gx = tl.x0 + tx;
    if (gy >= g.Hc || gx >= g.Wc) return 0.0;
    const long long chw = (long long)g.Hc * g.Wc;
    const long long at = tl.plane * chw + (long long)gy * g.Wc + gx;
    const int n = VECQ ? 4 : (g.Wc - gx < 4 ? g.Wc - gx : 4);
    float a[4] = {0.0f, 0.0f, 0.0f, 0.0f}, e[4] = {0.0f, 0.0f, 0.0f, 0.0f}, zv[4] = {0.0f, 0.0f, 0.0f, 0.0f}, rv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    double part = 0.0;
#define CG_LOAD(dst, src)                                                                                          \
    do {                                                                                                           \
        if (VECQ) { const cg_f4 v4 = *reinterpret_cast<const cg_f4*>((src) + at); dst[0] = v4[0]; dst[1] = v4[1]; dst[2] = v4[2]; dst[3] = v4[3]; } \
        else for (int j = 0; j < n; ++j) dst[j] = (src)[at + j];                                                   \
    } while (0)
#define CG_STORE(dst, src)                                                                                         \
    do {                                                                                                           \
        if (VECQ) { const cg_f4 v4 = {src[0], src[1], src[2], src[3]}; *reinterpret_cast<cg_f4*>((dst) + at) = v4; } \
        else for (int j = 0; j < n; ++j) (dst)[at + j] = src[j];                                                   \
    } while (0)
    if (mode == 0) {
        CG_LOAD(a, g.c);
        for (int j = 0; j < n; ++j) part += (double)a[j] * (double)a[j];
        CG_STORE(g.rr, a);
        CG_STORE(g.z, zv);
    } else if (mode == 1) {
        const float alpha = g.alpha[tl.plane];
        CG_LOAD(a, g.d);
        CG_LOAD(e, g.q);
        CG_LOAD(zv, g.z);
        CG_LOAD(rv, g.rr);
        for (int j = 0; j < n; ++j) {
            const float ad = alpha * a[j];
            zv[j] = zv[j] + ad;
            const float aq = alpha * e[j];
            rv[j] = rv[j] - aq;
            part += (double)rv[j] * (double)rv[j];
        }
        CG_STORE(g.z, zv);
        CG_STORE(g.rr, rv);
    } else {
        const float* msk = cg_mask_plane(g, tl.plane);
        const long long mat = (long long)gy * g.Wc + gx;
        CG_LOAD(zv, g.z);
        for (int j = 0; j < n; ++j) {
            const float mz = msk ? msk[mat + j] * zv[j] : zv[j];
            a[j] = g.lambda * mz;
        }
        CG_STORE(g.q_out, a);
    }
#undef CG_LOAD
#undef CG_STORE
    return part;
}

// ------------------------------------------------------------------------------------------------ a plane's total and its scalars
// One workgroup per plane.  phase 0: thread t adds the plane's tile partials t, t + 256, ... in ascending order;  phases 1 .. 8: a tree over
// the thread number, strides 128 .. 1;  phase 9, thread 0: mode 0 sigma_out = total;  1 rho = total;  2 alpha = rho / total (sigma);
// 3 beta = total (rho') / rho, rho = total.  alpha = beta = 0 when rho == 0, sigma <= 0 or either is not finite.
PSF_FN void psf_cg_sum_phase(int phase, int mode, const CgArgs& g, CgSumLds& s, long long plane, int tid) {
    const long long tiles = (long long)g.tiles_x * g.tiles_y;
    if (phase == 0) {
        double acc = 0.0;
        for (long long t = tid; t < tiles; t += CG_THREADS) acc += g.slots[plane * tiles + t];
        s.part[tid] = acc;
    } else if (phase <= 8) {
        const int stride = 256 >> phase;
        if (tid < stride) s.part[tid] += s.part[tid + stride];
    } else if (tid == 0) {
        const double total = s.part[0];
        if (mode == 0) {
            g.sigma_out[plane] = total;
        } else if (mode == 1) {
            g.rho[plane] = total;
        } else if (mode == 2) {
            const double rho = g.rho[plane];
            const bool ok = cg_finite(rho) && cg_finite(total) && rho != 0.0 && total > 0.0;
            g.alpha[plane] = ok ? (float)(rho / total) : 0.0f;
            g.ok[plane] = ok ? 1 : 0;
        } else {
            const double rho = g.rho[plane];
            const bool ok = g.ok[plane] != 0 && cg_finite(total);
            g.beta[plane] = ok ? (float)(total / rho) : 0.0f;
            g.rho[plane] = total;
        }
    }
}

// a tile's partial from its 256 thread shares: a butterfly over each wave of 64 (lane i takes v[i] + v[i ^ o], o = 32, 16, .. 1), then the four
// waves in wave order.  The kernels do it with shuffles (psf_cg.hip); this is the same order over an array, for the host.
PSF_FN double psf_cg_tile_sum_host(const double* part) {
    double w[4];
    for (int wave = 0; wave < 4; ++wave) {
        double v[64], n[64];
        for (int i = 0; i < 64; ++i) v[i] = part[wave * 64 + i];
        for (int o = 32; o > 0; o >>= 1) {
            for (int i = 0; i < 64; ++i) n[i] = v[i] + v[i ^ o];
            for (int i = 0; i < 64; ++i) v[i] = n[i];
        }
        w[wave] = v[0];
    }
    return ((w[0] + w[1]) + w[2]) + w[3];
}
