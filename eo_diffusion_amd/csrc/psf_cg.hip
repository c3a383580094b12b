// The exact PSF data-consistency solve (no reference line): conjugate gradients on the coarse grid for
// S z = c, S = M G M + mu I, G = A A^T = G_H (x) G_W the separable banded Gram matrix of section 9.7's A = D_f N^-1 B0, one independent
// system per plane (sample b, observed channel k).  The per-pixel contract is in include/eodiff.h; this file is built with -ffp-contract=off.
// The bodies live in psf_cg_body.h (one phase of one tile for one thread), so that a host program can run them as well.
//
// Launches: init (z = 0, r = c, <c, c> partials), plane totals; per iteration gram (q = S d with d = r + beta d formed while the tile is
// staged, <d, q> partials), plane totals -> alpha, update (z += alpha d, r -= alpha q, <r, r> partials), plane totals -> beta; final
// (q_out = lambda m z): 4 iters + 2 (the last iteration forms no beta).  Every partial goes to a slot indexed by (plane, tile) and a plane's total is a fixed tree over the tile
// index, so a plane's scalars depend on that plane alone: no atomics, no counters, nothing on the host.  Work items (plane, tile) beyond
// EOD_PSF_GRID_BLOCKS are taken by striding.  VECQ: 16-byte accesses (Wc % 4 == 0 and every pointer of the launch aligned).
#include <initializer_list>

#include "common.h"

#define PSF_FN __device__ __host__ __forceinline__
#include "psf_cg_body.h"

// the tile's partial from the threads' shares: a butterfly over each wave, then the four waves in wave order; thread 0 writes the slot
__device__ __forceinline__ void cg_tile_sum(double v, double* wsum, double* slot) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) *slot = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    __syncthreads();
}

template <bool VECQ, bool FUSE>
__global__ void __launch_bounds__(CG_THREADS) psf_cg_gram_kernel(CgArgs g, long long items) {
    __shared__ CgLds s;
    __shared__ double wsum[4];
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        psf_cg_gram_phase<VECQ, FUSE>(0, g, s, item, threadIdx.x);
        __syncthreads();
        psf_cg_gram_phase<VECQ, FUSE>(1, g, s, item, threadIdx.x);
        __syncthreads();
        const double part = psf_cg_gram_phase<VECQ, FUSE>(2, g, s, item, threadIdx.x);
        cg_tile_sum(part, wsum, g.slots + item);
    }
}

template <bool VECQ>
__global__ void __launch_bounds__(CG_THREADS) psf_cg_elem_kernel(CgArgs g, int mode, long long items) {
    __shared__ double wsum[4];
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const double part = psf_cg_elem<VECQ>(mode, g, item, threadIdx.x);
        if (mode != 2) cg_tile_sum(part, wsum, g.slots + item);
    }
}

__global__ void __launch_bounds__(CG_THREADS) psf_cg_sum_kernel(CgArgs g, int mode, long long planes) {
    __shared__ CgSumLds s;
    for (long long plane = blockIdx.x; plane < planes; plane += gridDim.x) {
        for (int phase = 0; phase <= 9; ++phase) {
            psf_cg_sum_phase(phase, mode, g, s, plane, threadIdx.x);
            __syncthreads();
        }
    }
}

static inline bool cg_overlap(const void* a, long long na, const void* b, long long nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}
static inline int cg_grid(long long items) { return (int)(items < EOD_PSF_GRID_BLOCKS ? items : EOD_PSF_GRID_BLOCKS); }
static inline long long cg_round4(long long n) { return (n + 3) / 4 * 4; }

struct CgWs {
    float *z, *r, *d0, *d1, *q, *alpha, *beta;
    double *slots, *rho;
    int* ok;
};

static long long cg_ws_bytes(long long P, long long chw, long long tiles) {
    return 16 + 5 * cg_round4(P * chw) * 4 + 8 * (P * tiles + P) + 4 * 3 * cg_round4(P);
}
static CgWs cg_ws_layout(void* ws, long long P, long long chw, long long tiles) {
    char* base = (char*)(((uintptr_t)ws + 15u) & ~(uintptr_t)15u);
    const long long n = cg_round4(P * chw);
    CgWs w;
    w.z = (float*)base;
    w.r = w.z + n;
    w.d0 = w.r + n;
    w.d1 = w.d0 + n;
    w.q = w.d1 + n;
    w.slots = (double*)(w.q + n);
    w.rho = w.slots + P * tiles;
    w.alpha = (float*)(w.rho + P);
    w.beta = w.alpha + cg_round4(P);
    w.ok = (int*)(w.beta + cg_round4(P));
    return w;
}

extern "C" int64_t eod_psf_cg_workspace_size(int B, int K, int Hc, int Wc) {
    if (B <= 0 || K <= 0 || Hc <= 0 || Wc <= 0) return -1;
    const long long tiles = (long long)((Hc + CG_T - 1) / CG_T) * ((Wc + CG_T - 1) / CG_T);
    return cg_ws_bytes((long long)B * K, (long long)Hc * Wc, tiles);
}

// what the two entry points share: the geometry, the refusals, the workspace
static int cg_common(const char* what, CgArgs& g, const void* in, void* out, void* ws, long long ws_bytes, CgWs& w, long long& items) {
    EOD_REQUIRE(in && out && g.gy && g.gx && ws, "%s: bad args (a null pointer)", what);
    EOD_REQUIRE(g.B > 0 && g.K > 0 && g.Hc > 0 && g.Wc > 0, "%s: bad args (B, K, Hc, Wc must be positive)", what);
    EOD_REQUIRE(g.b >= 0 && g.b <= CG_MAXB, "%s: the half-width b = %d is outside 0 .. %d", what, g.b, CG_MAXB);
    EOD_REQUIRE(g.mu - g.mu == 0.0f && g.mu >= 0.0f, "%s: mu must be finite and >= 0, got %g", what, (double)g.mu);
    g.tiles_x = (g.Wc + CG_T - 1) / CG_T;
    g.tiles_y = (g.Hc + CG_T - 1) / CG_T;
    const long long P = (long long)g.B * g.K, chw = (long long)g.Hc * g.Wc, tiles = (long long)g.tiles_x * g.tiles_y;
    const long long need = cg_ws_bytes(P, chw, tiles);
    EOD_REQUIRE(ws_bytes >= need, "%s: the workspace has %lld bytes, eod_psf_cg_workspace_size asks for %lld", what, ws_bytes, need);
    const long long nb = 2 * g.b + 1, nin = P * chw * 4, nmask = (long long)(g.mask_b1 ? 1 : g.B) * (g.mask_c1 ? 1 : g.K) * chw * 4;
    const void* ins[4] = {in, g.mask, g.gy, g.gx};
    const long long nins[4] = {nin, nmask, g.Hc * nb * 4, g.Wc * nb * 4};
    for (int i = 0; i < 4; ++i) {
        if (!ins[i]) continue;
        EOD_REQUIRE(!cg_overlap(out, nin, ins[i], nins[i]), "%s: the output overlaps an input", what);
        EOD_REQUIRE(!cg_overlap(ws, ws_bytes, ins[i], nins[i]), "%s: the workspace overlaps an input", what);
    }
    EOD_REQUIRE(!cg_overlap(ws, ws_bytes, out, nin), "%s: the workspace overlaps the output", what);
    w = cg_ws_layout(ws, P, chw, tiles);
    g.slots = w.slots;
    g.rho = w.rho;
    g.alpha = w.alpha;
    g.beta = w.beta;
    g.ok = w.ok;
    items = P * tiles;
    return EOD_OK;
}

static inline bool cg_vecq(const CgArgs& g, std::initializer_list<const void*> ptrs) {
    if (g.Wc % 4) return false;
    for (const void* p : ptrs)
        if (p && !eod_aligned16(p)) return false;
    return true;
}

static void cg_launch_gram(const CgArgs& g, bool fuse, long long items, hipStream_t st) {
    const bool vq = cg_vecq(g, {g.d, g.r, g.mask, g.q, g.d_out});
    const dim3 grid(cg_grid(items)), block(CG_THREADS);
    if (vq && fuse) hipLaunchKernelGGL((psf_cg_gram_kernel<true, true>), grid, block, 0, st, g, items);
    else if (vq) hipLaunchKernelGGL((psf_cg_gram_kernel<true, false>), grid, block, 0, st, g, items);
    else if (fuse) hipLaunchKernelGGL((psf_cg_gram_kernel<false, true>), grid, block, 0, st, g, items);
    else hipLaunchKernelGGL((psf_cg_gram_kernel<false, false>), grid, block, 0, st, g, items);
}
static void cg_launch_elem(const CgArgs& g, int mode, bool vq, long long items, hipStream_t st) {
    const dim3 grid(cg_grid(items)), block(CG_THREADS);
    if (vq) hipLaunchKernelGGL((psf_cg_elem_kernel<true>), grid, block, 0, st, g, mode, items);
    else hipLaunchKernelGGL((psf_cg_elem_kernel<false>), grid, block, 0, st, g, mode, items);
}
static void cg_launch_sum(const CgArgs& g, int mode, hipStream_t st) {
    const long long planes = (long long)g.B * g.K;
    hipLaunchKernelGGL(psf_cg_sum_kernel, dim3(cg_grid(planes)), dim3(CG_THREADS), 0, st, g, mode, planes);
}

extern "C" int eod_psf_gram(const float* d, const float* mask, float mu, const float* gy, const float* gx, int b, int B, int K, int Hc, int Wc,
                            int mask_b1, int mask_c1, float* q, double* sigma, void* ws, int64_t ws_bytes, void* stream) {
    const char* what = "psf_gram";
    CgArgs g;
    memset(&g, 0, sizeof(g));
    g.d = d; g.mask = mask; g.gy = gy; g.gx = gx; g.q = q; g.sigma_out = sigma; g.mu = mu;
    g.b = b; g.B = B; g.K = K; g.Hc = Hc; g.Wc = Wc; g.mask_b1 = mask_b1; g.mask_c1 = mask_c1;
    EOD_REQUIRE(sigma, "%s: bad args (a null pointer)", what);
    CgWs w;
    long long items;
    const int rc = cg_common(what, g, d, q, ws, ws_bytes, w, items);
    if (rc != EOD_OK) return rc;
    const long long P = (long long)B * K;
    EOD_REQUIRE(((uintptr_t)sigma & 7u) == 0, "%s: sigma must be 8-byte aligned", what);
    EOD_REQUIRE(!cg_overlap(sigma, P * 8, d, P * Hc * Wc * 4) && !cg_overlap(sigma, P * 8, q, P * Hc * Wc * 4) && !cg_overlap(sigma, P * 8, ws, ws_bytes),
                "%s: sigma overlaps another buffer", what);
    hipStream_t st = (hipStream_t)stream;
    cg_launch_gram(g, false, items, st);
    cg_launch_sum(g, 0, st);
    EOD_CHECK_LAUNCH(what);
    return EOD_OK;
}

extern "C" int eod_psf_cg(const float* c, const float* mask, float mu, float lambda, const float* gy, const float* gx, int b, int iters, int B,
                          int K, int Hc, int Wc, int mask_b1, int mask_c1, float* q_out, void* ws, int64_t ws_bytes, void* stream) {
    const char* what = "psf_cg";
    CgArgs g;
    memset(&g, 0, sizeof(g));
    g.c = c; g.mask = mask; g.gy = gy; g.gx = gx; g.q_out = q_out; g.mu = mu; g.lambda = lambda;
    g.b = b; g.B = B; g.K = K; g.Hc = Hc; g.Wc = Wc; g.mask_b1 = mask_b1; g.mask_c1 = mask_c1;
    EOD_REQUIRE(iters >= 1 && iters <= CG_MAX_ITERS, "%s: iters = %d is outside 1 .. %d", what, iters, CG_MAX_ITERS);
    EOD_REQUIRE(lambda >= 0.0f && lambda <= 1.0f, "%s: lambda must lie in [0, 1], got %g", what, (double)lambda);
    CgWs w;
    long long items;
    const int rc = cg_common(what, g, c, q_out, ws, ws_bytes, w, items);
    if (rc != EOD_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    g.z = w.z; g.rr = w.r; g.q = w.q;
    cg_launch_elem(g, 0, cg_vecq(g, {c}), items, st);                         // z = 0, r = c, <c, c>
    cg_launch_sum(g, 1, st);                                                  // rho
    const float* dcur = c;                                                    // d = c: the first pass reads the right-hand side itself
    for (int it = 0; it < iters; ++it) {
        if (it == 0) {
            g.d = c; g.r = nullptr; g.d_out = nullptr;
        } else {                                                              // d = r + beta d, formed while the tile is staged
            float* dnew = dcur == w.d0 ? w.d1 : w.d0;
            g.d = dcur; g.r = w.r; g.d_out = dnew;
            dcur = dnew;
        }
        cg_launch_gram(g, it != 0, items, st);                                // q = S d, <d, q>
        cg_launch_sum(g, 2, st);                                              // alpha
        g.d = dcur; g.r = nullptr; g.d_out = nullptr;
        cg_launch_elem(g, 1, cg_vecq(g, {dcur}), items, st);                  // z += alpha d, r -= alpha q, <r, r>
        if (it + 1 < iters) cg_launch_sum(g, 3, st);                          // beta, rho (the last iteration needs neither)
    }
    cg_launch_elem(g, 2, cg_vecq(g, {mask, q_out}), items, st);              // q_out = lambda (m z)
    EOD_CHECK_LAUNCH(what);
    return EOD_OK;
}
