// PSF-aware observations (no reference line): A = D_f N^-1 B0, B0 the zero-padded separable convolution with the
// symmetric taps h[0 .. 2r] (horizontal, then vertical), N = diag(B0 1), D_f the f x f block mean of section 9.5.  One Landweber step of
// data consistency is two launches: eod_psf_residual (q = lm * (A p - values), on the coarse grid) and eod_psf_update (out = p - A^T q
// scaled by step).  The per-pixel contract is in include/eodiff.h; this file is built with -ffp-contract=off, every operation is rounded
// once.  The bodies live in psf_body.h (one phase of one tile for one thread), so that a host program can run them as well.
//
// A workgroup of 256 threads owns a tile of tc x tc coarse pixels = ft x ft pixels, ft = tc * f <= 32 (psf_tile_coarse: tc a multiple of
// 4, so a tile starts at a quad of both grids).  It stages the tile and its halo of r pixels in LDS with out-of-plane lanes zero, runs
// the horizontal pass into a second buffer, then the vertical pass.  Work items (plane, tile) beyond EOD_PSF_GRID_BLOCKS are taken by
// striding.  Taps, the channel list and its inverse travel by value in the kernel arguments; nothing is allocated, copied or
// synchronised.  VEC: 16-byte accesses of the full-resolution tensors (W % 4 == 0, pointers aligned); VECQ: of the coarse ones
// (W / f % 4 == 0, pointers aligned); the element-wise forms run the same arithmetic.  Two more kernel pairs follow: the same through a
// band mix (section 9.10, eod_psf_*_mix) and the general form of section 9.11, one tap vector per axis, asymmetric taps allowed, a halo of
// ry rows and rx columns (eod_psf_*_xy).  The host side is written once for all nine entry points: psf_common, a residual launcher and an
// update launcher.
#include "common.h"

#define PSF_FN __device__ __host__ __forceinline__
#include "psf_body.h"

template <bool VEC, bool VECQ>
__global__ void __launch_bounds__(PSF_THREADS) psf_residual_kernel(PsfArgs g, PsfTaps t, long long items) {
    __shared__ PsfResLds s;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        psf_residual_phase<VEC, VECQ>(0, g, t, s, item, threadIdx.x);
        __syncthreads();
        psf_residual_phase<VEC, VECQ>(1, g, t, s, item, threadIdx.x);
        __syncthreads();
        psf_residual_phase<VEC, VECQ>(2, g, t, s, item, threadIdx.x);
        __syncthreads();
        psf_residual_phase<VEC, VECQ>(3, g, t, s, item, threadIdx.x);
        __syncthreads();
    }
}

template <bool VEC, bool VECQ>
__global__ void __launch_bounds__(PSF_THREADS) psf_update_kernel(PsfArgs g, PsfTaps t, long long items) {
    __shared__ PsfUpdLds s;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        psf_update_phase<VEC, VECQ>(0, g, t, s, item, threadIdx.x);
        __syncthreads();
        psf_update_phase<VEC, VECQ>(1, g, t, s, item, threadIdx.x);
        __syncthreads();
        psf_update_phase<VEC, VECQ>(2, g, t, s, item, threadIdx.x);
        __syncthreads();
        psf_update_phase<VEC, VECQ>(3, g, t, s, item, threadIdx.x);
        __syncthreads();
        psf_update_phase<VEC, VECQ>(4, g, t, s, item, threadIdx.x);
        __syncthreads();
    }
}

template <bool VEC, bool VECQ>
__global__ void __launch_bounds__(PSF_THREADS) psf_residual_mix_kernel(PsfArgs g, PsfTaps t, PsfMix mx, long long items) {
    __shared__ PsfResLds s;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        psf_residual_mix_phase<VEC, VECQ>(0, g, t, mx, s, item, threadIdx.x);
        __syncthreads();
        psf_residual_mix_phase<VEC, VECQ>(1, g, t, mx, s, item, threadIdx.x);
        __syncthreads();
        psf_residual_mix_phase<VEC, VECQ>(2, g, t, mx, s, item, threadIdx.x);
        __syncthreads();
        psf_residual_mix_phase<VEC, VECQ>(3, g, t, mx, s, item, threadIdx.x);
        __syncthreads();
    }
}

template <bool VEC, bool VECQ>
__global__ void __launch_bounds__(PSF_THREADS) psf_update_mix_kernel(PsfArgs g, PsfTaps t, PsfMix mx, long long items) {
    __shared__ PsfUpdLds s;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        psf_update_mix_phase<VEC, VECQ>(0, g, t, mx, s, item, threadIdx.x);
        __syncthreads();
        psf_update_mix_phase<VEC, VECQ>(1, g, t, mx, s, item, threadIdx.x);
        __syncthreads();
        psf_update_mix_phase<VEC, VECQ>(2, g, t, mx, s, item, threadIdx.x);
        __syncthreads();
        psf_update_mix_phase<VEC, VECQ>(3, g, t, mx, s, item, threadIdx.x);
        __syncthreads();
        psf_update_mix_phase<VEC, VECQ>(4, g, t, mx, s, item, threadIdx.x);
        __syncthreads();
    }
}

// One tap vector per axis: the same tile, access forms and stride loop; the halo is ry rows and rx columns.  One
// kernel per pair serves the plain and the mixed form (MIX: the matrix by value; the plain form passes it zeroed and never reads it).
template <bool VEC, bool VECQ, bool MIX>
__global__ void __launch_bounds__(PSF_THREADS) psf_residual_xy_kernel(PsfArgs g, PsfTapsXy tt, PsfMix mx, long long items) {
    __shared__ PsfResLds s;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        psf_residual_xy_phase<VEC, VECQ, MIX>(0, g, tt, &mx, s, item, threadIdx.x);
        __syncthreads();
        psf_residual_xy_phase<VEC, VECQ, MIX>(1, g, tt, &mx, s, item, threadIdx.x);
        __syncthreads();
        psf_residual_xy_phase<VEC, VECQ, MIX>(2, g, tt, &mx, s, item, threadIdx.x);
        __syncthreads();
        psf_residual_xy_phase<VEC, VECQ, MIX>(3, g, tt, &mx, s, item, threadIdx.x);
        __syncthreads();
    }
}

template <bool VEC, bool VECQ, bool MIX>
__global__ void __launch_bounds__(PSF_THREADS) psf_update_xy_kernel(PsfArgs g, PsfTapsXy tt, PsfMix mx, long long items) {
    __shared__ PsfUpdLds s;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        psf_update_xy_phase<VEC, VECQ, MIX>(0, g, tt, &mx, s, item, threadIdx.x);
        __syncthreads();
        psf_update_xy_phase<VEC, VECQ, MIX>(1, g, tt, &mx, s, item, threadIdx.x);
        __syncthreads();
        psf_update_xy_phase<VEC, VECQ, MIX>(2, g, tt, &mx, s, item, threadIdx.x);
        __syncthreads();
        psf_update_xy_phase<VEC, VECQ, MIX>(3, g, tt, &mx, s, item, threadIdx.x);
        __syncthreads();
        psf_update_xy_phase<VEC, VECQ, MIX>(4, g, tt, &mx, s, item, threadIdx.x);
        __syncthreads();
    }
}

static inline bool psf_overlap(const float* a, long long na, const float* b, long long nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + (uintptr_t)nb * sizeof(float) && pb < pa + (uintptr_t)na * sizeof(float);
}

// where an entry point's taps and observed planes come from
struct PsfSource {
    const float *taps_y, *taps_x;  // forward taps; symmetric: taps_x alone, for both axes
    int ry, rx;
    const int32_t* channels;       // exactly one of the channel list and the matrix
    const float* M;
    bool symmetric;                // one vector, refused unless bitwise symmetric: the one-vector kernels
};
static PsfSource psf_one_vector(const float* taps, int r, const int32_t* channels, const float* M) { return {nullptr, taps, 0, r, channels, M, true}; }
static PsfSource psf_two_vectors(const float* taps_y, int ry, const float* taps_x, int rx, const int32_t* channels, const float* M) {
    return {taps_y, taps_x, ry, rx, channels, M, false};
}

// one axis' taps into t, forward or reversed.  axis names them in messages: "y" / "x", or "" for the one vector of both axes
static int psf_axis_taps(const char* what, const char* axis, PsfTaps& t, const float* taps, int r, bool symmetric, bool reversed) {
    const char* us = axis[0] ? "_" : "";
    EOD_REQUIRE(taps, "%s: bad args", what);
    EOD_REQUIRE(r >= 0 && r <= PSF_MAXR, "%s: the tap radius r%s = %d is outside 0 .. %d", what, axis, r, PSF_MAXR);
    const int n = 2 * r + 1;
    for (int i = 0; i < n; ++i) {
        const float h = taps[i];
        EOD_REQUIRE(h == h && h - h == 0.0f && h >= 0.0f && !__builtin_signbit(h), "%s: taps%s%s[%d] = %g is not a finite non-negative number", what, us, axis, i, (double)h);
        EOD_REQUIRE(!symmetric || memcmp(&taps[i], &taps[n - 1 - i], sizeof(float)) == 0, "%s: the taps are not symmetric (taps[%d] != taps[%d])", what, i, n - 1 - i);
        t.h[reversed ? n - 1 - i : i] = h;
    }
    for (int i = n; i < 2 * PSF_MAXR + 1; ++i) t.h[i] = 0.0f;
    EOD_REQUIRE(taps[r] > 0.0f, "%s: the centre tap%s%s must be positive", what, axis[0] ? " of taps_" : "", axis);
    return EOD_OK;
}

// What every entry point shares: the geometry into g; exactly one of the channel list and the matrix M (rows x cols, row pitch `pitch`
// inside PsfMix; with it the bands are 0 .. K - 1 and every channel takes its mix) into g / mx; the taps into tt, reversed for the update.
// src.symmetric: the one vector goes into tt.x and g.r (what the one-vector kernels take; tt.y stays zero).
static int psf_common(const char* what, PsfArgs& g, PsfTapsXy& tt, PsfMix& mx, const PsfSource& src, int rows, int cols, int pitch, bool reversed) {
    const int32_t* channels = src.channels;
    const float* M = src.M;
    const bool one = src.symmetric;
    EOD_REQUIRE((channels != nullptr) != (M != nullptr), "%s: %s", what, one ? "bad args" : "exactly one of the channel list and the matrix must be given");
    EOD_REQUIRE(g.p && g.out && g.B > 0 && g.C > 0 && g.H > 0 && g.W > 0, "%s: bad args", what);
    if (M) {
        EOD_REQUIRE(g.K >= 1 && g.K <= PSF_MAXK && g.K <= g.C, "%s: needs 1 <= K <= min(C, %d), got K = %d, C = %d", what, PSF_MAXK, g.K, g.C);
        EOD_REQUIRE(g.C <= PSF_MAXC, "%s: at most %d channels (the matrix travels by value), got %d", what, PSF_MAXC, g.C);
    } else {
        EOD_REQUIRE(g.C <= PSF_MAXC, "%s: at most %d channels (the channel list travels by value), got %d", what, PSF_MAXC, g.C);
        EOD_REQUIRE(g.K >= 1 && g.K <= g.C, "%s: K = %d observed channels is outside 1 .. C = %d", what, g.K, g.C);
    }
    EOD_REQUIRE(g.f >= 1 && g.f <= 8, "%s: f = %d is outside 1..8", what, g.f);
    EOD_REQUIRE(g.H % g.f == 0 && g.W % g.f == 0, "%s: f = %d does not divide %d x %d", what, g.f, g.H, g.W);
    for (int c = 0; c < PSF_MAXC; ++c) g.kof[c] = M ? 0 : -1;    // update with a matrix: no copied plane
    for (int k = 0; k < PSF_MAXC; ++k) g.ch[k] = 0;
    for (int i = 0; i < PSF_MAXK * PSF_MAXC; ++i) mx.m[i] = 0.0f;
    if (M) {
        for (int k = 0; k < g.K; ++k) g.ch[k] = (unsigned char)k;
        for (int i = 0; i < rows; ++i)
            for (int j = 0; j < cols; ++j) {
                const float v = M[i * cols + j];
                EOD_REQUIRE(v - v == 0.0f, "%s: entry [%d][%d] = %g of the matrix is not finite", what, i, j, (double)v);
                mx.m[i * pitch + j] = v;
            }
    } else {
        for (int k = 0; k < g.K; ++k) {
            EOD_REQUIRE(channels[k] >= 0 && channels[k] < g.C, "%s: channels[%d] = %d is outside 0 .. %d", what, k, channels[k], g.C - 1);
            EOD_REQUIRE(k == 0 || channels[k] > channels[k - 1], "%s: channels must be strictly increasing", what);
            g.ch[k] = (unsigned char)channels[k];
            g.kof[channels[k]] = (signed char)k;
        }
    }
    tt = PsfTapsXy();
    int rc = one ? EOD_OK : psf_axis_taps(what, "y", tt.y, src.taps_y, src.ry, false, reversed);
    if (rc != EOD_OK) return rc;
    rc = psf_axis_taps(what, one ? "" : "x", tt.x, src.taps_x, src.rx, one, reversed);
    if (rc != EOD_OK) return rc;
    tt.ry = one ? 0 : src.ry;
    tt.rx = src.rx;
    g.r = tt.ry > tt.rx ? tt.ry : tt.rx;
    g.tc = psf_tile_coarse(g.f);
    const int ft = g.tc * g.f;
    g.tiles_x = (g.W + ft - 1) / ft;
    g.tiles_y = (g.H + ft - 1) / ft;
    return EOD_OK;
}

// The kernel of a launch, chosen by vec, vecq, mixed and one.  A single vector goes to the one-vector kernels (psf_<name>_kernel,
// psf_<name>_mix_kernel), a pair to the general ones: DESIGN.md section 9.11 measured the two-vector bodies 3-6 % slower at equal taps, and
// a single body with a one-vector flag 1-6 % slower than the one-vector kernels, so the bodies are not merged.
#define PSF_GO(kernel, ...) hipLaunchKernelGGL((kernel), grid, block, 0, (hipStream_t)stream, g, __VA_ARGS__, items)
#define PSF_FORM(name, V, Q)                                                        \
    do {                                                                            \
        if (one && mixed) PSF_GO((name##_mix_kernel<V, Q>), tt.x, mx);              \
        else if (one) PSF_GO((name##_kernel<V, Q>), tt.x);                          \
        else if (mixed) PSF_GO((name##_xy_kernel<V, Q, true>), tt, mx);             \
        else PSF_GO((name##_xy_kernel<V, Q, false>), tt, mx);                       \
    } while (0)
#define PSF_LAUNCH(name, items_)                                                                                  \
    do {                                                                                                          \
        const long long items = (items_);                                                                         \
        const dim3 grid((int)(items < EOD_PSF_GRID_BLOCKS ? items : EOD_PSF_GRID_BLOCKS)), block(PSF_THREADS);    \
        if (vec && vecq) PSF_FORM(name, true, true);                                                              \
        else if (vec) PSF_FORM(name, true, false);                                                                \
        else if (vecq) PSF_FORM(name, false, true);                                                               \
        else PSF_FORM(name, false, false);                                                                        \
    } while (0)

// g.values == NULL: the operator alone
static int psf_residual_launch(const char* what, PsfArgs g, const PsfSource& src, void* stream) {
    PsfTapsXy tt;
    PsfMix mx;
    const bool mixed = src.M != nullptr, one = src.symmetric;
    const int rc = psf_common(what, g, tt, mx, src, g.K, g.C, PSF_MAXC, false);
    if (rc != EOD_OK) return rc;
    EOD_REQUIRE(!mixed || !g.values || g.mask_c1, "%s: with a matrix the mask is one plane for all bands (mask_c1 != 0)", what);
    const long long hw = (long long)g.H * g.W, chw = hw / (g.f * g.f);
    const long long np = (long long)g.B * g.C * hw, nq = (long long)g.B * g.K * chw;
    EOD_REQUIRE(!psf_overlap(g.out, nq, g.p, np), "%s: the output overlaps %s", what, g.values ? "p" : "x");
    if (g.values) {
        EOD_REQUIRE(g.lambda >= 0.0f && g.lambda <= 1.0f, "%s: the weight must lie in [0, 1], got %g", what, (double)g.lambda);
        EOD_REQUIRE(!psf_overlap(g.out, nq, g.values, (long long)(g.values_b1 ? 1 : g.B) * g.K * chw), "%s: q overlaps values", what);
        EOD_REQUIRE(!g.mask || !psf_overlap(g.out, nq, g.mask, (long long)(g.mask_b1 ? 1 : g.B) * (g.mask_c1 ? 1 : g.K) * chw), "%s: q overlaps mask", what);
    }
    const bool vec = g.W % 4 == 0 && eod_aligned16(g.p);
    const bool vecq = (g.W / g.f) % 4 == 0 && eod_aligned16(g.out) && (!g.values || eod_aligned16(g.values)) && (!g.mask || eod_aligned16(g.mask));
    PSF_LAUNCH(psf_residual, (long long)g.B * g.K * g.tiles_x * g.tiles_y);
    EOD_CHECK_LAUNCH(what);
    return EOD_OK;
}

static int psf_update_launch(const char* what, const float* p, const float* q, float step, const PsfSource& src, int f, int K, int B, int C, int H,
                             int W, float* out, void* stream) {
    EOD_REQUIRE(q, "%s: bad args", what);
    PsfArgs g = {p, nullptr, nullptr, q, out, 0.0f, step, 0, f, K, B, C, H, W, 0, 0, 0, 0, 0, 0, {0}, {0}};
    PsfTapsXy tt;
    PsfMix mx;
    const bool mixed = src.M != nullptr, one = src.symmetric;
    const int rc = psf_common(what, g, tt, mx, src, C, K, PSF_MAXK, true);
    if (rc != EOD_OK) return rc;
    EOD_REQUIRE(step - step == 0.0f && step > 0.0f, "%s: step must be finite and positive, got %g", what, (double)step);
    const long long hw = (long long)H * W, chw = hw / (f * f);
    const long long np = (long long)B * C * hw, nq = (long long)B * K * chw;
    EOD_REQUIRE(!psf_overlap(out, np, p, np), "%s: out overlaps p (a tile's halo is read after its neighbours have written)", what);
    EOD_REQUIRE(!psf_overlap(out, np, q, nq), "%s: out overlaps q", what);
    const bool vec = W % 4 == 0 && eod_aligned16(p) && eod_aligned16(out);
    const bool vecq = (W / f) % 4 == 0 && eod_aligned16(q);
    PSF_LAUNCH(psf_update, (long long)B * C * g.tiles_x * g.tiles_y);
    EOD_CHECK_LAUNCH(what);
    return EOD_OK;
}

// ------------------------------------------------------------------------------------------------ symmetric taps
extern "C" int eod_psf_residual(const float* p, const float* values, const float* mask, float lambda, const float* taps, int r, int f,
                                const int32_t* channels, int K, int B, int C, int H, int W, int values_b1, int mask_b1, int mask_c1, float* q,
                                void* stream) {
    EOD_REQUIRE(values, "psf_residual: bad args");
    PsfArgs g = {p, values, mask, nullptr, q, lambda, 0.0f, 0, f, K, B, C, H, W, values_b1, mask_b1, mask_c1, 0, 0, 0, {0}, {0}};
    return psf_residual_launch("psf_residual", g, psf_one_vector(taps, r, channels, nullptr), stream);
}

extern "C" int eod_psf_apply(const float* x, const float* taps, int r, int f, const int32_t* channels, int K, float* out, int B, int C, int H,
                             int W, void* stream) {
    PsfArgs g = {x, nullptr, nullptr, nullptr, out, 0.0f, 0.0f, 0, f, K, B, C, H, W, 0, 0, 0, 0, 0, 0, {0}, {0}};
    return psf_residual_launch("psf_apply", g, psf_one_vector(taps, r, channels, nullptr), stream);
}

extern "C" int eod_psf_update(const float* p, const float* q, float step, const float* taps, int r, int f, const int32_t* channels, int K,
                              int B, int C, int H, int W, float* out, void* stream) {
    return psf_update_launch("psf_update", p, q, step, psf_one_vector(taps, r, channels, nullptr), f, K, B, C, H, W, out, stream);
}

// ------------------------------------------------------------------------------------------------ through a band mix
extern "C" int eod_psf_residual_mix(const float* p, const float* values, const float* mask, float lambda, const float* taps, int r, int f,
                                    const float* R, int K, int B, int C, int H, int W, int values_b1, int mask_b1, float* q, void* stream) {
    EOD_REQUIRE(values, "psf_residual_mix: bad args");
    PsfArgs g = {p, values, mask, nullptr, q, lambda, 0.0f, 0, f, K, B, C, H, W, values_b1, mask_b1, 1, 0, 0, 0, {0}, {0}};
    return psf_residual_launch("psf_residual_mix", g, psf_one_vector(taps, r, nullptr, R), stream);
}

extern "C" int eod_psf_apply_mix(const float* x, const float* taps, int r, int f, const float* R, int K, float* out, int B, int C, int H, int W,
                                 void* stream) {
    PsfArgs g = {x, nullptr, nullptr, nullptr, out, 0.0f, 0.0f, 0, f, K, B, C, H, W, 0, 0, 1, 0, 0, 0, {0}, {0}};
    return psf_residual_launch("psf_apply_mix", g, psf_one_vector(taps, r, nullptr, R), stream);
}

extern "C" int eod_psf_update_mix(const float* p, const float* q, float step, const float* taps, int r, int f, const float* G, int K, int B,
                                  int C, int H, int W, float* out, void* stream) {
    return psf_update_launch("psf_update_mix", p, q, step, psf_one_vector(taps, r, nullptr, G), f, K, B, C, H, W, out, stream);
}

// ------------------------------------------------------------------------------------------------ one tap vector per axis
extern "C" int eod_psf_residual_xy(const float* p, const float* values, const float* mask, float lambda, const float* taps_y, int ry,
                                   const float* taps_x, int rx, int f, const int32_t* channels, const float* R, int K, int B, int C, int H, int W,
                                   int values_b1, int mask_b1, int mask_c1, float* q, void* stream) {
    EOD_REQUIRE(values, "psf_residual_xy: bad args");
    PsfArgs g = {p, values, mask, nullptr, q, lambda, 0.0f, 0, f, K, B, C, H, W, values_b1, mask_b1, mask_c1, 0, 0, 0, {0}, {0}};
    return psf_residual_launch("psf_residual_xy", g, psf_two_vectors(taps_y, ry, taps_x, rx, channels, R), stream);
}

extern "C" int eod_psf_apply_xy(const float* x, const float* taps_y, int ry, const float* taps_x, int rx, int f, const int32_t* channels,
                                const float* R, int K, float* out, int B, int C, int H, int W, void* stream) {
    PsfArgs g = {x, nullptr, nullptr, nullptr, out, 0.0f, 0.0f, 0, f, K, B, C, H, W, 0, 0, R ? 1 : 0, 0, 0, 0, {0}, {0}};
    return psf_residual_launch("psf_apply_xy", g, psf_two_vectors(taps_y, ry, taps_x, rx, channels, R), stream);
}

extern "C" int eod_psf_update_xy(const float* p, const float* q, float step, const float* taps_y, int ry, const float* taps_x, int rx, int f,
                                 const int32_t* channels, const float* G, int K, int B, int C, int H, int W, float* out, void* stream) {
    return psf_update_launch("psf_update_xy", p, q, step, psf_two_vectors(taps_y, ry, taps_x, rx, channels, G), f, K, B, C, H, W, out, stream);
}
