// Image-quality metrics: eod_band_stats, one pass over a prediction and a truth for the per-band sums and the
// spectral angle, and eod_ssim, the structural similarity map and its per-band sum.  include/eodiff.h states the operations.
//
// All arithmetic is float64 (the raw-moment variance E[x^2] - mu^2 cancels in fp32 on bright flat bands).  No floating-point atomics: every
// thread accumulates its own elements in ascending order, a workgroup adds its threads in a fixed order (met_reduce), the workgroup's
// partial goes to its own slot of the workspace, and the slots are added from left to right in groups of MET_FOLD, the group sums again,
// until one is left (met_fold_kernel: a plane of 2048^2 has thousands of slots, and one thread walking them all is a latency chain).  Which
// elements a thread and a workgroup own depends on the plane's shape alone, never on B or on the grid: a member of a stack has the bits of
// its single call.
#define SSIM_FN __device__ __forceinline__
#include "common.h"
#include "met_sum.h"
#include "ssim_body.h"

#include <math.h>

#define MET_MAXC SSIM_MAXC

struct BstArgs {
    const float* pred;
    const float* ref;
    const float* where;
    double* part;  // [B][chunks][C * BST_NB + BST_NS]
    long long HW, chunks;
    int B, C, ref_B, where_B;
    double a, b;
};

// grid (chunks of a sample, samples)
__global__ void __launch_bounds__(BST_THREADS) bst_kernel(BstArgs g) {
    __shared__ double red[2][BST_NB * BST_THREADS];  // two in turn: a band's sums are read while the next band's are written
    const int t = threadIdx.x;
    const int NV = g.C * BST_NB + BST_NS;
    for (long long chunk = blockIdx.x; chunk < g.chunks; chunk += gridDim.x) {
        for (int b = blockIdx.y; b < g.B; b += gridDim.y) {
            const long long base = chunk * BST_CHUNK + t;
            const long long wb = g.where_B == 1 ? 0 : (long long)b * g.HW;
            bool on[BST_PER];
            double pp[BST_PER], tt[BST_PER], dot[BST_PER];
#pragma unroll
            for (int j = 0; j < BST_PER; ++j) {
                const long long i = base + (long long)BST_THREADS * j;
                on[j] = i < g.HW && (!g.where || g.where[wb + i] != 0.0f);
                pp[j] = tt[j] = dot[j] = 0.0;
            }
            double* out = g.part + ((long long)b * g.chunks + chunk) * NV;
            for (int c = 0; c < g.C; ++c) {
                const float* ps = g.pred + ((long long)b * g.C + c) * g.HW;
                const float* ts = g.ref + ((long long)(g.ref_B == 1 ? 0 : b) * g.C + c) * g.HW;
                double s[BST_NB] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int j = 0; j < BST_PER; ++j) {
                    if (!on[j]) continue;
                    const long long i = base + (long long)BST_THREADS * j;
                    const double mp = g.a * (double)ps[i], mt = g.a * (double)ts[i];
                    const double p = mp + g.b, q = mt + g.b;
                    const double d = p - q;
                    const double p2 = p * p, q2 = q * q, pq = p * q, d2 = d * d;
                    s[0] = s[0] + 1.0;
                    s[1] = s[1] + p;
                    s[2] = s[2] + q;
                    s[3] = s[3] + p2;
                    s[4] = s[4] + q2;
                    s[5] = s[5] + pq;
                    s[6] = s[6] + d2;
                    s[7] = met_max(s[7], fabs(d));
                    pp[j] = pp[j] + p2;
                    tt[j] = tt[j] + q2;
                    dot[j] = dot[j] + pq;
                }
                const double x = met_reduce<BST_NB, 7>(red[c & 1], s, t);
                if ((t & 31) == 0) out[c * BST_NB + (t >> 5)] = x;
            }
            double a3[BST_NS] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int j = 0; j < BST_PER; ++j) {
                if (!on[j]) continue;
                if (pp[j] == 0.0 || tt[j] == 0.0) {
                    a3[2] = a3[2] + 1.0;
                } else {
                    const double x = pp[j] * tt[j], y = dot[j] * dot[j];
                    double w = x - y;
                    w = w > 0.0 ? w : 0.0;
                    a3[0] = a3[0] + atan2(sqrt(w), dot[j]);
                    a3[1] = a3[1] + 1.0;
                }
            }
            const double x = met_reduce<BST_NS, -1>(red[g.C & 1], a3, t);
            if ((t & 31) == 0 && (t >> 5) < BST_NS) out[g.C * BST_NB + (t >> 5)] = x;
            __syncthreads();  // (the next sample starts with red[0] again)
        }
    }
}

// grid (tiles of a plane, planes)
__global__ void __launch_bounds__(SSIM_THREADS) ssim_kernel(SsimArgs g, SsimTaps k) {
    extern __shared__ double ssim_lds[];  // P, T: E x E each; hb: E x SSIM_TILE (the launch sizes it)
    const int t = threadIdx.x, E = SSIM_TILE + 2 * g.r;
    double* P = ssim_lds;
    double* T = P + E * E;
    double* hb = T + E * E;
    const long long HW = (long long)g.H * g.W, planes = (long long)g.B * g.C, tiles = (long long)g.tiles_x * g.tiles_y;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int ty = (int)(tile / g.tiles_x), tx = (int)(tile - (long long)ty * g.tiles_x);
        const int y0 = ty * SSIM_TILE, x0 = tx * SSIM_TILE;
        for (long long bc = blockIdx.y; bc < planes; bc += gridDim.y) {
            const long long b = bc / g.C, c = bc - b * g.C;
            const long long plane_t = ((g.ref_B == 1 ? 0 : b) * g.C + c) * HW;
            const long long plane_w = g.where_B == 1 ? 0 : b * HW;
            ssim_load(g, t, bc * HW, plane_t, y0, x0, P, T);
            __syncthreads();
            double m[5 * SSIM_PER];
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                ssim_hpass(g, k, q, t, P, T, hb);
                __syncthreads();
                ssim_vpass(g, k, t, hb, m + q * SSIM_PER);
                __syncthreads();
            }
            double v[2];
            ssim_finish(g, t, bc * HW, plane_w, y0, x0, m, &v[0], &v[1]);
            const double x = met_reduce<2, -1>(hb, v, t);  // (hb: E x 32 >= 2 x 256 doubles)
            if ((t & 31) == 0 && (t >> 5) < 2) g.part[(bc * tiles + tile) * 2 + (t >> 5)] = x;
            __syncthreads();
        }
    }
}

static inline bool met_overlap(const void* a, long long na, const void* b, long long nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}
static inline bool met_aligned8(const void* p) { return ((uintptr_t)p & 7u) == 0; }
static inline bool met_finite(double v) { return v - v == 0.0; }

// the refusals both operators share; 0 when the arguments are good
static int met_common(const char* what, const float* pred, const float* ref, const float* where, int B, int ref_B, int where_B, int C, int H, int W,
                      double a, double b, const void* ws) {
    EOD_REQUIRE(pred && ref && ws, "%s: bad args (a null pointer)", what);
    EOD_REQUIRE(B > 0 && H > 0 && W > 0, "%s: B, H and W must be positive, got %d, %d, %d", what, B, H, W);
    EOD_REQUIRE(C >= 1 && C <= MET_MAXC, "%s: C must be in 1 .. %d, got %d", what, MET_MAXC, C);
    EOD_REQUIRE(ref_B == B || ref_B == 1, "%s: ref has %d members, pred has %d (ref_B is B or 1)", what, ref_B, B);
    EOD_REQUIRE(!where || where_B == B || where_B == 1, "%s: where has %d members, pred has %d (where_B is B or 1)", what, where_B, B);
    EOD_REQUIRE(met_finite(a) && met_finite(b), "%s: the affine (a, b) must be finite, got (%g, %g)", what, a, b);
    return EOD_OK;
}

extern "C" int64_t eod_band_stats_workspace_size(int B, int C, int H, int W) {
    if (B <= 0 || C < 1 || C > MET_MAXC || H <= 0 || W <= 0) return -1;
    const long long chunks = ((long long)H * W + BST_CHUNK - 1) / BST_CHUNK;
    const int NV = C * BST_NB + BST_NS;
    return ((int64_t)B * chunks * NV + met_fold_extra(B, chunks, NV)) * 8 + 16;  // (+ 16: the workspace may have any alignment)
}

extern "C" int eod_band_stats(const float* pred, const float* ref, const float* where, int B, int ref_B, int where_B, int C, int H, int W, double a,
                              double b, double* band, double* sample, void* ws, int64_t ws_bytes, void* stream) {
    const char* what = "band_stats";
    const int rc = met_common(what, pred, ref, where, B, ref_B, where_B, C, H, W, a, b, ws);
    if (rc != EOD_OK) return rc;
    EOD_REQUIRE(band && sample, "%s: bad args (a null output)", what);
    EOD_REQUIRE(met_aligned8(band) && met_aligned8(sample), "%s: the float64 outputs must be 8-byte aligned", what);
    const long long need = eod_band_stats_workspace_size(B, C, H, W);
    EOD_REQUIRE(ws_bytes >= need, "%s: the workspace has %lld bytes, eod_band_stats_workspace_size asks for %lld", what, (long long)ws_bytes, need);
    const long long nb = (long long)B * C * BST_NB * 8, ns = (long long)B * BST_NS * 8;
    EOD_REQUIRE(!met_overlap(band, nb, sample, ns) && !met_overlap(band, nb, ws, ws_bytes) && !met_overlap(sample, ns, ws, ws_bytes),
                "%s: band, sample and the workspace overlap each other", what);
    BstArgs g;
    g.pred = pred; g.ref = ref; g.where = where;
    g.part = reinterpret_cast<double*>(((uintptr_t)ws + 15u) & ~(uintptr_t)15u);
    g.HW = (long long)H * W;
    g.chunks = (g.HW + BST_CHUNK - 1) / BST_CHUNK;
    g.B = B; g.C = C; g.ref_B = ref_B; g.where_B = where ? where_B : 1;
    g.a = a; g.b = b;
    const dim3 grid((unsigned)(g.chunks < 2147483647LL ? g.chunks : 2147483647LL), (unsigned)(B < 65535 ? B : 65535));
    hipLaunchKernelGGL(bst_kernel, grid, dim3(BST_THREADS), 0, (hipStream_t)stream, g);
    EOD_CHECK_LAUNCH(what);
    return met_fold(what, g.part, B, g.chunks, C * BST_NB + BST_NS, C, nullptr, band, sample, (hipStream_t)stream);
}

extern "C" int64_t eod_ssim_workspace_size(int B, int C, int H, int W, int r) {
    if (B <= 0 || C < 1 || C > MET_MAXC || r < 0 || r > SSIM_MAXR || H < 2 * r + 1 || W < 2 * r + 1) return -1;
    const long long tx = (W - 2 * r + SSIM_TILE - 1) / SSIM_TILE, ty = (H - 2 * r + SSIM_TILE - 1) / SSIM_TILE;
    return ((int64_t)B * C * tx * ty * 2 + met_fold_extra((long long)B * C, tx * ty, 2)) * 8 + 16;
}

extern "C" int eod_ssim(const float* pred, const float* ref, const float* where, int B, int ref_B, int where_B, int C, int H, int W,
                        const double* taps, int r, double a, double b, double c1, double c2, float* map, double* sums, void* ws, int64_t ws_bytes,
                        void* stream) {
    const char* what = "ssim";
    const int rc = met_common(what, pred, ref, where, B, ref_B, where_B, C, H, W, a, b, ws);
    if (rc != EOD_OK) return rc;
    EOD_REQUIRE(sums && taps, "%s: bad args (a null pointer)", what);
    EOD_REQUIRE(met_aligned8(sums), "%s: the float64 output must be 8-byte aligned", what);
    EOD_REQUIRE(r >= 0 && r <= SSIM_MAXR, "%s: the window radius must be in 0 .. %d, got %d", what, SSIM_MAXR, r);
    EOD_REQUIRE(H >= 2 * r + 1 && W >= 2 * r + 1, "%s: a %d x %d image is smaller than the %d-tap window", what, H, W, 2 * r + 1);
    EOD_REQUIRE(met_finite(c1) && met_finite(c2), "%s: c1 and c2 must be finite, got (%g, %g)", what, c1, c2);
    SsimTaps k;
    for (int i = 0; i < 2 * SSIM_MAXR + 1; ++i) k.g[i] = 0.0;
    for (int i = 0; i < 2 * r + 1; ++i) {
        EOD_REQUIRE(met_finite(taps[i]), "%s: tap %d is not finite", what, i);
        k.g[i] = taps[i];
    }
    const long long need = eod_ssim_workspace_size(B, C, H, W, r);
    EOD_REQUIRE(ws_bytes >= need, "%s: the workspace has %lld bytes, eod_ssim_workspace_size asks for %lld", what, (long long)ws_bytes, need);
    const long long planes = (long long)B * C, nm = planes * H * W * 4, nsum = planes * 2 * 8;
    EOD_REQUIRE(!met_overlap(sums, nsum, ws, ws_bytes) && (!map || (!met_overlap(map, nm, ws, ws_bytes) && !met_overlap(map, nm, sums, nsum))),
                "%s: map, sums and the workspace overlap each other", what);
    EOD_REQUIRE(!map || (!met_overlap(map, nm, pred, nm) && !met_overlap(map, nm, ref, (long long)ref_B * C * H * W * 4)),
                "%s: map overlaps an input", what);
    SsimArgs g;
    g.pred = pred; g.ref = ref; g.where = where; g.map = map;
    g.part = reinterpret_cast<double*>(((uintptr_t)ws + 15u) & ~(uintptr_t)15u);
    g.B = B; g.C = C; g.H = H; g.W = W; g.r = r; g.ref_B = ref_B; g.where_B = where ? where_B : 1;
    g.tiles_x = (W - 2 * r + SSIM_TILE - 1) / SSIM_TILE;
    g.tiles_y = (H - 2 * r + SSIM_TILE - 1) / SSIM_TILE;
    g.a = a; g.b = b; g.c1 = c1; g.c2 = c2;
    const long long tiles = (long long)g.tiles_x * g.tiles_y;
    const dim3 grid((unsigned)(tiles < 2147483647LL ? tiles : 2147483647LL), (unsigned)(planes < 65535 ? planes : 65535));
    const int E = SSIM_TILE + 2 * r;
    const size_t lds = (size_t)(2 * E * E + E * SSIM_TILE) * sizeof(double);  // 64512 B at r = 12
    hipLaunchKernelGGL(ssim_kernel, grid, dim3(SSIM_THREADS), lds, (hipStream_t)stream, g, k);
    EOD_CHECK_LAUNCH(what);
    return met_fold(what, g.part, planes, tiles, 2, 0, sums, nullptr, nullptr, (hipStream_t)stream);
}
