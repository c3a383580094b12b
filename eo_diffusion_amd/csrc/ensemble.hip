// Ensemble statistics: eod_scene_quantiles, per-pixel order statistics over the B <= 64 members of a stack, and
// eod_ensemble_stats, the verification of the stack against one truth (CRPS, rank histogram, coverage, spread and skill).  include/eodiff.h
// states the operations.
//
// One lane owns one pixel at a time: it loads the pixel's B members (member b of pixel i is x[b * n + i], so a wave's loads are contiguous
// per member), turns them into order-preserving integer keys, and sorts the keys in registers with a fixed network (ensemble_body.h),
// instantiated for the padded sizes P = 1, 2, 4 .. 64; the stack streams through once.  The float64 sums of the verification follow the
// discipline of eod_band_stats (met_sum.h): per-thread ascending order, a fixed order inside a workgroup, one slot per workgroup, the slots
// folded left to right; which pixels a thread and a workgroup own depends on H * W alone.  The integer counts go through integer atomics
// (a workgroup's histogram in LDS first): their result does not depend on the order.
#define ENS_FN __device__ __forceinline__
#include "common.h"
#include "ensemble_body.h"
#include "met_sum.h"

#include <math.h>

#define ENS_MAXC 32
#define ENS_THREADS BST_THREADS                 // 256 (met_reduce is written for it)
#define ENS_VEC 4                               // pixels per lane and trip of the vector form of the quantile kernel (P <= ENS_VEC_MAXP)
#define ENS_VEC_MAXP 16                         // the widest network whose four pixels' keys fit the register budget (4 x 16 keys)
#define ENS_PER 2                               // pixels per thread of the verification: t + ENS_THREADS * j (small: a pixel is ~1000 instructions,
                                                // and a 256 x 256 band should still be more workgroups than the device has units)
#define ENS_CHUNK (ENS_THREADS * ENS_PER)       // 512 pixels: one workgroup's share of a band (tests/test_gpu_ensemble.py: ENS_CHUNK)
#define ENS_GRID 4096                           // workgroups of one eod_ensemble_stats launch, about (16 per compute unit)
#define ENS_NV 5                                // float64 sums per band
#define ENS_NCOUNT (2 + ENS_MAXB + 1 + ENS_MAXL)

struct EnsQuant {
    int k[ENS_MAXQ];
    float frac[ENS_MAXQ];
    int Q;
};

// B as a scalar register the compiler knows nothing about: the P conditions `b < B` of an unrolled member loop are then evaluated where they
// are used, one scalar compare each, instead of being hoisted out of the pixel loop into P register pairs (more than a wave has)
__device__ __forceinline__ int ens_opaque(int B) {
    asm volatile("" : "+s"(B));
    return B;
}
// (and the member stride: the P offsets b * stride likewise)
__device__ __forceinline__ long long ens_opaque(long long stride) {
    asm volatile("" : "+s"(stride));
    return stride;
}

// grid-stride over the n / V items; V = 4: 16-byte loads and stores
template <int P, int V>
__global__ void __launch_bounds__(ENS_THREADS) ens_quant_kernel(const float* __restrict__ x, float* __restrict__ out, int B, long long n, EnsQuant q) {
    typedef float vec __attribute__((ext_vector_type(V)));
    const long long items = n / V;
    for (long long j = (long long)blockIdx.x * ENS_THREADS + threadIdx.x; j < items; j += (long long)gridDim.x * ENS_THREADS) {
        const vec* px = reinterpret_cast<const vec*>(x) + j;
        const int Bs = ens_opaque(B);
        const long long stride = ens_opaque(items);
        uint32_t key[V][P];
#pragma unroll
        for (int b = 0; b < P; ++b) {
            if (b < Bs) {
                const vec v = px[b * stride];
#pragma unroll
                for (int e = 0; e < V; ++e) key[e][b] = ens_key(v[e]);
            } else {
#pragma unroll
                for (int e = 0; e < V; ++e) key[e][b] = ENS_TOP;
            }
        }
#pragma unroll
        for (int e = 0; e < V; ++e) ens_sort<P>(key[e]);
#pragma unroll
        for (int jq = 0; jq < ENS_MAXQ; ++jq) {
            if (jq < q.Q) {
                const int at = ens_opaque(q.k[jq]);  // (the conditions of ens_pick's levels, too)
                vec o;
#pragma unroll
                for (int e = 0; e < V; ++e) o[e] = ens_quantile<P>(key[e], at, q.frac[jq]);
                reinterpret_cast<vec*>(out)[(long long)jq * items + j] = o;
            }
        }
    }
}

struct EnsStats {
    const float* x;      // [B][C][HW]
    const float* y;      // [C][HW]
    const float* where;  // [HW] or null
    double* part;        // [C][chunks][ENS_NV]
    unsigned long long* counts;  // [C][2 + B + 1 + L], cleared by the call
    float* map;          // [C][HW] or null
    long long HW, chunks;
    int B, C, L;
    int k_lo[ENS_MAXL], k_hi[ENS_MAXL];
    float f_lo[ENS_MAXL], f_hi[ENS_MAXL];
};

// grid (workgroups of a band: each walks the chunks blockIdx.x, blockIdx.x + gridDim.x, .., bands)
template <int P>
__global__ void __launch_bounds__(ENS_THREADS) ens_stats_kernel(EnsStats g) {
    __shared__ double red[ENS_NV * ENS_THREADS];
    __shared__ unsigned hist[ENS_NCOUNT];
    const int t = threadIdx.x, B = g.B;
    const int nc = 2 + B + 1 + g.L;
    const double dB = (double)B, dBB = dB * dB, dB1 = (double)(B - 1);
    for (int c = blockIdx.y; c < g.C; c += gridDim.y) {
        // the counts of every chunk this workgroup walks meet in LDS and go to the band's counters once, at the end: one integer atomic per
        // bin and workgroup (per chunk, the thousands of workgroups of a 2048 x 2048 band would queue on the same few addresses)
        if (t < nc) hist[t] = 0u;
        __syncthreads();
        const float* xs = g.x + (long long)c * g.HW;
        const float* ys = g.y + (long long)c * g.HW;
        unsigned cnt = 0u, ties = 0u, cov[ENS_MAXL] = {0u, 0u, 0u, 0u};  // this thread's counts; the ranks go to the histogram one by one
        for (long long chunk = blockIdx.x; chunk < g.chunks; chunk += gridDim.x) {
            double s[ENS_NV] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
            for (int j = 0; j < ENS_PER; ++j) {
                const long long i = chunk * ENS_CHUNK + t + (long long)ENS_THREADS * j;
                if (i >= g.HW) break;
                if (g.where && !(g.where[i] != 0.0f)) {
                    if (g.map) g.map[(long long)c * g.HW + i] = __uint_as_float(0x7fc00000u);
                    continue;
                }
                const int Bs = ens_opaque(B);
                const long long stride = ens_opaque(g.C * g.HW);
                uint32_t key[P];
#pragma unroll
                for (int b = 0; b < P; ++b) key[b] = b < Bs ? ens_key(xs[b * stride + i]) : ENS_TOP;
                ens_sort<P>(key);
                const float y = ys[i];
                const uint32_t yk = ens_key(y);
                const double yd = (double)y;
                double a = 0.0, gs = 0.0, sum = 0.0;
                int rank = 0;
                bool tie = false;
                const int Bt = ens_opaque(B);  // (a value of its own per loop: shared conditions would live across the sort)
#pragma unroll
                for (int b = 0; b < P; ++b) {
                    if (b < Bt) {
                        const double xd = (double)ens_unkey(key[b]);
                        const double ad = fabs(xd - yd);
                        const double gx = (double)(2 * b - Bt + 1) * xd;
                        a = a + ad;
                        gs = gs + gx;
                        sum = sum + xd;
                        rank += key[b] < yk ? 1 : 0;
                        tie = tie || key[b] == yk;
                    }
                }
                const double m = sum / dB;
                double ss = 0.0;
                const int Bu = ens_opaque(B);
#pragma unroll
                for (int b = 0; b < P; ++b) {
                    if (b < Bu) {
                        asm volatile("" : "+v"(key[b]));  // (decode the key again: 64 doubles kept from the first pass are 128 registers)
                        const double d = (double)ens_unkey(key[b]) - m;
                        const double dd = d * d;
                        ss = ss + dd;
                    }
                }
                const double s2 = B > 1 ? ss / dB1 : 0.0;
                const double t1 = a / dB, t2 = gs / dBB;
                const double e = m - yd;
                const double ee = e * e;
                s[0] = s[0] + t1;
                s[1] = s[1] + t2;
                s[2] = s[2] + ee;
                s[3] = s[3] + s2;
                s[4] = s[4] + e;
                if (g.map) g.map[(long long)c * g.HW + i] = (float)(t1 - t2);
                cnt += 1u;
                ties += tie ? 1u : 0u;
                atomicAdd(&hist[2 + rank], 1u);
#pragma unroll
                for (int l = 0; l < ENS_MAXL; ++l) {
                    if (l < g.L) {
                        const float qlo = ens_quantile<P>(key, ens_opaque(g.k_lo[l]), g.f_lo[l]);
                        const float qhi = ens_quantile<P>(key, ens_opaque(g.k_hi[l]), g.f_hi[l]);
                        cov[l] += (qlo <= y && y <= qhi) ? 1u : 0u;
                    }
                }
            }
            const double v = met_reduce<ENS_NV, -1>(red, s, t);
            if ((t & 31) == 0 && (t >> 5) < ENS_NV) g.part[((long long)c * g.chunks + chunk) * ENS_NV + (t >> 5)] = v;
            __syncthreads();  // (red is written again by the next chunk)
        }
        if (cnt) atomicAdd(&hist[0], cnt);
        if (ties) atomicAdd(&hist[1], ties);
#pragma unroll
        for (int l = 0; l < ENS_MAXL; ++l)
            if (cov[l]) atomicAdd(&hist[2 + B + 1 + l], cov[l]);
        __syncthreads();
        if (t < nc && hist[t] != 0u) atomicAdd(&g.counts[(long long)c * nc + t], (unsigned long long)hist[t]);
        __syncthreads();
    }
}

static inline bool ens_overlap(const void* a, long long na, const void* b, long long nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}
static inline bool ens_aligned8(const void* p) { return ((uintptr_t)p & 7u) == 0; }
static inline int ens_padded(int B) {
    int P = 1;
    while (P < B) P <<= 1;
    return P;
}
// (k, frac) names x_(k), or a point between x_(k) and x_(k + 1)
static inline bool ens_rank_ok(int k, float frac, int B) { return k >= 0 && k < B && frac >= 0.0f && frac < 1.0f && (frac == 0.0f || k + 1 < B); }

template <int V>
static void ens_quant_launch(int P, dim3 grid, hipStream_t stream, const float* x, float* out, int B, long long n, const EnsQuant& q) {
    switch (P) {
#define ENS_CASE(PP) case PP: hipLaunchKernelGGL((ens_quant_kernel<PP, V>), grid, dim3(ENS_THREADS), 0, stream, x, out, B, n, q); break
        ENS_CASE(1); ENS_CASE(2); ENS_CASE(4); ENS_CASE(8); ENS_CASE(16);
        default: break;
#undef ENS_CASE
    }
}

extern "C" int eod_scene_quantiles(const float* x, float* out, int B, int64_t n, const int32_t* k, const float* frac, int Q, void* stream) {
    const char* what = "scene_quantiles";
    EOD_REQUIRE(x && out && k && frac, "%s: bad args (a null pointer)", what);
    EOD_REQUIRE(B >= 1 && B <= ENS_MAXB, "%s: B must be in 1 .. %d, got %d", what, ENS_MAXB, B);
    EOD_REQUIRE(n > 0, "%s: n must be positive, got %lld", what, (long long)n);
    EOD_REQUIRE(Q >= 1 && Q <= ENS_MAXQ, "%s: Q must be in 1 .. %d, got %d", what, ENS_MAXQ, Q);
    EnsQuant q;
    q.Q = Q;
    for (int j = 0; j < ENS_MAXQ; ++j) {
        q.k[j] = 0;
        q.frac[j] = 0.0f;
    }
    for (int j = 0; j < Q; ++j) {
        EOD_REQUIRE(ens_rank_ok(k[j], frac[j], B), "%s: quantile %d: 0 <= k < B, 0 <= frac < 1 and k + 1 < B where frac > 0, got (%d, %g) at B = %d", what, j,
                    k[j], (double)frac[j], B);
        q.k[j] = k[j];
        q.frac[j] = frac[j];
    }
    EOD_REQUIRE(!ens_overlap(out, (long long)Q * n * 4, x, (long long)B * n * 4), "%s: out overlaps x", what);
    const int P = ens_padded(B);
    const bool v4 = P <= ENS_VEC_MAXP && (n % ENS_VEC == 0) && eod_aligned16(x) && eod_aligned16(out);
    const long long items = v4 ? n / ENS_VEC : n, blocks = (items + ENS_THREADS - 1) / ENS_THREADS;
    const dim3 grid((unsigned)(blocks < 16384 ? blocks : 16384));
    if (v4) {
        ens_quant_launch<ENS_VEC>(P, grid, (hipStream_t)stream, x, out, B, (long long)n, q);
    } else if (P == 32) {
        hipLaunchKernelGGL((ens_quant_kernel<32, 1>), grid, dim3(ENS_THREADS), 0, (hipStream_t)stream, x, out, B, (long long)n, q);
    } else if (P == 64) {
        hipLaunchKernelGGL((ens_quant_kernel<64, 1>), grid, dim3(ENS_THREADS), 0, (hipStream_t)stream, x, out, B, (long long)n, q);
    } else {
        ens_quant_launch<1>(P, grid, (hipStream_t)stream, x, out, B, (long long)n, q);
    }
    EOD_CHECK_LAUNCH(what);
    return EOD_OK;
}

extern "C" int64_t eod_ensemble_stats_workspace_size(int B, int C, int H, int W) {
    if (B < 1 || B > ENS_MAXB || C < 1 || C > ENS_MAXC || H <= 0 || W <= 0) return -1;
    const long long chunks = ((long long)H * W + ENS_CHUNK - 1) / ENS_CHUNK;
    return ((int64_t)C * chunks * ENS_NV + met_fold_extra(C, chunks, ENS_NV)) * 8 + 16;  // (+ 16: the workspace may have any alignment)
}

extern "C" int eod_ensemble_stats(const float* x, const float* truth, const float* where, int B, int C, int H, int W, const int32_t* level_k,
                                  const float* level_frac, int L, double* sums, int64_t* counts, float* crps_map, void* ws, int64_t ws_bytes,
                                  void* stream) {
    const char* what = "ensemble_stats";
    EOD_REQUIRE(x && truth && sums && counts && ws, "%s: bad args (a null pointer)", what);
    EOD_REQUIRE(B >= 1 && B <= ENS_MAXB, "%s: B must be in 1 .. %d, got %d", what, ENS_MAXB, B);
    EOD_REQUIRE(C >= 1 && C <= ENS_MAXC, "%s: C must be in 1 .. %d, got %d", what, ENS_MAXC, C);
    EOD_REQUIRE(H > 0 && W > 0, "%s: H and W must be positive, got %d, %d", what, H, W);
    EOD_REQUIRE(L >= 0 && L <= ENS_MAXL, "%s: L must be in 0 .. %d, got %d", what, ENS_MAXL, L);
    EOD_REQUIRE(L == 0 || (level_k && level_frac), "%s: bad args (a null level table)", what);
    EnsStats g;
    for (int l = 0; l < ENS_MAXL; ++l) {
        g.k_lo[l] = g.k_hi[l] = 0;
        g.f_lo[l] = g.f_hi[l] = 0.0f;
    }
    for (int l = 0; l < L; ++l) {
        EOD_REQUIRE(ens_rank_ok(level_k[2 * l], level_frac[2 * l], B) && ens_rank_ok(level_k[2 * l + 1], level_frac[2 * l + 1], B),
                    "%s: level %d: 0 <= k < B, 0 <= frac < 1 and k + 1 < B where frac > 0, got (%d, %g) and (%d, %g) at B = %d", what, l, level_k[2 * l],
                    (double)level_frac[2 * l], level_k[2 * l + 1], (double)level_frac[2 * l + 1], B);
        g.k_lo[l] = level_k[2 * l];
        g.k_hi[l] = level_k[2 * l + 1];
        g.f_lo[l] = level_frac[2 * l];
        g.f_hi[l] = level_frac[2 * l + 1];
    }
    EOD_REQUIRE(ens_aligned8(sums) && ens_aligned8(counts), "%s: sums and counts must be 8-byte aligned", what);
    const long long need = eod_ensemble_stats_workspace_size(B, C, H, W);
    EOD_REQUIRE(ws_bytes >= need, "%s: the workspace has %lld bytes, eod_ensemble_stats_workspace_size asks for %lld", what, (long long)ws_bytes, need);
    const long long HW = (long long)H * W, nc = 2 + B + 1 + L;
    const long long nsum = (long long)C * ENS_NV * 8, ncnt = (long long)C * nc * 8, nmap = (long long)C * HW * 4, nx = (long long)B * C * HW * 4;
    EOD_REQUIRE(!ens_overlap(sums, nsum, counts, ncnt) && !ens_overlap(sums, nsum, ws, ws_bytes) && !ens_overlap(counts, ncnt, ws, ws_bytes),
                "%s: sums, counts and the workspace overlap each other", what);
    EOD_REQUIRE(!crps_map || (!ens_overlap(crps_map, nmap, sums, nsum) && !ens_overlap(crps_map, nmap, counts, ncnt) && !ens_overlap(crps_map, nmap, ws, ws_bytes)),
                "%s: crps_map overlaps sums, counts or the workspace", what);
    EOD_REQUIRE(!crps_map || (!ens_overlap(crps_map, nmap, x, nx) && !ens_overlap(crps_map, nmap, truth, nmap) && (!where || !ens_overlap(crps_map, nmap, where, HW * 4))),
                "%s: crps_map overlaps an input", what);
    g.x = x; g.y = truth; g.where = where; g.map = crps_map;
    g.part = reinterpret_cast<double*>(((uintptr_t)ws + 15u) & ~(uintptr_t)15u);
    g.counts = reinterpret_cast<unsigned long long*>(counts);
    g.HW = HW;
    g.chunks = (HW + ENS_CHUNK - 1) / ENS_CHUNK;
    g.B = B; g.C = C; g.L = L;
    if (hipMemsetAsync(counts, 0, (size_t)ncnt, (hipStream_t)stream) != hipSuccess) {
        (void)hipGetLastError();
        eod_set_error("%s: clearing the counts failed", what);
        return EOD_ELAUNCH;
    }
    const long long per_band = (ENS_GRID + C - 1) / C;  // (the grid only decides who computes a chunk's slot, never its value)
    const dim3 grid((unsigned)(g.chunks < per_band ? g.chunks : per_band), (unsigned)C);
    switch (ens_padded(B)) {
#define ENS_CASE(PP) case PP: hipLaunchKernelGGL((ens_stats_kernel<PP>), grid, dim3(ENS_THREADS), 0, (hipStream_t)stream, g); break
        ENS_CASE(1); ENS_CASE(2); ENS_CASE(4); ENS_CASE(8); ENS_CASE(16); ENS_CASE(32); ENS_CASE(64);
        default: break;
#undef ENS_CASE
    }
    EOD_CHECK_LAUNCH(what);
    return met_fold(what, g.part, C, g.chunks, ENS_NV, 0, sums, nullptr, nullptr, (hipStream_t)stream);
}
