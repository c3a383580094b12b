// Dynamic thresholding: per sample, the exact order statistics a_(k), a_(k+1) of |p| by radix selection over the
// 31 key bits, the scale s from them, and out = clamp(p, -s, s) / s.  include/eodiff.h states the operations.
//
// The key bits are cut into four fields, 8 + 8 + 8 + 7 from the top (the first field is the exponent).  Level L reads the sample once
// (thr_hist_kernel<L>): every key whose bits above the field equal the prefix a rank has been narrowed to is counted by its field, in
// 256 integer counters per rank in LDS and from there in the sample's counters in the workspace.  The next launch starts by finding the
// bin that holds each rank (thr_select: a scan over 256 counters, done by every workgroup for itself) and goes on with the longer
// prefix; the apply pass does the same for the last field and has both keys.  The two ranks k and k + 1 are followed side by side: as
// long as their prefixes agree they share one histogram, from the level where they part each has its own.  Every counter is an integer,
// so neither the order of the atomic adds nor the grid can change a result.  What one launch hands to the next (the counters, and the
// 4 words of state that workgroup 0 of a sample stores) crosses a kernel boundary; nothing is passed between workgroups of a launch.
//
// Hot bins (a constant or saturated tensor puts every key into one counter; real predictions fill a few dozen exponent bins): every
// wave has its own copy of the LDS counters, and before a wave adds, the lanes that hold the same counter as the first pending lane are
// added as one number, twice; what is left goes lane by lane.
#include "common.h"

#define THR_LEVELS 4
#define THR_BINS 256
#define THR_WAVES 4
#define THR_CNT_BYTES ((long long)THR_LEVELS * 2 * THR_BINS * 4)  // per sample: [level][rank][bin] uint32
#define THR_ST_BYTES ((long long)THR_LEVELS * 4 * 4)               // per sample: [level]{prefix, rank} x 2 uint32

struct ThrArgs {
    const float* p;
    float* out;
    float* s_out;
    unsigned* cnt;  // [B][THR_LEVELS][2][THR_BINS]
    unsigned* st;   // [B][THR_LEVELS][4]
    long long n;
    unsigned k0, k1;  // the two ranks
    float frac, cap;
    int B;
};

struct ThrRanks {
    unsigned p0, r0, p1, r1;  // per rank: the key bits above the current field, and the rank among the keys that share them
};

__host__ __device__ constexpr int thr_shift(int L) { return L == 0 ? 23 : L == 1 ? 15 : L == 2 ? 7 : 0; }
__host__ __device__ constexpr int thr_width(int L) { return L == 3 ? 7 : 8; }

// The bin of level L's counters that holds each rank, and the ranks inside it.  Called by all 256 threads; sh: 12 words of LDS.
template <int L>
__device__ __forceinline__ ThrRanks thr_select(const ThrArgs& g, int b, const ThrRanks in, unsigned* sh) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const unsigned* H = g.cnt + ((long long)b * THR_LEVELS + L) * 2 * THR_BINS;
    const bool split = in.p1 != in.p0;
    const unsigned ca = H[t], cb = split ? H[THR_BINS + t] : 0u;
    unsigned ia = ca, ib = cb;  // inclusive sums
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned ua = __shfl_up(ia, o), ub = __shfl_up(ib, o);
        if (lane >= o) { ia += ua; ib += ub; }
    }
    if (lane == 63) { sh[w] = ia; sh[THR_WAVES + w] = ib; }
    if (t < 4) sh[2 * THR_WAVES + t] = 0u;
    __syncthreads();
    for (int j = 0; j < w; ++j) { ia += sh[j]; ib += sh[THR_WAVES + j]; }
    const unsigned ea = ia - ca, eb = ib - cb;
    if (in.r0 >= ea && in.r0 < ia) { sh[8] = (unsigned)t; sh[9] = in.r0 - ea; }
    const unsigned i1 = split ? ib : ia, e1 = split ? eb : ea;
    if (in.r1 >= e1 && in.r1 < i1) { sh[10] = (unsigned)t; sh[11] = in.r1 - e1; }
    __syncthreads();
    const ThrRanks out = {(in.p0 << thr_width(L)) | sh[8], sh[9], (in.p1 << thr_width(L)) | sh[10], sh[11]};
    __syncthreads();  // (sh is written again by the next caller)
    return out;
}

// The ranks as level L meets them (L = THR_LEVELS: the two keys themselves).  Level L - 1's selection is made here, from the state that the
// launch before this one stored; workgroup 0 of the sample stores the result for the launch after this one.
template <int L>
__device__ __forceinline__ ThrRanks thr_ranks(const ThrArgs& g, int b, unsigned* sh) {
    ThrRanks in = {0u, g.k0, 0u, g.k1};
    if constexpr (L == 0) {
        return in;
    } else {
        if constexpr (L >= 2) {
            const unsigned* s = g.st + ((long long)b * THR_LEVELS + (L - 2)) * 4;
            in.p0 = s[0]; in.r0 = s[1]; in.p1 = s[2]; in.r1 = s[3];
        }
        const ThrRanks out = thr_select<L - 1>(g, b, in, sh);
        if (L < THR_LEVELS && blockIdx.x == 0 && threadIdx.x == 0) {
            unsigned* s = g.st + ((long long)b * THR_LEVELS + (L - 1)) * 4;
            s[0] = out.p0; s[1] = out.r0; s[2] = out.p1; s[3] = out.r1;
        }
        return out;
    }
}

// one count into the wave's counters h; slot < 0: nothing to count.  Every lane of the wave calls.
__device__ __forceinline__ void thr_count(unsigned* h, int slot, int lane) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const unsigned long long pending = __ballot(slot >= 0);
        if (pending == 0ull) return;
        const int leader = __ffsll((long long)pending) - 1;
        const int ls = __shfl(slot, leader);
        const unsigned long long same = __ballot(slot == ls);
        if (lane == leader) atomicAdd(&h[ls], (unsigned)__popcll(same));
        if (slot == ls) slot = -1;
    }
    if (slot >= 0) atomicAdd(&h[slot], 1u);
}

template <bool VEC>
__device__ __forceinline__ int thr_load(const float* src, long long n, long long qd, long long quads, float* v) {
    v[0] = v[1] = v[2] = v[3] = 0.0f;
    if (qd >= quads) return 0;
    const long long i0 = qd * 4;
    if (VEC) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(src + i0);
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
        return 4;
    }
    const int nv = n - i0 >= 4 ? 4 : (int)(n - i0);
    for (int j = 0; j < nv; ++j) v[j] = src[i0 + j];
    return nv;
}

// grid (workgroups per sample, samples); the workgroups of a sample stride over its quads, two quads per thread in flight
template <int L, bool VEC>
__global__ void __launch_bounds__(256) thr_hist_kernel(ThrArgs g) {
    __shared__ unsigned hist[THR_WAVES * 2 * THR_BINS];
    __shared__ unsigned sh[12];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    constexpr int SH = thr_shift(L), UP = thr_shift(L) + thr_width(L);
    constexpr unsigned FIELD = (1u << thr_width(L)) - 1u;
    const long long quads = (g.n + 3) / 4, stride = (long long)gridDim.x * 256;
    for (int b = blockIdx.y; b < g.B; b += gridDim.y) {
        const ThrRanks rk = thr_ranks<L>(g, b, sh);
        for (int i = t; i < THR_WAVES * 2 * THR_BINS; i += 256) hist[i] = 0u;
        __syncthreads();
        unsigned* hw = hist + w * 2 * THR_BINS;
        const float* ps = g.p + (long long)b * g.n;
        for (long long q0 = (long long)blockIdx.x * 256; q0 < quads; q0 += 2 * stride) {  // (q0 is the same for the whole workgroup)
            float v[2][4];
            int nv[2];
            nv[0] = thr_load<VEC>(ps, g.n, q0 + t, quads, v[0]);
            nv[1] = thr_load<VEC>(ps, g.n, q0 + stride + t, quads, v[1]);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const unsigned key = __float_as_uint(v[u][j]) & 0x7fffffffu;
                    const unsigned up = key >> UP;
                    int slot = j >= nv[u] ? -1 : (up == rk.p0 ? 0 : (up == rk.p1 ? THR_BINS : -1));
                    if (slot >= 0) slot += (int)((key >> SH) & FIELD);
                    thr_count(hw, slot, lane);
                }
            }
        }
        __syncthreads();
        unsigned* H = g.cnt + ((long long)b * THR_LEVELS + L) * 2 * THR_BINS;
        for (int i = t; i < 2 * THR_BINS; i += 256) {
            unsigned c = 0u;
#pragma unroll
            for (int ww = 0; ww < THR_WAVES; ++ww) c += hist[ww * 2 * THR_BINS + i];
            if (c != 0u) atomicAdd(&H[i], c);
        }
        __syncthreads();
    }
}

template <bool VEC>
__global__ void __launch_bounds__(256) thr_apply_kernel(ThrArgs g) {
    __shared__ unsigned sh[12];
    const int t = threadIdx.x;
    const long long quads = (g.n + 3) / 4, stride = (long long)gridDim.x * 256;
    for (int b = blockIdx.y; b < g.B; b += gridDim.y) {
        const ThrRanks rk = thr_ranks<THR_LEVELS>(g, b, sh);
        const float lo = __uint_as_float(rk.p0), hi = __uint_as_float(rk.p1);
        float v = lo;
        if (g.frac != 0.0f) {
            const float d = hi - lo;
            const float m = g.frac * d;
            v = lo + m;
        }
        const float s = fminf(fmaxf(v, 1.0f), g.cap);
        if (blockIdx.x == 0 && t == 0) g.s_out[b] = s;
        const float* ps = g.p + (long long)b * g.n;
        float* po = g.out + (long long)b * g.n;
        for (long long qd = (long long)blockIdx.x * 256 + t; qd < quads; qd += stride) {
            float x[4], o[4];
            const int nv = thr_load<VEC>(ps, g.n, qd, quads, x);
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = fminf(fmaxf(x[j], -s), s) / s;
            if (VEC) {
                const f32x4 q = {o[0], o[1], o[2], o[3]};
                *reinterpret_cast<f32x4*>(po + qd * 4) = q;
            } else {
                for (int j = 0; j < nv; ++j) po[qd * 4 + j] = o[j];
            }
        }
    }
}

static inline bool thr_overlap(const void* a, long long na, const void* b, long long nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}

extern "C" int64_t eod_dyn_threshold_workspace_size(int B, int64_t n) {
    if (B <= 0 || n <= 0 || n > 2147483647LL) return -1;
    return (int64_t)B * (THR_CNT_BYTES + THR_ST_BYTES) + 16;  // (+ 16: the workspace may have any alignment)
}

extern "C" int eod_dyn_threshold(const float* p, int64_t k, float frac, float cap, float* out, float* s_out, int B, int64_t n, void* ws,
                                 int64_t ws_bytes, void* stream) {
    const char* what = "dyn_threshold";
    EOD_REQUIRE(p && out && s_out && ws, "%s: bad args (a null pointer)", what);
    EOD_REQUIRE(B > 0, "%s: B must be positive, got %d", what, B);
    EOD_REQUIRE(n > 0 && n <= 2147483647LL, "%s: n must be in 1 .. 2^31 - 1, got %lld", what, (long long)n);
    EOD_REQUIRE(k >= 0 && k <= n - 1, "%s: k must be in 0 .. n - 1 = %lld, got %lld", what, (long long)(n - 1), (long long)k);
    EOD_REQUIRE(frac >= 0.0f && frac < 1.0f, "%s: frac must be in [0, 1), got %g", what, (double)frac);
    EOD_REQUIRE(cap >= 1.0f, "%s: cap must be >= 1 (+inf allowed), got %g", what, (double)cap);
    const long long need = eod_dyn_threshold_workspace_size(B, n);
    EOD_REQUIRE(ws_bytes >= need, "%s: the workspace has %lld bytes, eod_dyn_threshold_workspace_size asks for %lld", what,
                (long long)ws_bytes, need);
    const long long np = (long long)B * n * 4, ns = (long long)B * 4;
    EOD_REQUIRE(!thr_overlap(out, np, p, np) && !thr_overlap(s_out, ns, p, np) && !thr_overlap(ws, ws_bytes, p, np),
                "%s: out, s_out or the workspace overlaps p", what);
    EOD_REQUIRE(!thr_overlap(out, np, s_out, ns) && !thr_overlap(out, np, ws, ws_bytes) && !thr_overlap(s_out, ns, ws, ws_bytes),
                "%s: out, s_out and the workspace overlap each other", what);
    unsigned char* base = reinterpret_cast<unsigned char*>(((uintptr_t)ws + 15u) & ~(uintptr_t)15u);
    ThrArgs g;
    g.p = p; g.out = out; g.s_out = s_out;
    g.cnt = reinterpret_cast<unsigned*>(base);
    g.st = reinterpret_cast<unsigned*>(base + (long long)B * THR_CNT_BYTES);
    g.n = n;
    g.k0 = (unsigned)k;
    g.k1 = (unsigned)(k + 1 < n ? k + 1 : n - 1);
    g.frac = frac; g.cap = cap; g.B = B;
    // the counters are cleared here, on the stream, whatever an earlier call or the caller left in them; the state words are written
    // before they are read
    if (hipMemsetAsync(g.cnt, 0, (size_t)((long long)B * THR_CNT_BYTES), (hipStream_t)stream) != hipSuccess) {
        (void)hipGetLastError();
        eod_set_error("%s: clearing the counters failed", what);
        return EOD_ELAUNCH;
    }
    // workgroups per sample: about 1024 in all (4 per CU), never more than the sample has quads for
    const long long quads = (n + 3) / 4;
    long long per = (1024 + B - 1) / B, most = (quads + 255) / 256;
    if (per > most) per = most;
    if (per < 1) per = 1;
    const dim3 grid((unsigned)per, (unsigned)(B < 65535 ? B : 65535)), block(256);
    const bool vec = n % 4 == 0 && eod_aligned16(p) && eod_aligned16(out);
#define THR_HIST(L)                                                                                        \
    do {                                                                                                   \
        if (vec) hipLaunchKernelGGL((thr_hist_kernel<L, true>), grid, block, 0, (hipStream_t)stream, g);   \
        else hipLaunchKernelGGL((thr_hist_kernel<L, false>), grid, block, 0, (hipStream_t)stream, g);      \
        EOD_CHECK_LAUNCH(what);                                                                            \
    } while (0)
    THR_HIST(0);
    THR_HIST(1);
    THR_HIST(2);
    THR_HIST(3);
#undef THR_HIST
    if (vec) hipLaunchKernelGGL((thr_apply_kernel<true>), grid, block, 0, (hipStream_t)stream, g);
    else hipLaunchKernelGGL((thr_apply_kernel<false>), grid, block, 0, (hipStream_t)stream, g);
    EOD_CHECK_LAUNCH(what);
    return EOD_OK;
}
