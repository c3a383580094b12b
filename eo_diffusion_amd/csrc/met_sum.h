// The float64 summation discipline of the metrics (DESIGN.md sections 9.13 and 9.14), shared by metrics.hip and ensemble.hip: no floating-point
// atomics; every thread accumulates its own elements in ascending order, a workgroup of BST_THREADS adds its threads in a fixed order
// (met_reduce), the workgroup's partial goes to its own slot of the workspace, and the slots are added from left to right in groups of
// MET_FOLD, the group sums again, until one is left (met_fold).  Each translation unit gets its own copy of the fold kernel.
#pragma once
#include "common.h"

#define BST_THREADS 256
#define BST_PER 8                               // pixels per thread: t + BST_THREADS * j
#define BST_CHUNK (BST_THREADS * BST_PER)       // 2048 pixels: one workgroup's share (tests/test_gpu_metrics.py: BST_CHUNK)
#define BST_NB 8                                // values per (sample, band)
#define BST_NS 3                                // values per sample: sum of angles, pixels with an angle, pixels without
#define MET_FOLD 64                             // slots one thread of a fold level adds, left to right

// the larger of two magnitudes; a NaN stays
__device__ __forceinline__ double met_max(double m, double d) { return (d > m || d != d) ? d : m; }

// v[0 .. NV) of every thread, NV <= 8 -> the workgroup's value k in every lane of half-wave k (returned; lane 0 of it stores).  Thread
// (k, l) = (t / 32, t % 32) adds x[l], x[l + 32], .. x[l + 224] of value k in ascending order, then the 32 sums meet by the butterfly
// x = x + x[l ^ 16], .. x[l ^ 1] (the same bits in every lane: the additions commute).  MAXK: the index that is a maximum, not a sum.
// One barrier; red (NV * 256 doubles) is read until the caller's next barrier.
template <int NV, int MAXK>
__device__ __forceinline__ double met_reduce(double* red, const double* v, int t) {
#pragma unroll
    for (int k = 0; k < NV; ++k) red[k * BST_THREADS + t] = v[k];
    __syncthreads();
    const int k = t >> 5, l = t & 31;
    const bool is_max = k == MAXK;
    double x = 0.0;
    if (k < NV) {
        const double* r = red + k * BST_THREADS + l;
        x = r[0];
#pragma unroll
        for (int i = 1; i < BST_THREADS / 32; ++i) x = is_max ? met_max(x, r[32 * i]) : x + r[32 * i];
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
        const double y = __shfl_xor(x, o, 32);
        x = is_max ? met_max(x, y) : x + y;
    }
    return x;
}

// One level of the slot sum: dst[o][g][v] = src[o][g * MET_FOLD][v] + .. left to right over the up to MET_FOLD slots of group g, n slots and
// NV values per o.  C > 0: the values are eod_band_stats' (v < C * BST_NB with v % BST_NB == 7 is a maximum), and the last level (one group)
// stores to band / sample.
static __global__ void __launch_bounds__(256) met_fold_kernel(const double* src, double* dst, long long outer, long long n, int NV, int C, double* band,
                                                       double* sample) {
    const long long nout = (n + MET_FOLD - 1) / MET_FOLD, total = outer * nout * NV;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int v = (int)(i % NV);
        const long long g = (i / NV) % nout, o = i / (NV * nout);
        const bool is_max = v < C * BST_NB && (v % BST_NB) == 7;
        const long long first = g * MET_FOLD;
        const int cnt = (int)(n - first < MET_FOLD ? n - first : MET_FOLD);
        const double* s = src + (o * n + first) * NV + v;
        double acc = 0.0;
#pragma unroll 8
        for (int j = 0; j < cnt; ++j) {
            const double x = s[(long long)j * NV];
            acc = is_max ? met_max(acc, x) : acc + x;
        }
        if (band && nout == 1) {
            if (v < C * BST_NB) band[o * C * BST_NB + v] = acc;
            else sample[o * BST_NS + (v - C * BST_NB)] = acc;
        } else {
            dst[i] = acc;
        }
    }
}

// doubles of the levels between the slots and the result (the slots themselves not counted)
static inline long long met_fold_extra(long long outer, long long n, int NV) {
    long long extra = 0;
    for (n = (n + MET_FOLD - 1) / MET_FOLD; n > 1; n = (n + MET_FOLD - 1) / MET_FOLD) extra += outer * n * NV;
    return extra;
}

// the levels, launched in order; part holds outer * n * NV slots followed by met_fold_extra() doubles
static int met_fold(const char* what, double* part, long long outer, long long n, int NV, int C, double* out, double* band, double* sample,
                    hipStream_t stream) {
    double* src = part;
    double* next = part + outer * n * NV;
    for (;;) {
        const long long nout = (n + MET_FOLD - 1) / MET_FOLD, total = outer * nout * NV;
        double* dst = nout == 1 ? out : next;
        const long long blocks = (total + 255) / 256;
        hipLaunchKernelGGL(met_fold_kernel, dim3((unsigned)(blocks < 65535 ? blocks : 65535)), dim3(256), 0, stream, src, dst, outer, n, NV, C,
                           nout == 1 ? band : nullptr, sample);
        EOD_CHECK_LAUNCH(what);
        if (nout == 1) return EOD_OK;
        src = dst;
        next = dst + total;
        n = nout;
    }
}
