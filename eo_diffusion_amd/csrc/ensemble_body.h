// The per-pixel step of the ensemble statistics (csrc/ensemble.hip): the order-preserving key of an fp32 member, the
// fixed compare-exchange network that sorts up to 64 keys in registers, the pick of an order statistic whose index is a launch argument,
// and the quantile between two of them.  Plain C++ behind ENS_FN, so that a host build can run the same text.
#pragma once
#include <stdint.h>
#include <string.h>

#ifndef ENS_FN
#define ENS_FN static inline
#endif

#define ENS_MAXB 64             // members of a stack
#define ENS_MAXQ 8              // quantiles of one eod_scene_quantiles call
#define ENS_MAXL 4              // central intervals of one eod_ensemble_stats call
#define ENS_TOP 0xffffffffu     // the key of every NaN, and of the pads behind member B - 1

ENS_FN uint32_t ens_bits(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    return u;
}
ENS_FN float ens_float(uint32_t u) {
    float x;
    memcpy(&x, &u, 4);
    return x;
}

// -inf < .. < -0.0 < +0.0 < .. < +inf < NaN as unsigned integers: the sign bit of a non-negative float is flipped, every bit of a negative
// one; a NaN of either sign becomes ENS_TOP (no other float does: 0x7fffffff is itself a NaN)
ENS_FN uint32_t ens_key(float x) {
    const uint32_t u = ens_bits(x);
    const uint32_t k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return (u & 0x7fffffffu) > 0x7f800000u ? ENS_TOP : k;
}
// the float of a key: the member's own bits; ENS_TOP gives the quiet NaN 0x7fc00000
ENS_FN float ens_unkey(uint32_t k) {
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return ens_float(k == ENS_TOP ? 0x7fc00000u : u);
}

// Batcher's bitonic network on P = 2^p keys, ascending: p (p + 1) / 2 layers of P / 2 compare-exchanges, each an integer minimum and an
// integer maximum (P = 64: 21 layers, 672 exchanges, 1344 operations).  Every index is a constant after unrolling, so k stays in registers.
template <int P>
ENS_FN void ens_sort(uint32_t (&k)[P]) {
#pragma unroll
    for (int size = 2; size <= P; size <<= 1) {
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
#pragma unroll
            for (int i = 0; i < P; ++i) {
                const int j = i ^ stride;
                if (j > i) {
                    const uint32_t a = k[i], b = k[j];
                    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
                    const bool up = (i & size) == 0;
                    k[i] = up ? lo : hi;
                    k[j] = up ? hi : lo;
                }
            }
        }
    }
}

// k[at] of the sorted keys for an index that is not a constant: a tree of selects over the unrolled array, one level per bit of `at` (a
// dynamically indexed register array would go to scratch).  P - 1 selects under log2(P) conditions: a chain of P selects `i == at ? k[i] : v`
// has P conditions, which the compiler hoists out of the pixel loop into more scalar registers than there are.  0 <= at < P.
template <int P>
ENS_FN uint32_t ens_pick(const uint32_t (&k)[P], int at) {
    uint32_t t[P];
#pragma unroll
    for (int i = 0; i < P; ++i) t[i] = k[i];
#pragma unroll
    for (int w = P / 2, bit = 0; w >= 1; w >>= 1, ++bit) {
        const bool odd = ((at >> bit) & 1) != 0;
#pragma unroll
        for (int m = 0; m < w; ++m) t[m] = odd ? t[2 * m + 1] : t[2 * m];
    }
    return t[0];
}

// the quantile (at, frac) of the sorted keys: x_(at) itself at frac == 0, else lo + frac * (hi - lo), every operation rounded separately in
// fp32 (the translation unit is built with -ffp-contract=off), the form of eod_dyn_threshold
template <int P>
ENS_FN float ens_quantile(const uint32_t (&k)[P], int at, float frac) {
    const float lo = ens_unkey(ens_pick<P>(k, at));
    if (frac == 0.0f) return lo;
    const float hi = ens_unkey(ens_pick<P>(k, (at + 1) & (P - 1)));  // (frac > 0 comes with at + 1 < B <= P: the callers refuse anything else)
    const float d = hi - lo;
    const float m = frac * d;
    return lo + m;
}
