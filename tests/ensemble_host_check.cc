// The per-pixel step of the ensemble statistics (csrc/ensemble_body.h) compiled for the host: the key order and its inverse, the sorting
// network of every padded size against std::sort on random members with NaNs, zeros of both signs and pads, the select-tree pick at every
// index, and the quantile against the same three fp32 operations written out.  Built with -fsanitize=address,undefined by
// tests/test_ensemble_host.py and run as a program of its own; prints "ok <checks>".
#include "../eo_diffusion_amd/csrc/ensemble_body.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

static long checks = 0, bad = 0;
static void expect(bool ok) {
    ++checks;
    bad += ok ? 0 : 1;
}

template <int P>
static void run() {
    for (int it = 0; it < 500; ++it) {
        uint32_t k[P];
        std::vector<uint32_t> v(P);
        const int B = 1 + rand() % P;
        for (int i = 0; i < P; ++i) {
            float x = (float)(rand() % 17 - 8) * 0.37f;
            if (rand() % 23 == 0) x = NAN;
            if (rand() % 19 == 0) x = -0.0f;
            if (rand() % 29 == 0) x = -INFINITY;
            k[i] = i < B ? ens_key(x) : ENS_TOP;
            v[i] = k[i];
        }
        ens_sort<P>(k);
        std::sort(v.begin(), v.end());
        for (int i = 0; i < P; ++i) expect(k[i] == v[i]);
        for (int at = 0; at < P; ++at) expect(ens_pick<P>(k, at) == v[at]);
        for (int at = 0; at < B; ++at) expect(ens_bits(ens_quantile<P>(k, at, 0.0f)) == ens_bits(ens_unkey(v[at])));
        for (int at = 0; at + 1 < B; ++at) {
            const float q = ens_quantile<P>(k, at, 0.25f);
            const float lo = ens_unkey(v[at]), hi = ens_unkey(v[at + 1]);
            const float d = hi - lo;
            const float m = 0.25f * d;
            const float w = lo + m;
            expect(ens_bits(q) == ens_bits(w) || (q != q && w != w));
        }
    }
}

int main() {
    srand(12345);
    const float t[] = {-INFINITY, -3.5f, -1e-45f, -0.0f, 0.0f, 1e-45f, 2.0f, INFINITY};
    for (int i = 0; i + 1 < 8; ++i) expect(ens_key(t[i]) < ens_key(t[i + 1]));
    for (float x : t) expect(ens_bits(ens_unkey(ens_key(x))) == ens_bits(x) && ens_key(x) != ENS_TOP);
    expect(ens_key(NAN) == ENS_TOP && ens_key(-NAN) == ENS_TOP && ens_bits(ens_unkey(ENS_TOP)) == 0x7fc00000u);
    run<1>();
    run<2>();
    run<4>();
    run<8>();
    run<16>();
    run<32>();
    run<64>();
    if (bad) {
        printf("FAILED %ld of %ld\n", bad, checks);
        return 1;
    }
    printf("ok %ld\n", checks);
    return 0;
}
