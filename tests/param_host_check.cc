// The bodies of eod_param_pred / eod_ddpm_param_pred / eod_q_sample_v (eo_diffusion_amd/csrc/param_body.h) compiled for the host and run sample
// by sample, thread number by thread number, against a whole-tensor evaluation of the contract of include/eodiff_param.h written straight from
// its lines.  Meant to be built with -ffp-contract=off -fsanitize=address,undefined: every tensor and table is a heap buffer of exactly its
// size, so a read or write outside it, and a misaligned 16-byte access, ends the run.  Both access forms, chw in {77, 768} (77 is no multiple
// of 4: the element-wise form with a ragged last quad), kinds x0 and v, clip on and off, with and without the noise estimate, the levels
// a in {0 (v only), 2.43e-9, 0.37, 0.99995875}; the per-sample forms with N = 3, T = 1000 and timesteps {0, T - 1, 500}, {0, T, 5} and
// {5, -1, 3} (a member outside [0, T): its sample NaN, the others untouched by it); more and fewer threads than quads.
// With a path as argv[1] every case's inputs and outputs are also written there as raw little-endian words, one line per case on stdout:
//   case <form> <kind> <clip> <with_e> <N> <chw> <T> <a> <s1> <offset in floats>
// and at the offset x, o, out0, out1 [N * chw each], then for the per-sample forms t (N int64 = 2 N words), sa_tab, s1_tab [T each].
// Prints "ok <cases>" and returns 0 when every output is bit-equal.  tests/test_param_host.py builds and runs it, and compares the file with
// tests/param_ref.py.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../eo_diffusion_amd/csrc/param_body.h"

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static float rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (float)((rng_state >> 40) & 0xFFFFFF) / 8388608.0f - 1.0f;
}

template <typename T>
struct Buf {   // an exactly sized heap buffer
    T* p;
    long long n;
    explicit Buf(long long n_) : p((T*)malloc((size_t)n_ * sizeof(T))), n(n_) {}
    ~Buf() { free(p); }
    Buf(const Buf&) = delete;
};

enum { FORM_SCALAR = 0, FORM_DDPM = 1, FORM_PAIR = 2 };

// ------------------------------------------------------------------------------------------------ the contract, whole tensors
static void ref(const ParamArgs& g, int form, float* out0, float* out1) {
    for (int n = 0; n < g.N; ++n) {
        bool bad = false;
        float sa, s1;
        if (form == FORM_SCALAR) {
            sa = sqrtf(g.a);
            s1 = g.s1;
        } else {
            const long long t = g.t[n];
            bad = t < 0 || t >= g.T;
            sa = g.sa_tab[bad ? 0 : t];
            s1 = g.s1_tab[bad ? 0 : t];
        }
        for (long long i = n * g.chw; i < (n + 1) * g.chw; ++i) {
            const float x = g.x[i], o = g.o[i];
            if (form == FORM_PAIR) {
                const float p = sa * x;
                const float q = s1 * o;
                const float r = sa * o;
                const float w = s1 * x;
                out0[i] = bad ? NAN : p + q;
                out1[i] = bad ? NAN : r - w;
                continue;
            }
            float p, e;
            if (g.kind == PARAM_V) {
                const float u = sa * x;
                const float w = s1 * o;
                p = u - w;
                const float r = sa * o;
                const float q = s1 * x;
                e = r + q;
            } else {
                p = o;
                const float u = sa * o;
                const float d = x - u;
                e = d / s1;
            }
            if (g.clip) p = p != p ? p : fminf(fmaxf(p, -1.0f), 1.0f);   // torch.clamp: a NaN stays NaN
            out0[i] = bad ? NAN : p;
            if (out1) out1[i] = bad ? NAN : e;
        }
    }
}

// ------------------------------------------------------------------------------------------------ the bodies, as the kernels run them
template <bool VEC>
static void run(const ParamArgs& g, int form, long long threads) {
    for (int n = 0; n < g.N; ++n)
        for (long long tid = 0; tid < threads; ++tid) {
            if (form == FORM_PAIR) q_sample_v_thread<VEC>(g, n, tid, threads);
            else param_pred_thread<VEC>(g, n, tid, threads);
        }
}

static int failures = 0, cases = 0;
static FILE* dump = nullptr;
static long long dumped = 0;

static void put(const void* p, long long words) {
    if (fwrite(p, 4, (size_t)words, dump) != (size_t)words) { printf("write failed\n"); exit(2); }
    dumped += words;
}

static void same(const char* what, const float* a, const float* b, long long n, int form, const ParamArgs& g, int vec, long long threads) {
    if (memcmp(a, b, (size_t)n * sizeof(float)) == 0) return;
    long long bad = 0, first = -1;
    for (long long i = 0; i < n; ++i)
        if (memcmp(a + i, b + i, sizeof(float))) { if (first < 0) first = i; ++bad; }
    printf("MISMATCH %s form=%d kind=%d clip=%d N=%d chw=%lld vec=%d threads=%lld: %lld of %lld differ, first at %lld (%g vs %g)\n", what, form,
           g.kind, g.clip, g.N, g.chw, vec, threads, bad, n, first, (double)a[first], (double)b[first]);
    ++failures;
}

static void one_case(int form, int kind, int clip, int with_e, int N, long long chw, int T, float a, int tcase) {
    const long long n = N * chw;
    Buf<float> x(n), o(n), out0(n), out1(n), want0(n), want1(n), sa_tab(T > 0 ? T : 1), s1_tab(T > 0 ? T : 1);
    Buf<long long> t(N);
    double prod = 1.0;
    for (int i = 0; i < T; ++i) {   // the cosine schedule's shape: betas rise to the 0.999 clip
        const double f0 = cos(((double)i / T + 0.008) / 1.008 * M_PI * 0.5), f1 = cos(((double)(i + 1) / T + 0.008) / 1.008 * M_PI * 0.5);
        double b = 1.0 - (f1 * f1) / (f0 * f0);
        b = b > 0.999 ? 0.999 : b;
        prod *= 1.0 - (double)(float)b;
        sa_tab.p[i] = sqrtf((float)prod);
        s1_tab.p[i] = sqrtf(1.0f - (float)prod);
    }
    for (long long i = 0; i < n; ++i) { x.p[i] = 3.0f * rnd(); o.p[i] = 3.0f * rnd(); }
    const long long tc[3][3] = {{0, (long long)T - 1, 500}, {0, (long long)T, 5}, {5, -1, 3}};
    for (int i = 0; i < N; ++i) t.p[i] = tc[tcase][i % 3];
    ParamArgs g;
    memset(&g, 0, sizeof(g));
    g.x = x.p; g.o = o.p; g.N = N; g.chw = chw; g.kind = kind; g.clip = clip;
    if (form == FORM_SCALAR) { g.a = a; g.s1 = sqrtf(1.0f - a); }
    else { g.t = t.p; g.sa_tab = sa_tab.p; g.s1_tab = s1_tab.p; g.T = T; }
    const bool two = form == FORM_PAIR || with_e;
    ref(g, form, want0.p, two ? want1.p : nullptr);
    const long long quads = (chw + 3) / 4;
    const long long threads[3] = {256, quads + 37, 7};
    for (int vec = 0; vec < 2; ++vec) {
        if (vec && chw % 4) continue;
        for (int th = 0; th < 3; ++th) {
            for (long long i = 0; i < n; ++i) out0.p[i] = out1.p[i] = -123.0f;
            g.out0 = out0.p;
            g.out1 = two ? out1.p : nullptr;
            if (vec) run<true>(g, form, threads[th]); else run<false>(g, form, threads[th]);
            same("out0", out0.p, want0.p, n, form, g, vec, threads[th]);
            if (two) same("out1", out1.p, want1.p, n, form, g, vec, threads[th]);
            else for (long long i = 0; i < n; ++i) if (out1.p[i] != -123.0f) { printf("out1 written without e_t\n"); ++failures; break; }
        }
    }
    ++cases;
    if (!dump) return;
    printf("case %d %d %d %d %d %lld %d %.9g %.9g %lld\n", form, kind, clip, two ? 1 : 0, N, chw, T, (double)g.a, (double)g.s1, dumped);
    put(x.p, n); put(o.p, n); put(want0.p, n);
    if (!two) for (long long i = 0; i < n; ++i) want1.p[i] = 0.0f;
    put(want1.p, n);
    if (form != FORM_SCALAR) { put(t.p, 2LL * N); put(sa_tab.p, T); put(s1_tab.p, T); }
}

int main(int argc, char** argv) {
    if (argc > 1) {
        dump = fopen(argv[1], "wb");
        if (!dump) { printf("cannot open %s\n", argv[1]); return 2; }
    }
    const long long chws[2] = {77, 768};
    const float levels[4] = {0.0f, 2.43e-9f, 0.37f, 0.99995875f};
    for (int ci = 0; ci < 2; ++ci) {
        for (int kind = PARAM_X0; kind <= PARAM_V; ++kind)
            for (int clip = 0; clip < 2; ++clip) {
                for (int with_e = 0; with_e < 2; ++with_e)
                    for (int li = kind == PARAM_V ? 0 : 1; li < 4; ++li) one_case(FORM_SCALAR, kind, clip, with_e, 1, chws[ci], 0, levels[li], 0);
                for (int tcase = 0; tcase < 3; ++tcase) one_case(FORM_DDPM, kind, clip, 0, 3, chws[ci], 1000, 0.0f, tcase);
            }
        for (int tcase = 0; tcase < 3; ++tcase) one_case(FORM_PAIR, PARAM_V, 0, 1, 3, chws[ci], 1000, 0.0f, tcase);
    }
    if (dump) fclose(dump);
    if (failures) { printf("FAILED %d of %d\n", failures, cases); return 1; }
    printf("ok %d\n", cases);
    return 0;
}
