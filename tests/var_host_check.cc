// The bodies of eod_ddpm_var_pred / eod_ddpm_step_p0_var and the element of eod_hybrid_loss (eo_diffusion_amd/csrc/var_body.h) compiled for the
// host and run sample by sample, thread number by thread number.  Meant to be built with -ffp-contract=off -fsanitize=address,undefined: every
// tensor and table is a heap buffer of exactly its size, so a read or write outside it, and a misaligned 16-byte access, ends the run.
// N = 3, T = 50 (a cosine schedule), chw in {105 (the element form, a ragged last quad), 192 (the quad form)}, more and fewer threads than quads.
//   pred: kinds eps / x0 / v, clip on and off, timesteps {0, 1, T - 1} and {5, T, -1}: bit-equal to ddpm_pred_x0_thread / param_pred_thread on a
//         dense copy of the mean half; the variance half is NaN (never read).
//   step: timesteps {3, 1, T - 1}, {0, 1, T - 1} and {5, T, 2}; the mean half is NaN (never read).  z = 0, or a member at t = 0 (any z, v NaN):
//         bit-equal to ddpm_step_p0_thread.  Otherwise against the header's own lines written out here.
//   term: var_vlb_element on a grid of (x_0, p0, v) for a t > 0 level and the t = 0 level, x_0 = +-1 included.
// With a path as argv[1] the step and term cases are also written there as raw little-endian doubles, one line per case on stdout:
//   step <N> <chw> <T> <offset>: x, p0c, z, out [N chw each], o [2 N chw], t [N], betas, alphas, acp, sigma_min, half_gap [T each]
//   term <t0> <K> <c1> <lmin> <gap> <h> <offset>: x0, p0, v, term, dterm_dv [K each]       (the scalars printed with %.17g)
// Prints "ok <cases>" and returns 0.  tests/test_var_host.py builds and runs it, and compares the file with tests/var_ref.py.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../eo_diffusion_amd/csrc/var_body.h"

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

static bool same_bits(const float* a, const float* b, long long n) {
    for (long long i = 0; i < n; ++i) {
        if (a[i] != a[i] && b[i] != b[i]) continue;
        if (memcmp(a + i, b + i, 4) != 0) return false;
    }
    return true;
}

static const int T = 50, N = 3;
static std::vector<double> file;
static int cases = 0;

struct Tables {
    Buf<float> betas, alphas, acp, sa, s1, smin, hgap;
    std::vector<double> c1, lmin, gap;
    Tables() : betas(T), alphas(T), acp(T), sa(T), s1(T), smin(T), hgap(T), c1(T), lmin(T), gap(T) {
        auto f = [](double s) { const double c = cos(((s / T + 0.008) / 1.008) * M_PI * 0.5); return c * c; };
        float cum = 1.0f;
        for (int t = 0; t < T; ++t) {
            double b = 1.0 - f(t + 1) / f(t);
            b = b < 0.0 ? 0.0 : (b > 0.999 ? 0.999 : b);
            betas.p[t] = (float)b;
            alphas.p[t] = 1.0f - betas.p[t];
            cum = cum * alphas.p[t];
            acp.p[t] = cum;
            sa.p[t] = sqrtf(cum);
            s1.p[t] = sqrtf(1.0f - cum);
        }
        std::vector<double> bt(T);
        for (int t = 0; t < T; ++t) {
            const double ap = t ? (double)acp.p[t - 1] : 1.0;
            bt[t] = (double)betas.p[t] * (1.0 - ap) / (1.0 - (double)acp.p[t]);
            c1[t] = (double)betas.p[t] * sqrt(ap) / (1.0 - (double)acp.p[t]);
        }
        bt[0] = bt[1];
        for (int t = 0; t < T; ++t) {
            lmin[t] = log(bt[t]);
            gap[t] = log((double)betas.p[t]) - lmin[t];
            smin.p[t] = (float)sqrt(bt[t]);
            hgap.p[t] = (float)(gap[t] / 2.0);
        }
    }
};

template <bool VEC, typename F>
static void run_threads(F body, int threads) {
    for (int n = 0; n < N; ++n)
        for (int th = 0; th < threads; ++th) body(n, (long long)th, (long long)threads);
}

static int fail(const char* what, long long chw, int a, int b) {
    printf("FAILED %s chw %lld (%d, %d)\n", what, chw, a, b);
    return 1;
}

static int check_pred(const Tables& tb, long long chw, int threads) {
    const long long n = N * chw;
    const long long tsets[2][3] = {{0, 1, T - 1}, {5, T, -1}};
    for (int ts = 0; ts < 2; ++ts)
        for (int kind = 0; kind < 3; ++kind)
            for (int clip = 0; clip < 2; ++clip) {
                Buf<float> x(n), o(2 * n), dense(n), got(n), want(n);
                Buf<long long> t(N);
                for (int i = 0; i < N; ++i) t.p[i] = tsets[ts][i];
                for (long long i = 0; i < n; ++i) x.p[i] = 2.0f * rnd();
                for (int s = 0; s < N; ++s)
                    for (long long i = 0; i < chw; ++i) {
                        dense.p[s * chw + i] = o.p[2 * s * chw + i] = 3.0f * rnd();
                        o.p[(2 * s + 1) * chw + i] = NAN;
                    }
                VarArgs g = {x.p, o.p, nullptr, nullptr, t.p, nullptr, nullptr, kind == PARAM_EPS ? tb.acp.p : nullptr, kind == PARAM_EPS ? nullptr : tb.sa.p,
                             kind == PARAM_EPS ? nullptr : tb.s1.p, nullptr, nullptr, got.p, N, chw, T, kind, clip};
                DdpmP0Args d = {x.p, dense.p, nullptr, nullptr, t.p, nullptr, nullptr, tb.acp.p, want.p, N, chw, T, clip};
                ParamArgs p = {x.p, dense.p, t.p, tb.sa.p, tb.s1.p, 0.0f, 0.0f, want.p, nullptr, N, chw, T, kind, clip};
                if (chw % 4 == 0) run_threads<true>([&](int s, long long f, long long st) { var_pred_thread<true>(g, s, f, st); }, threads);
                else run_threads<false>([&](int s, long long f, long long st) { var_pred_thread<false>(g, s, f, st); }, threads);
                run_threads<false>([&](int s, long long f, long long st) {
                    if (kind == PARAM_EPS) ddpm_pred_x0_thread<false>(d, s, f, st);
                    else param_pred_thread<false>(p, s, f, st);
                }, 7);
                if (!same_bits(got.p, want.p, n)) return fail("pred", chw, kind, clip);
                for (int s = 0; s < N; ++s) {
                    const bool bad = t.p[s] < 0 || t.p[s] >= T;
                    for (long long i = 0; i < chw; ++i)
                        if ((got.p[s * chw + i] != got.p[s * chw + i]) != bad) return fail("pred poison", chw, kind, s);
                }
                ++cases;
            }
    return 0;
}

static int check_step(const Tables& tb, long long chw, int threads, bool to_file) {
    const long long n = N * chw;
    const long long tsets[3][3] = {{3, 1, T - 1}, {0, 1, T - 1}, {5, T, 2}};
    for (int ts = 0; ts < 3; ++ts)
        for (int zero_z = 0; zero_z < 2; ++zero_z) {
            Buf<float> x(n), p0(n), z(n), o(2 * n), got(n), want(n);
            Buf<long long> t(N);
            for (int i = 0; i < N; ++i) t.p[i] = tsets[ts][i];
            const bool has0 = ts == 1;
            for (long long i = 0; i < n; ++i) {
                x.p[i] = 2.0f * rnd();
                p0.p[i] = rnd();
                z.p[i] = zero_z ? 0.0f : 3.0f * rnd();
            }
            for (int s = 0; s < N; ++s)
                for (long long i = 0; i < chw; ++i) {
                    o.p[2 * s * chw + i] = NAN;
                    o.p[(2 * s + 1) * chw + i] = has0 ? NAN : 2.0f * rnd();
                }
            VarArgs g = {x.p, o.p, p0.p, z.p, t.p, tb.betas.p, tb.alphas.p, tb.acp.p, nullptr, nullptr, tb.smin.p, tb.hgap.p, got.p, N, chw, T, 0, 0};
            if (chw % 4 == 0) run_threads<true>([&](int s, long long f, long long st) { var_step_thread<true>(g, s, f, st); }, threads);
            else run_threads<false>([&](int s, long long f, long long st) { var_step_thread<false>(g, s, f, st); }, threads);
            DdpmP0Args d = {x.p, nullptr, p0.p, z.p, t.p, tb.betas.p, tb.alphas.p, tb.acp.p, want.p, N, chw, T, 0};
            run_threads<false>([&](int s, long long f, long long st) { ddpm_step_p0_thread<false>(d, s, f, st); }, 5);
            if (zero_z || has0) {
                if (!same_bits(got.p, want.p, n)) return fail("step against ddpm_step_p0", chw, ts, zero_z);
            } else {   // the header's lines: the mean of ddpm_step_p0 (its output at z = 0 is not the mean's bits at -0; so: recompute)
                for (int s = 0; s < N; ++s) {
                    const bool bad = t.p[s] < 0 || t.p[s] >= T;
                    const long long tn = bad ? 0 : t.p[s];
                    const float acp_prev = tb.acp.p[tn > 0 ? tn - 1 : 0], acp_t = tb.acp.p[tn];
                    const float m_x0 = tb.betas.p[tn] * sqrtf(acp_prev) / (1.0f - acp_t);
                    const float m_xt = (1.0f - acp_prev) * sqrtf(tb.alphas.p[tn]) / (1.0f - acp_t);
                    for (long long i = s * chw; i < (s + 1) * chw; ++i) {
                        const float a = m_x0 * p0.p[i];
                        const float b = m_xt * x.p[i];
                        const float mean = a + b;
                        const float v = o.p[(2 * s + 1) * chw + (i - s * chw)];
                        const float v1 = v + 1.0f;
                        const float frac = v1 * 0.5f;
                        const float arg = frac * tb.hgap.p[tn];
                        const float sg = tb.smin.p[tn] * expf(arg);
                        const float sz = sg * z.p[i];
                        want.p[i] = bad ? NAN : mean + sz;
                    }
                }
                if (!same_bits(got.p, want.p, n)) return fail("step against its lines", chw, ts, zero_z);
                if (to_file) {
                    printf("step %d %lld %d %zu\n", N, chw, T, file.size());
                    for (const Buf<float>* b : {&x, &p0, &z, &got, &o})
                        for (long long i = 0; i < b->n; ++i) file.push_back((double)b->p[i]);
                    for (int i = 0; i < N; ++i) file.push_back((double)t.p[i]);
                    for (const Buf<float>* b : {&tb.betas, &tb.alphas, &tb.acp, &tb.smin, &tb.hgap})
                        for (long long i = 0; i < b->n; ++i) file.push_back((double)b->p[i]);
                }
            }
            ++cases;
        }
    return 0;
}

static void check_terms(const Tables& tb) {
    const double h = 1.0 / 255.0;
    for (int tn : {0, 1, 7, T - 1}) {
        VarLevel L = {(double)tb.sa.p[tn], (double)tb.s1.p[tn], tb.c1[tn], tb.lmin[tn], tb.gap[tn], tn == 0};
        std::vector<double> x0s, p0s, vs, terms, dvs;
        for (int i = 0; i < 400; ++i) {
            double x0 = (double)rnd();
            if (i % 10 == 0) x0 = 1.0;
            if (i % 10 == 5) x0 = -1.0;
            const double spread = tn == 0 ? 0.02 : 1.0;          // (at t = 0 the standard deviation is about 0.01: stay within a few of it)
            const double p0 = tn == 0 ? x0 + spread * (double)rnd() : (double)(1.5f * rnd());
            const double v = i % 7 == 0 ? -1.0 : (double)(1.5f * rnd());
            double term, dv;
            var_vlb_element(L, x0, p0, v, h, term, dv);
            x0s.push_back(x0); p0s.push_back(p0); vs.push_back(v); terms.push_back(term); dvs.push_back(dv);
        }
        printf("term %d %zu %.17g %.17g %.17g %.17g %zu\n", (int)(tn == 0), x0s.size(), L.c1, L.lmin, L.gap, h, file.size());
        for (const std::vector<double>* a : {&x0s, &p0s, &vs, &terms, &dvs}) file.insert(file.end(), a->begin(), a->end());
        ++cases;
    }
}

int main(int argc, char** argv) {
    Tables tb;
    for (long long chw : {105LL, 192LL})
        for (int threads : {1, 5, 64}) {
            if (check_pred(tb, chw, threads)) return 1;
            if (check_step(tb, chw, threads, threads == 5)) return 1;
        }
    // sigma at v = -1 is sigma_min itself, bit for bit
    for (int t = 0; t < T; ++t) {
        const float s = var_sigma(-1.0f, tb.smin.p[t], tb.hgap.p[t]);
        if (memcmp(&s, &tb.smin.p[t], 4) != 0) return fail("sigma at v = -1", 0, t, 0);
    }
    check_terms(tb);
    if (argc > 1) {
        FILE* f = fopen(argv[1], "wb");
        if (!f || fwrite(file.data(), sizeof(double), file.size(), f) != file.size()) return 2;
        fclose(f);
    }
    printf("ok %d\n", cases);
    return 0;
}
