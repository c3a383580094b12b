// The bodies of eod_ddpm_pred_x0 / eod_ddpm_step_p0 (eo_diffusion_amd/csrc/ddpm_p0_body.h) compiled for the host and run sample by sample,
// thread number by thread number, against a whole-tensor evaluation of the contract of include/eodiff.h written straight from its lines.
// Meant to be built with -ffp-contract=off -fsanitize=address,undefined: every tensor and table is a heap buffer of exactly its size, so a
// read or write outside it, and a misaligned 16-byte access, ends the run.  Both access forms, chw in {126, 768} (126 is no multiple of 4:
// the element-wise form with a ragged last quad), N in {1, 3}, T in {8, 1000}, timesteps all positive, all 0, all T - 1, mixed with a 0, and
// with one member outside [0, T) among positive ones (its sample NaN; the batch-wide branch then reads acp_prev of index 0, not -1), clip on
// and off, more and fewer threads than quads.  Prints "ok <cases>" and returns 0 when every output is bit-equal.
// tests/test_ancestral_host.py builds and runs it.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../eo_diffusion_amd/csrc/ddpm_p0_body.h"

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

// ------------------------------------------------------------------------------------------------ the contract, whole tensors
static void ref_pred(const DdpmP0Args& g, float* out) {
    for (int n = 0; n < g.N; ++n) {
        const long long t = g.t[n];
        const bool bad = t < 0 || t >= g.T;
        const float acp_t = g.acp[bad ? 0 : t];
        const float c_x0 = sqrtf(1.0f / acp_t);
        const float c_pred = sqrtf(1.0f / acp_t - 1.0f);
        for (long long i = 0; i < g.chw; ++i) {
            const float u = c_x0 * g.x[n * g.chw + i];
            const float v = c_pred * g.e[n * g.chw + i];
            float p0 = u - v;
            if (g.clip) p0 = p0 != p0 ? p0 : fminf(fmaxf(p0, -1.0f), 1.0f);   // torch.clamp: a NaN stays NaN
            out[n * g.chw + i] = bad ? NAN : p0;
        }
    }
}

static void ref_step(const DdpmP0Args& g, float* out) {
    long long tmin = g.t[0];
    for (int n = 1; n < g.N; ++n) tmin = g.t[n] < tmin ? g.t[n] : tmin;
    const bool all_pos = tmin > 0;
    for (int n = 0; n < g.N; ++n) {
        const bool bad = g.t[n] < 0 || g.t[n] >= g.T;
        const long long t = bad ? 0 : g.t[n];
        const float beta_t = g.betas[t], alpha_t = g.alphas[t], acp_t = g.acp[t];
        float m_x0, m_xt = 0.0f, std = 0.0f;
        if (all_pos) {
            const float acp_prev = g.acp[t > 0 ? t - 1 : 0];
            m_x0 = beta_t * sqrtf(acp_prev) / (1.0f - acp_t);
            m_xt = (1.0f - acp_prev) * sqrtf(alpha_t) / (1.0f - acp_t);
            std = sqrtf(beta_t * (1.0f - acp_prev) / (1.0f - acp_t));
        } else {
            m_x0 = beta_t / (1.0f - acp_t);
        }
        for (long long i = 0; i < g.chw; ++i) {
            const float x = g.x[n * g.chw + i], p = g.p0c[n * g.chw + i], z = g.z[n * g.chw + i];
            float mean;
            if (all_pos) {
                const float a = m_x0 * p;
                const float b = m_xt * x;
                mean = a + b;
            } else {
                mean = m_x0 * p;
            }
            const float sz = std * z;
            out[n * g.chw + i] = bad ? NAN : mean + sz;
        }
    }
}

// ------------------------------------------------------------------------------------------------ the bodies, as the kernels run them
template <bool STEP, bool VEC>
static void run(const DdpmP0Args& g, long long threads) {
    for (int n = 0; n < g.N; ++n)
        for (long long tid = 0; tid < threads; ++tid) {
            if (STEP) ddpm_step_p0_thread<VEC>(g, n, tid, threads);
            else ddpm_pred_x0_thread<VEC>(g, n, tid, threads);
        }
}

static int failures = 0, cases = 0;
static void same(const char* what, const float* a, const float* b, long long n, const DdpmP0Args& g, int vec, int tcase) {
    ++cases;
    if (memcmp(a, b, (size_t)n * sizeof(float)) == 0) return;
    long long bad = 0, first = -1;
    for (long long i = 0; i < n; ++i)
        if (memcmp(a + i, b + i, sizeof(float))) { if (first < 0) first = i; ++bad; }
    printf("MISMATCH %s N=%d chw=%lld T=%d clip=%d vec=%d t-case %d: %lld of %lld differ, first at %lld (%g vs %g)\n", what, g.N, g.chw, g.T,
           g.clip, vec, tcase, bad, n, first, (double)a[first], (double)b[first]);
    ++failures;
}

static void one_case(int N, long long chw, int T, int tcase, int clip) {
    Buf<float> betas(T), alphas(T), acp(T), x(N * chw), e(N * chw), z(N * chw), p0(N * chw), p0r(N * chw), out(N * chw), outr(N * chw);
    Buf<long long> t(N);
    double prod = 1.0;
    for (int i = 0; i < T; ++i) {   // the cosine schedule's shape: betas rise to the 0.999 clip
        const double f0 = cos(((double)i / T + 0.008) / 1.008 * M_PI * 0.5), f1 = cos(((double)(i + 1) / T + 0.008) / 1.008 * M_PI * 0.5);
        double b = 1.0 - (f1 * f1) / (f0 * f0);
        b = b > 0.999 ? 0.999 : b;
        betas.p[i] = (float)b;
        alphas.p[i] = 1.0f - betas.p[i];
        prod *= alphas.p[i];
        acp.p[i] = (float)prod;
    }
    for (long long i = 0; i < N * chw; ++i) { x.p[i] = 3.0f * rnd(); e.p[i] = 3.0f * rnd(); z.p[i] = 3.0f * rnd(); }
    for (int n = 0; n < N; ++n) {
        const long long mixed[3] = {0, 3, T - 1}, range[3] = {5, (long long)T + 2, 3}, neg[3] = {5, -1, 3};
        t.p[n] = tcase == 0 ? 5 : tcase == 1 ? 0 : tcase == 2 ? T - 1 : tcase == 3 ? mixed[n % 3] : tcase == 4 ? range[(n + 1) % 3] : neg[(n + 1) % 3];
    }
    DdpmP0Args g;
    memset(&g, 0, sizeof(g));
    g.x = x.p; g.e = e.p; g.z = z.p; g.t = t.p; g.betas = betas.p; g.alphas = alphas.p; g.acp = acp.p;
    g.N = N; g.chw = chw; g.T = T; g.clip = clip;
    g.out = p0r.p;
    ref_pred(g, p0r.p);
    g.p0c = p0r.p;
    ref_step(g, outr.p);
    const long long quads = (chw + 3) / 4;
    const long long threads[3] = {256, quads + 37, 7};
    for (int vec = 0; vec < 2; ++vec) {
        if (vec && chw % 4) continue;
        for (int th = 0; th < 3; ++th) {
            for (long long i = 0; i < N * chw; ++i) p0.p[i] = out.p[i] = -123.0f;
            g.out = p0.p;
            if (vec) run<false, true>(g, threads[th]); else run<false, false>(g, threads[th]);
            same("pred_x0", p0.p, p0r.p, N * chw, g, vec, tcase);
            g.out = out.p;
            if (vec) run<true, true>(g, threads[th]); else run<true, false>(g, threads[th]);
            same("step_p0", out.p, outr.p, N * chw, g, vec, tcase);
        }
    }
}

int main() {
    const int Ns[2] = {1, 3}, Ts[2] = {8, 1000};
    const long long chws[2] = {126, 768};
    for (int ni = 0; ni < 2; ++ni)
        for (int ci = 0; ci < 2; ++ci)
            for (int ti = 0; ti < 2; ++ti)
                for (int tcase = 0; tcase < 6; ++tcase)
                    for (int clip = 0; clip < 2; ++clip) one_case(Ns[ni], chws[ci], Ts[ti], tcase, clip);
    if (failures) { printf("FAILED %d of %d\n", failures, cases); return 1; }
    printf("ok %d\n", cases);
    return 0;
}
