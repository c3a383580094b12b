// The bodies of the coarse-grid CG kernels (eo_diffusion_amd/csrc/psf_cg_body.h) compiled for the host and run tile by tile, phase by phase,
// thread number by thread number, against a whole-plane evaluation of the contract of include/eodiff.h written straight from its lines (padded
// planes, sequential adds).  Meant to be built with -ffp-contract=off -fsanitize=address,undefined: every tensor is a heap buffer of exactly
// its size, so a read or write outside a plane or a table, and a misaligned 16-byte access, ends the run.  Planes of 1 x 1, planes narrower
// than the half-width b, b in {0, 3, 24}, several ragged tiles, both access forms, every mask form, the staging with d = r + beta d.  Prints
// "ok <cases>" and returns 0 when every tensor is bit-equal and every total is within 1e-12 of a whole-plane float64 sum (relative to the sum
// of the absolute products).  tests/test_psf_cg_host.py builds and runs it.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../eo_diffusion_amd/csrc/psf_cg_body.h"

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static float rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (float)((rng_state >> 40) & 0xFFFFFF) / 8388608.0f - 1.0f;
}

template <typename T> struct Buf {   // an exactly sized heap buffer
    T* p;
    long long n;
    explicit Buf(long long n_) : p((T*)malloc((size_t)n_ * sizeof(T))), n(n_) {}
    ~Buf() { free(p); }
    Buf(const Buf&) = delete;
    void fill() { for (long long i = 0; i < n; ++i) p[i] = (T)rnd(); }
    void binary() { for (long long i = 0; i < n; ++i) p[i] = rnd() > -0.4f ? (T)1 : (T)0; }
    void nan() { memset(p, 0xff, (size_t)n * sizeof(T)); }
};

static int failures = 0, cases = 0;
static void same(const char* what, const float* a, const float* b, long long n, const CgArgs& g, int form) {
    ++cases;
    if (memcmp(a, b, (size_t)n * sizeof(float)) == 0) return;
    long long bad = 0, first = -1;
    for (long long i = 0; i < n; ++i)
        if (memcmp(a + i, b + i, sizeof(float))) { if (first < 0) first = i; ++bad; }
    printf("MISMATCH %s b=%d %dx%d form=%d: %lld of %lld differ, first at %lld (%g vs %g)\n", what, g.b, g.Hc, g.Wc, form, bad, n, first,
           (double)a[first], (double)b[first]);
    ++failures;
}
static void close_to(const char* what, double got, double want, double scale, const CgArgs& g, int form) {
    ++cases;
    if (fabs(got - want) <= 1e-12 * scale) return;
    printf("MISMATCH %s b=%d %dx%d form=%d: %.17g vs %.17g (scale %g)\n", what, g.b, g.Hc, g.Wc, form, got, want, scale);
    ++failures;
}

// ------------------------------------------------------------------------------------------------ the contract, whole planes
static void ref_gram(const CgArgs& g, const float* d, float* q, double* sigma, double* scale) {
    const int b = g.b, nb = 2 * b + 1, Hc = g.Hc, Wc = g.Wc, PW = Wc + 2 * b, PH = Hc + 2 * b;
    const size_t chw = (size_t)Hc * Wc;
    for (long long pl = 0; pl < (long long)g.B * g.K; ++pl) {
        const float* dp = d + pl * chw;
        const float* m = cg_mask_plane(g, pl);
        std::vector<float> pad((size_t)Hc * PW, 0.0f), t((size_t)PH * Wc, 0.0f);
        for (int y = 0; y < Hc; ++y)
            for (int x = 0; x < Wc; ++x) pad[(size_t)y * PW + x + b] = m ? m[(size_t)y * Wc + x] * dp[(size_t)y * Wc + x] : dp[(size_t)y * Wc + x];
        for (int y = 0; y < Hc; ++y)
            for (int x = 0; x < Wc; ++x) {
                float acc = g.gx[(size_t)x * nb] * pad[(size_t)y * PW + x];
                for (int j = 1; j < nb; ++j) {
                    const float pr = g.gx[(size_t)x * nb + j] * pad[(size_t)y * PW + x + j];
                    acc = acc + pr;
                }
                t[(size_t)(y + b) * Wc + x] = acc;
            }
        double s = 0.0, sc = 0.0;
        for (int y = 0; y < Hc; ++y)
            for (int x = 0; x < Wc; ++x) {
                float acc = g.gy[(size_t)y * nb] * t[(size_t)y * Wc + x];
                for (int j = 1; j < nb; ++j) {
                    const float pr = g.gy[(size_t)y * nb + j] * t[(size_t)(y + j) * Wc + x];
                    acc = acc + pr;
                }
                const float dv = dp[(size_t)y * Wc + x];
                const float mq = m ? m[(size_t)y * Wc + x] * acc : acc;
                const float md = g.mu * dv;
                const float o = mq + md;
                q[pl * chw + (size_t)y * Wc + x] = o;
                s += (double)dv * (double)o;
                sc += fabs((double)dv * (double)o);
            }
        sigma[pl] = s;
        scale[pl] = sc;
    }
}

// ------------------------------------------------------------------------------------------------ the kernels' bodies, as the kernels run them
template <bool VECQ, bool FUSE>
static void run_gram(const CgArgs& g) {
    CgLds* s = (CgLds*)malloc(sizeof(CgLds));
    const long long items = (long long)g.B * g.K * g.tiles_x * g.tiles_y;
    for (long long item = 0; item < items; ++item) {
        memset(s, 0xff, sizeof(*s));   // NaN: nothing may depend on what an earlier tile left behind
        double part[CG_THREADS];
        for (int phase = 0; phase < 3; ++phase)
            for (int tid = 0; tid < CG_THREADS; ++tid) part[tid] = psf_cg_gram_phase<VECQ, FUSE>(phase, g, *s, item, tid);
        g.slots[item] = psf_cg_tile_sum_host(part);
    }
    free(s);
}
template <bool VECQ>
static void run_elem(int mode, const CgArgs& g) {
    const long long items = (long long)g.B * g.K * g.tiles_x * g.tiles_y;
    for (long long item = 0; item < items; ++item) {
        double part[CG_THREADS];
        for (int tid = 0; tid < CG_THREADS; ++tid) part[tid] = psf_cg_elem<VECQ>(mode, g, item, tid);
        if (mode != 2) g.slots[item] = psf_cg_tile_sum_host(part);
    }
}
static void run_sum(int mode, const CgArgs& g) {
    CgSumLds* s = (CgSumLds*)malloc(sizeof(CgSumLds));
    for (long long plane = 0; plane < (long long)g.B * g.K; ++plane) {
        memset(s, 0xff, sizeof(*s));
        for (int phase = 0; phase <= 9; ++phase)
            for (int tid = 0; tid < CG_THREADS; ++tid) psf_cg_sum_phase(phase, mode, g, *s, plane, tid);
    }
    free(s);
}

static void one_case(int b, int Hc, int Wc, int mask_form, float mu) {
    const int B = 2, K = 2, nb = 2 * b + 1;
    const long long P = B * K, chw = (long long)Hc * Wc;
    CgArgs g;
    memset(&g, 0, sizeof(g));
    g.b = b; g.B = B; g.K = K; g.Hc = Hc; g.Wc = Wc; g.mu = mu; g.lambda = 0.75f;
    g.mask_b1 = mask_form == 1 || mask_form == 2;
    g.mask_c1 = mask_form == 2;
    g.tiles_x = (Wc + CG_T - 1) / CG_T;
    g.tiles_y = (Hc + CG_T - 1) / CG_T;
    const long long tiles = (long long)g.tiles_x * g.tiles_y;
    Buf<float> d(P * chw), r(P * chw), mask((g.mask_b1 ? 1 : B) * (g.mask_c1 ? 1 : K) * chw), gy((long long)Hc * nb), gx((long long)Wc * nb);
    Buf<float> q(P * chw), qr(P * chw), dn(P * chw), dnr(P * chw), z(P * chw), zr(P * chw), rr(P * chw), rrr(P * chw), qo(P * chw);
    Buf<float> alpha(P), beta(P);
    Buf<double> slots(P * tiles), rho(P), sigma(P), sref(P), scale(P);
    Buf<int> ok(P);
    d.fill(); r.fill(); mask.binary(); alpha.fill(); beta.fill();
    gy.fill(); gx.fill();
    for (long long i = 0; i < gy.n; ++i) gy.p[i] = fabsf(gy.p[i]);
    for (long long i = 0; i < gx.n; ++i) gx.p[i] = fabsf(gx.p[i]);
    g.mask = mask_form == 3 ? nullptr : mask.p;
    g.gy = gy.p; g.gx = gx.p; g.slots = slots.p; g.rho = rho.p; g.alpha = alpha.p; g.beta = beta.p; g.ok = ok.p; g.sigma_out = sigma.p;
    const bool vecq = Wc % 4 == 0;
    // q = S d and <d, q>
    ref_gram(g, d.p, qr.p, sref.p, scale.p);
    for (int form = 0; form < 2; ++form) {
        if (form && !vecq) continue;
        q.nan(); slots.nan(); sigma.nan();
        g.d = d.p; g.r = nullptr; g.d_out = nullptr; g.q = q.p;
        if (form) run_gram<true, false>(g); else run_gram<false, false>(g);
        same("gram", q.p, qr.p, q.n, g, form);
        run_sum(0, g);
        for (long long pl = 0; pl < P; ++pl) close_to("sigma", sigma.p[pl], sref.p[pl], scale.p[pl], g, form);
    }
    // the same with d = r + beta d formed while the tile is staged
    for (long long i = 0; i < P * chw; ++i) {
        const float bd = beta.p[i / chw] * d.p[i];
        dnr.p[i] = r.p[i] + bd;
    }
    ref_gram(g, dnr.p, qr.p, sref.p, scale.p);
    for (int form = 0; form < 2; ++form) {
        if (form && !vecq) continue;
        q.nan(); dn.nan(); slots.nan(); sigma.nan();
        g.d = d.p; g.r = r.p; g.d_out = dn.p; g.q = q.p;
        if (form) run_gram<true, true>(g); else run_gram<false, true>(g);
        same("gram+d", q.p, qr.p, q.n, g, form);
        same("d_out", dn.p, dnr.p, dn.n, g, form);
        run_sum(0, g);
        for (long long pl = 0; pl < P; ++pl) close_to("sigma+d", sigma.p[pl], sref.p[pl], scale.p[pl], g, form);
    }
    // init, update, final
    for (int form = 0; form < 2; ++form) {
        if (form && !vecq) continue;
        z.nan(); rr.nan(); slots.nan();
        g.c = d.p; g.z = z.p; g.rr = rr.p;
        if (form) run_elem<true>(0, g); else run_elem<false>(0, g);
        run_sum(1, g);
        for (long long i = 0; i < P * chw; ++i) zr.p[i] = 0.0f;
        same("init z", z.p, zr.p, z.n, g, form);
        same("init r", rr.p, d.p, rr.n, g, form);
        for (long long pl = 0; pl < P; ++pl) {
            double s = 0.0;
            for (long long i = 0; i < chw; ++i) s += (double)d.p[pl * chw + i] * (double)d.p[pl * chw + i];
            close_to("rho", rho.p[pl], s, s, g, form);
        }
        // z += alpha d, r -= alpha q from a random state
        for (long long i = 0; i < P * chw; ++i) { z.p[i] = zr.p[i] = rnd(); rr.p[i] = rrr.p[i] = rnd(); }
        g.d = d.p; g.q = qr.p;
        for (long long i = 0; i < P * chw; ++i) {
            const float a = alpha.p[i / chw];
            const float ad = a * d.p[i];
            zr.p[i] = zr.p[i] + ad;
            const float aq = a * qr.p[i];
            rrr.p[i] = rrr.p[i] - aq;
        }
        slots.nan();
        if (form) run_elem<true>(1, g); else run_elem<false>(1, g);
        same("update z", z.p, zr.p, z.n, g, form);
        same("update r", rr.p, rrr.p, rr.n, g, form);
        for (long long pl = 0; pl < P; ++pl) ok.p[pl] = 1;
        for (long long pl = 0; pl < P; ++pl) rho.p[pl] = 2.0;
        run_sum(3, g);
        for (long long pl = 0; pl < P; ++pl) {
            double s = 0.0;
            for (long long i = 0; i < chw; ++i) s += (double)rrr.p[pl * chw + i] * (double)rrr.p[pl * chw + i];
            close_to("rho'", rho.p[pl], s, s, g, form);
            ++cases;
            if (beta.p[pl] != (float)(rho.p[pl] / 2.0)) { printf("MISMATCH beta\n"); ++failures; }
        }
        beta.fill();
        // alpha and its guard
        for (long long pl = 0; pl < P; ++pl) rho.p[pl] = pl == 1 ? 0.0 : 3.0;
        for (long long t = 0; t < P * tiles; ++t) slots.p[t] = (t / tiles == 2) ? -1.0 : 0.5;
        run_sum(2, g);
        for (long long pl = 0; pl < P; ++pl) {
            const float want = (pl == 1 || pl == 2) ? 0.0f : (float)(3.0 / (0.5 * (double)tiles));
            ++cases;
            if (alpha.p[pl] != want || ok.p[pl] != (want != 0.0f)) { printf("MISMATCH alpha plane %lld: %g vs %g\n", pl, (double)alpha.p[pl], (double)want); ++failures; }
        }
        alpha.fill();
        // q_out = lambda (m z)
        qo.nan();
        g.q_out = qo.p;
        if (form) run_elem<true>(2, g); else run_elem<false>(2, g);
        for (long long i = 0; i < P * chw; ++i) {
            const float* m = cg_mask_plane(g, i / chw);
            const float mz = m ? m[i % chw] * z.p[i] : z.p[i];
            q.p[i] = g.lambda * mz;
        }
        same("final", qo.p, q.p, qo.n, g, form);
    }
}

int main() {
    const int bs[3] = {0, 3, 24};
    const int dims[8][2] = {{1, 1}, {2, 3}, {4, 8}, {7, 14}, {3, 21}, {40, 40}, {33, 68}, {70, 75}};
    int n = 0;
    for (int bi = 0; bi < 3; ++bi)
        for (int d = 0; d < 8; ++d, ++n) one_case(bs[bi], dims[d][0], dims[d][1], n % 4, n % 2 ? 0.05f : 0.0f);
    if (failures) { printf("FAILED %d of %d\n", failures, cases); return 1; }
    printf("ok %d\n", cases);
    return 0;
}
