// The bodies of the two mixed PSF kernels (eo_diffusion_amd/csrc/psf_body.h: psf_residual_mix_phase, psf_update_mix_phase) compiled for the
// host and run tile by tile, phase by phase, thread number by thread number, against a whole-plane evaluation of the contract of
// include/eodiff.h written straight from its lines.  Meant to be built with -ffp-contract=off
// -fsanitize=address,undefined: every tensor is a heap buffer of exactly its size, so a read or write outside a plane, and a misaligned
// 16-byte access, ends the run.  Planes from one coarse pixel to several ragged tiles, (C, K) from (1, 1) to (32, 8), every access form,
// mask absent / full / broadcast, the operator alone.  Prints "ok <cases>" and returns 0 when every output is bit-equal.
// tests/test_spectral_psf_host.py builds and runs it.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../eo_diffusion_amd/csrc/psf_body.h"

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static float rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (float)((rng_state >> 40) & 0xFFFFFF) / 8388608.0f - 1.0f;
}

struct Buf {   // an exactly sized heap buffer
    float* p;
    long long n;
    explicit Buf(long long n_) : p((float*)malloc((size_t)n_ * sizeof(float))), n(n_) {}
    ~Buf() { free(p); }
    Buf(const Buf&) = delete;
    void fill() { for (long long i = 0; i < n; ++i) p[i] = rnd(); }
    void nan() { for (long long i = 0; i < n; ++i) p[i] = NAN; }
};

// ------------------------------------------------------------------------------------------------ the contract, whole planes
static void ref_norm(const PsfTaps& t, int r, int L, std::vector<float>& n) {
    n.resize(L);
    for (int x = 0; x < L; ++x) {
        float acc = 0.0f;
        for (int i = 0; i <= 2 * r; ++i) {
            const int xi = x - r + i;
            const float pr = t.h[i] * ((xi >= 0 && xi < L) ? 1.0f : 0.0f);
            acc = i ? acc + pr : pr;
        }
        n[x] = acc;
    }
}

static void ref_blur(const PsfTaps& t, int r, const float* u, int H, int W, std::vector<float>& out) {
    const int PH = H + 2 * r, PW = W + 2 * r;
    std::vector<float> pad((size_t)PH * PW, 0.0f), hz((size_t)PH * W);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) pad[(size_t)(y + r) * PW + x + r] = u[(size_t)y * W + x];
    for (int y = 0; y < PH; ++y)
        for (int x = 0; x < W; ++x) {
            float acc = t.h[0] * pad[(size_t)y * PW + x];
            for (int i = 1; i <= 2 * r; ++i) {
                const float pr = t.h[i] * pad[(size_t)y * PW + x + i];
                acc = acc + pr;
            }
            hz[(size_t)y * W + x] = acc;
        }
    out.resize((size_t)H * W);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            float acc = t.h[0] * hz[(size_t)y * W + x];
            for (int i = 1; i <= 2 * r; ++i) {
                const float pr = t.h[i] * hz[(size_t)(y + i) * W + x];
                acc = acc + pr;
            }
            out[(size_t)y * W + x] = acc;
        }
}

// R [K][C] dense
static void ref_residual(const PsfArgs& g, const PsfTaps& t, const std::vector<float>& R, float* q) {
    const int f = g.f, Hc = g.H / f, Wc = g.W / f;
    const size_t hw = (size_t)g.H * g.W, pl = (size_t)Hc * Wc;
    std::vector<float> nh, nv, bl, u(hw);
    ref_norm(t, g.r, g.W, nh);
    ref_norm(t, g.r, g.H, nv);
    for (int b = 0; b < g.B; ++b)
        for (int k = 0; k < g.K; ++k) {
            const float* p = g.p + (size_t)b * g.C * hw;
            for (size_t i = 0; i < hw; ++i) {
                float acc = R[(size_t)k * g.C] * p[i];
                for (int c = 1; c < g.C; ++c) {
                    const float pr = R[(size_t)k * g.C + c] * p[(size_t)c * hw + i];
                    acc = acc + pr;
                }
                u[i] = acc;
            }
            ref_blur(t, g.r, u.data(), g.H, g.W, bl);
            for (size_t i = 0; i < hw; ++i) {
                const float n = nv[i / g.W] * nh[i % g.W];
                bl[i] = bl[i] / n;
            }
            for (int cy = 0; cy < Hc; ++cy)
                for (int cx = 0; cx < Wc; ++cx) {
                    float s = bl[(size_t)cy * f * g.W + cx * f];
                    for (int i = 1; i < f * f; ++i) s = s + bl[(size_t)(cy * f + i / f) * g.W + cx * f + i % f];
                    const float mean = s / (float)(f * f);
                    const size_t at = (size_t)cy * Wc + cx;
                    float o = mean;
                    if (g.values) {
                        const float m = g.mask ? g.mask[(size_t)(g.mask_b1 ? 0 : b) * pl + at] : 1.0f;
                        const float v = g.values[((size_t)(g.values_b1 ? 0 : b) * g.K + k) * pl + at];
                        const float lm = g.lambda * m;
                        const float df = mean - v;
                        o = lm * df;
                    }
                    q[((size_t)b * g.K + k) * pl + at] = o;
                }
        }
}

// G [C][K] dense
static void ref_update(const PsfArgs& g, const PsfTaps& t, const std::vector<float>& G, float* out) {
    const int f = g.f, Wc = g.W / f;
    const size_t hw = (size_t)g.H * g.W, pl = hw / (f * f);
    std::vector<float> nh, nv, w(hw), bl, s(pl);
    ref_norm(t, g.r, g.W, nh);
    ref_norm(t, g.r, g.H, nv);
    for (int b = 0; b < g.B; ++b)
        for (int c = 0; c < g.C; ++c) {
            const float* p = g.p + ((size_t)b * g.C + c) * hw;
            float* o = out + ((size_t)b * g.C + c) * hw;
            const float* q = g.q + (size_t)b * g.K * pl;
            for (size_t i = 0; i < pl; ++i) {
                float acc = G[(size_t)c * g.K] * q[i];
                for (int k = 1; k < g.K; ++k) {
                    const float pr = G[(size_t)c * g.K + k] * q[(size_t)k * pl + i];
                    acc = acc + pr;
                }
                s[i] = acc;
            }
            for (int y = 0; y < g.H; ++y)
                for (int x = 0; x < g.W; ++x) {
                    const float ts = s[(size_t)(y / f) * Wc + x / f] * g.step;
                    const float n = nv[y] * nh[x];
                    w[(size_t)y * g.W + x] = ts / n;
                }
            ref_blur(t, g.r, w.data(), g.H, g.W, bl);
            for (size_t i = 0; i < hw; ++i) o[i] = p[i] - bl[i];
        }
}

// ------------------------------------------------------------------------------------------------ the kernels' bodies, as the kernels run them
template <bool VEC, bool VECQ>
static void run_residual(const PsfArgs& g, const PsfTaps& t, const PsfMix& mx) {
    PsfResLds* s = (PsfResLds*)malloc(sizeof(PsfResLds));
    const long long items = (long long)g.B * g.K * g.tiles_x * g.tiles_y;
    for (long long item = 0; item < items; ++item) {
        memset(s, 0xff, sizeof(*s));   // NaN: nothing may depend on what an earlier tile left behind
        for (int phase = 0; phase < 4; ++phase)
            for (int tid = 0; tid < PSF_THREADS; ++tid) psf_residual_mix_phase<VEC, VECQ>(phase, g, t, mx, *s, item, tid);
    }
    free(s);
}
template <bool VEC, bool VECQ>
static void run_update(const PsfArgs& g, const PsfTaps& t, const PsfMix& mx) {
    PsfUpdLds* s = (PsfUpdLds*)malloc(sizeof(PsfUpdLds));
    const long long items = (long long)g.B * g.C * g.tiles_x * g.tiles_y;
    for (long long item = 0; item < items; ++item) {
        memset(s, 0xff, sizeof(*s));
        for (int phase = 0; phase < 5; ++phase)
            for (int tid = 0; tid < PSF_THREADS; ++tid) psf_update_mix_phase<VEC, VECQ>(phase, g, t, mx, *s, item, tid);
    }
    free(s);
}

static int failures = 0, cases = 0;
static void same(const char* what, const float* a, const float* b, long long n, const PsfArgs& g, int form, int mask_form) {
    ++cases;
    if (memcmp(a, b, (size_t)n * sizeof(float)) == 0) return;
    long long bad = 0, first = -1;
    for (long long i = 0; i < n; ++i)
        if (memcmp(a + i, b + i, sizeof(float))) { if (first < 0) first = i; ++bad; }
    printf("MISMATCH %s f=%d r=%d C=%d K=%d %dx%d form=%d mask=%d: %lld of %lld differ, first at %lld (%g vs %g)\n", what, g.f, g.r, g.C, g.K, g.H,
           g.W, form, mask_form, bad, n, first, (double)a[first], (double)b[first]);
    ++failures;
}

static void one_case(int f, int r, int H, int W, int C, int K) {
    const int B = 2;
    PsfArgs g;
    memset(&g, 0, sizeof(g));
    PsfTaps t;
    memset(&t, 0, sizeof(t));
    double sum = 0.0;
    for (int i = 0; i <= r; ++i) { t.h[i] = t.h[2 * r - i] = (float)exp(-0.5 * (i - r) * (i - r) / (0.3 * r * r + 0.5)); }
    for (int i = 0; i <= 2 * r; ++i) sum += t.h[i];
    for (int i = 0; i <= r; ++i) t.h[i] = t.h[2 * r - i] = (float)(t.h[i] / sum);
    g.r = r; g.f = f; g.K = K; g.B = B; g.C = C; g.H = H; g.W = W;
    g.lambda = 0.75f; g.step = 0.9f;
    g.mask_c1 = 1;                                            // one mask for all K bands
    for (int c = 0; c < PSF_MAXC; ++c) g.kof[c] = 0;          // as psf_common_mix leaves them
    for (int k = 0; k < PSF_MAXC; ++k) g.ch[k] = (unsigned char)(k < K ? k : 0);
    g.tc = psf_tile_coarse(f);
    const int ft = g.tc * f;
    g.tiles_x = (W + ft - 1) / ft;
    g.tiles_y = (H + ft - 1) / ft;
    const long long hw = (long long)H * W, chw = hw / (f * f);
    std::vector<float> R((size_t)K * C), G((size_t)C * K);
    for (float& v : R) v = rnd();
    for (float& v : G) v = rnd();
    R[(size_t)(K - 1) * C + C / 2] = 0.0f;                    // a zero entry: its product is formed like any other
    if (C > 1) for (int k = 0; k < K; ++k) G[(size_t)(C - 1) * K + k] = 0.0f;   // a zero row of G: out_c = p_c - blur(0)
    PsfMix mr, mg;
    memset(&mr, 0, sizeof(mr));
    memset(&mg, 0, sizeof(mg));
    for (int k = 0; k < K; ++k)
        for (int c = 0; c < C; ++c) { mr.m[k * PSF_MAXC + c] = R[(size_t)k * C + c]; mg.m[c * PSF_MAXK + k] = G[(size_t)c * K + k]; }
    Buf p(B * C * hw), q(B * K * chw), qr(B * K * chw), out(B * C * hw), outr(B * C * hw);
    p.fill();
    g.p = p.p;
    const bool vec = W % 4 == 0, vecq = (W / f) % 4 == 0;
    for (int mask_form = 0; mask_form < 4; ++mask_form) {     // 0: full, 1: values and mask broadcast, 2: no mask, 3: the operator alone
        PsfArgs a = g;
        a.values_b1 = mask_form == 1;
        a.mask_b1 = mask_form == 1;
        Buf values((a.values_b1 ? 1 : B) * K * chw), mask((a.mask_b1 ? 1 : B) * chw);
        values.fill(); mask.fill();
        a.values = mask_form == 3 ? nullptr : values.p;
        a.mask = mask_form >= 2 ? nullptr : mask.p;
        ref_residual(a, t, R, qr.p);
        for (int form = 0; form < 4; ++form) {
            if (((form & 1) && !vec) || ((form & 2) && !vecq)) continue;
            q.nan();
            a.out = q.p;
            if (form == 0) run_residual<false, false>(a, t, mr);
            else if (form == 1) run_residual<true, false>(a, t, mr);
            else if (form == 2) run_residual<false, true>(a, t, mr);
            else run_residual<true, true>(a, t, mr);
            same(mask_form == 3 ? "apply_mix" : "residual_mix", q.p, qr.p, q.n, a, form, mask_form);
        }
    }
    g.q = qr.p;                                               // (the operator's output: any finite coarse tensor will do)
    ref_update(g, t, G, outr.p);
    if (C > 1 && memcmp(outr.p + (C - 1) * hw, p.p + (C - 1) * hw, (size_t)hw * sizeof(float))) {
        printf("MISMATCH a zero row of G does not return p_c (f=%d r=%d C=%d K=%d)\n", f, r, C, K);
        ++failures;
    }
    for (int form = 0; form < 4; ++form) {
        if (((form & 1) && !vec) || ((form & 2) && !vecq)) continue;
        out.nan();
        g.out = out.p;
        if (form == 0) run_update<false, false>(g, t, mg);
        else if (form == 1) run_update<true, false>(g, t, mg);
        else if (form == 2) run_update<false, true>(g, t, mg);
        else run_update<true, true>(g, t, mg);
        same("update_mix", out.p, outr.p, out.n, g, form, -1);
    }
}

int main() {
    const int planes[5][4] = {{6, 9, 6, 6}, {3, 5, 12, 18}, {5, 7, 35, 70}, {1, 12, 40, 40}, {2, 3, 140, 148}};   // f, r, H, W
    const int ck[4][2] = {{1, 1}, {4, 1}, {13, 2}, {32, 8}};
    for (int d = 0; d < 5; ++d)
        for (int m = 0; m < 4; ++m) one_case(planes[d][0], planes[d][1], planes[d][2], planes[d][3], ck[m][0], ck[m][1]);
    if (failures) { printf("FAILED %d of %d\n", failures, cases); return 1; }
    printf("ok %d\n", cases);
    return 0;
}
