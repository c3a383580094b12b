// The bodies of the two PSF kernels (eo_diffusion_amd/csrc/psf_body.h) compiled for the host and run tile by tile, phase by phase, thread
// number by thread number, against a whole-plane evaluation of the contract of include/eodiff.h written straight from its lines (padded
// planes, sequential adds).  Meant to be built with -ffp-contract=off -fsanitize=address,undefined: every tensor is a heap buffer of exactly
// its size, so a read or write outside a plane, and a misaligned 16-byte access, ends the run.  Every f, r in {0, 1, 12}, both access forms
// of both grids, planes smaller than the halo, several tiles with a ragged edge.  Prints "ok <cases>" and returns 0 when every output is
// bit-equal.  tests/test_psf_host.py builds and runs it.
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

static void ref_residual(const PsfArgs& g, const PsfTaps& t, float* q) {
    const int f = g.f, Hc = g.H / f, Wc = g.W / f;
    std::vector<float> nh, nv, bl;
    ref_norm(t, g.r, g.W, nh);
    ref_norm(t, g.r, g.H, nv);
    for (int b = 0; b < g.B; ++b)
        for (int k = 0; k < g.K; ++k) {
            ref_blur(t, g.r, g.p + ((size_t)b * g.C + g.ch[k]) * g.H * g.W, g.H, g.W, bl);
            for (size_t i = 0; i < bl.size(); ++i) {
                const float n = nv[i / g.W] * nh[i % g.W];
                bl[i] = bl[i] / n;
            }
            for (int cy = 0; cy < Hc; ++cy)
                for (int cx = 0; cx < Wc; ++cx) {
                    float s = bl[(size_t)cy * f * g.W + cx * f];
                    for (int i = 1; i < f * f; ++i) s = s + bl[(size_t)(cy * f + i / f) * g.W + cx * f + i % f];
                    const float mean = s / (float)(f * f);
                    const size_t at = (size_t)cy * Wc + cx, pl = (size_t)Hc * Wc;
                    float o = mean;
                    if (g.values) {
                        const float m = g.mask ? g.mask[((size_t)(g.mask_b1 ? 0 : b) * (g.mask_c1 ? 1 : g.K) + (g.mask_c1 ? 0 : k)) * pl + at] : 1.0f;
                        const float v = g.values[((size_t)(g.values_b1 ? 0 : b) * g.K + k) * pl + at];
                        const float lm = g.lambda * m;
                        const float df = mean - v;
                        o = lm * df;
                    }
                    q[((size_t)b * g.K + k) * pl + at] = o;
                }
        }
}

static void ref_update(const PsfArgs& g, const PsfTaps& t, float* out) {
    const int f = g.f, Wc = g.W / f;
    const size_t hw = (size_t)g.H * g.W;
    std::vector<float> nh, nv, w(hw), bl;
    ref_norm(t, g.r, g.W, nh);
    ref_norm(t, g.r, g.H, nv);
    for (int b = 0; b < g.B; ++b)
        for (int c = 0; c < g.C; ++c) {
            const float* p = g.p + ((size_t)b * g.C + c) * hw;
            float* o = out + ((size_t)b * g.C + c) * hw;
            if (g.kof[c] < 0) { memcpy(o, p, hw * sizeof(float)); continue; }
            const float* q = g.q + ((size_t)b * g.K + g.kof[c]) * (hw / (f * f));
            for (int y = 0; y < g.H; ++y)
                for (int x = 0; x < g.W; ++x) {
                    const float ts = q[(size_t)(y / f) * Wc + x / f] * g.step;
                    const float n = nv[y] * nh[x];
                    w[(size_t)y * g.W + x] = ts / n;
                }
            ref_blur(t, g.r, w.data(), g.H, g.W, bl);
            for (size_t i = 0; i < hw; ++i) o[i] = p[i] - bl[i];
        }
}

// ------------------------------------------------------------------------------------------------ the kernels' bodies, as the kernels run them
template <bool VEC, bool VECQ>
static void run_residual(const PsfArgs& g, const PsfTaps& t) {
    PsfResLds* s = (PsfResLds*)malloc(sizeof(PsfResLds));
    const long long items = (long long)g.B * g.K * g.tiles_x * g.tiles_y;
    for (long long item = 0; item < items; ++item) {
        memset(s, 0xff, sizeof(*s));   // NaN: nothing may depend on what an earlier tile left behind
        for (int phase = 0; phase < 4; ++phase)
            for (int tid = 0; tid < PSF_THREADS; ++tid) psf_residual_phase<VEC, VECQ>(phase, g, t, *s, item, tid);
    }
    free(s);
}
template <bool VEC, bool VECQ>
static void run_update(const PsfArgs& g, const PsfTaps& t) {
    PsfUpdLds* s = (PsfUpdLds*)malloc(sizeof(PsfUpdLds));
    const long long items = (long long)g.B * g.C * g.tiles_x * g.tiles_y;
    for (long long item = 0; item < items; ++item) {
        memset(s, 0xff, sizeof(*s));
        for (int phase = 0; phase < 5; ++phase)
            for (int tid = 0; tid < PSF_THREADS; ++tid) psf_update_phase<VEC, VECQ>(phase, g, t, *s, item, tid);
    }
    free(s);
}

static int failures = 0, cases = 0;
static void same(const char* what, const float* a, const float* b, long long n, const PsfArgs& g, int form) {
    ++cases;
    if (memcmp(a, b, (size_t)n * sizeof(float)) == 0) return;
    long long bad = 0, first = -1;
    for (long long i = 0; i < n; ++i)
        if (memcmp(a + i, b + i, sizeof(float))) { if (first < 0) first = i; ++bad; }
    printf("MISMATCH %s f=%d r=%d %dx%d form=%d: %lld of %lld differ, first at %lld (%g vs %g)\n", what, g.f, g.r, g.H, g.W, form, bad, n, first,
           (double)a[first], (double)b[first]);
    ++failures;
}

static void one_case(int f, int r, int H, int W, int mask_form) {
    const int B = 2, C = 3, K = 2;
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
    for (int c = 0; c < PSF_MAXC; ++c) g.kof[c] = -1;
    g.ch[0] = 0; g.ch[1] = 2; g.kof[0] = 0; g.kof[2] = 1;
    g.tc = psf_tile_coarse(f);
    const int ft = g.tc * f;
    g.tiles_x = (W + ft - 1) / ft;
    g.tiles_y = (H + ft - 1) / ft;
    const long long hw = (long long)H * W, chw = hw / (f * f);
    g.values_b1 = mask_form == 1;
    g.mask_b1 = mask_form == 1 || mask_form == 2;
    g.mask_c1 = mask_form == 2;
    Buf p(B * C * hw), values((g.values_b1 ? 1 : B) * K * chw), mask((g.mask_b1 ? 1 : B) * (g.mask_c1 ? 1 : K) * chw), q(B * K * chw), qr(B * K * chw);
    Buf out(B * C * hw), outr(B * C * hw);
    p.fill(); values.fill(); mask.fill();
    g.p = p.p; g.values = values.p; g.mask = mask_form == 3 ? nullptr : mask.p;
    const bool vec = W % 4 == 0, vecq = (W / f) % 4 == 0;
    for (int apply = 0; apply < 2; ++apply) {
        PsfArgs a = g;
        if (apply) { a.values = nullptr; a.mask = nullptr; }
        ref_residual(a, t, qr.p);
        for (int form = 0; form < 4; ++form) {
            if (((form & 1) && !vec) || ((form & 2) && !vecq)) continue;
            q.nan();
            a.out = q.p;
            if (form == 0) run_residual<false, false>(a, t);
            else if (form == 1) run_residual<true, false>(a, t);
            else if (form == 2) run_residual<false, true>(a, t);
            else run_residual<true, true>(a, t);
            same(apply ? "apply" : "residual", q.p, qr.p, q.n, a, form);
        }
    }
    ref_residual(g, t, qr.p);
    g.q = qr.p;
    ref_update(g, t, outr.p);
    for (int form = 0; form < 4; ++form) {
        if (((form & 1) && !vec) || ((form & 2) && !vecq)) continue;
        out.nan();
        g.out = out.p;
        if (form == 0) run_update<false, false>(g, t);
        else if (form == 1) run_update<true, false>(g, t);
        else if (form == 2) run_update<false, true>(g, t);
        else run_update<true, true>(g, t);
        same("update", out.p, outr.p, out.n, g, form);
    }
}

int main() {
    const int rs[3] = {0, 1, 12};
    for (int f = 1; f <= 8; ++f) {
        const int ft = psf_tile_coarse(f) * f;
        const int dims[5][2] = {{f, f}, {3 * f, 5 * f}, {4 * f, 4 * f}, {ft + f, 2 * ft + 4 * f}, {2 * ft + 3 * f, ft + 8 * f}};
        for (int ri = 0; ri < 3; ++ri)
            for (int d = 0; d < 5; ++d) one_case(f, rs[ri], dims[d][0], dims[d][1], (f + ri + d) % 4);
    }
    if (failures) { printf("FAILED %d of %d\n", failures, cases); return 1; }
    printf("ok %d\n", cases);
    return 0;
}
