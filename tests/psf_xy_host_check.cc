// The per-axis phase bodies of the PSF kernels (psf_residual_xy_phase / psf_update_xy_phase of eo_diffusion_amd/csrc/psf_body.h; DESIGN.md
// section 9.11) compiled for the host and run tile by tile, phase by phase, thread number by thread number, against a whole-plane
// evaluation of the contract of include/eodiff.h written straight from its lines (padded planes, sequential adds, the update with the
// reversed taps and the forward n).  Meant to be built with -ffp-contract=off -fsanitize=address,undefined: every tensor is a heap buffer
// of exactly its size, so a read or write outside a plane, and a misaligned 16-byte access, ends the run.  The cases are the shape list of
// tests/test_gpu_psf_xy.py, each with three tap families (two different symmetric Gaussians; Gaussians shifted by +-0.37 f; the one-sided
// [0 .. .6 .4]), the plain and the mixed form, every access form the shape allows.  With a directory as its argument it also writes one
// file per case (inputs and the three outputs) for tests/test_psf_xy_host.py to compare with the torch emulation.  A last family is the
// fact any merge of the bodies rests on: with equal, bitwise symmetric taps (r = 12 on both axes) the one-vector bodies (psf_residual_phase
// / psf_update_phase and their _mix forms, which the bare and the _mix entry points run) give the bits of the per-axis bodies -- apply,
// residual and update, plain and mixed, every access form, at the list's two smallest planes (6 x 7, 12 x 28) and at its smallest plane
// that allows all four access forms (32 x 64 at f = 4).  Prints "ok <cases>" and returns 0 when every output is bit-equal.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
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
static void ref_norm(const float* h, int r, int L, std::vector<float>& n) {
    n.resize(L);
    for (int x = 0; x < L; ++x) {
        float acc = 0.0f;
        for (int i = 0; i <= 2 * r; ++i) {
            const int xi = x - r + i;
            const float pr = h[i] * ((xi >= 0 && xi < L) ? 1.0f : 0.0f);
            acc = i ? acc + pr : pr;
        }
        n[x] = acc;
    }
}

// conv_y(conv_x(u; hx, rx); hy, ry)
static void ref_blur(const float* hy, int ry, const float* hx, int rx, const float* u, int H, int W, std::vector<float>& out) {
    const int PH = H + 2 * ry, PW = W + 2 * rx;
    std::vector<float> pad((size_t)PH * PW, 0.0f), hz((size_t)PH * W);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) pad[(size_t)(y + ry) * PW + x + rx] = u[(size_t)y * W + x];
    for (int y = 0; y < PH; ++y)
        for (int x = 0; x < W; ++x) {
            float acc = hx[0] * pad[(size_t)y * PW + x];
            for (int i = 1; i <= 2 * rx; ++i) {
                const float pr = hx[i] * pad[(size_t)y * PW + x + i];
                acc = acc + pr;
            }
            hz[(size_t)y * W + x] = acc;
        }
    out.resize((size_t)H * W);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            float acc = hy[0] * hz[(size_t)y * W + x];
            for (int i = 1; i <= 2 * ry; ++i) {
                const float pr = hy[i] * hz[(size_t)(y + i) * W + x];
                acc = acc + pr;
            }
            out[(size_t)y * W + x] = acc;
        }
}

struct Case {
    int f, ry, rx, H, W, B, C, K, mixed, mask_form;
    int one;                           // equal symmetric taps: the one-vector bodies are run as well and must give the same bits
    std::vector<float> hy, hx, M, G;   // forward taps; R [K][C] and G [C][K] of the mixed form
};

static void ref_residual(const Case& cs, const PsfArgs& g, float* q) {
    const int f = g.f, Hc = g.H / f, Wc = g.W / f;
    const size_t hw = (size_t)g.H * g.W;
    std::vector<float> nh, nv, bl, u(hw);
    ref_norm(cs.hx.data(), cs.rx, g.W, nh);
    ref_norm(cs.hy.data(), cs.ry, g.H, nv);
    for (int b = 0; b < g.B; ++b)
        for (int k = 0; k < g.K; ++k) {
            const float* src = g.p + (size_t)b * g.C * hw;
            if (cs.mixed) {
                for (size_t i = 0; i < hw; ++i) {
                    float acc = cs.M[(size_t)k * g.C] * src[i];
                    for (int c = 1; c < g.C; ++c) {
                        const float pr = cs.M[(size_t)k * g.C + c] * src[(size_t)c * hw + i];
                        acc = acc + pr;
                    }
                    u[i] = acc;
                }
            } else {
                memcpy(u.data(), src + (size_t)g.ch[k] * hw, hw * sizeof(float));
            }
            ref_blur(cs.hy.data(), cs.ry, cs.hx.data(), cs.rx, u.data(), g.H, g.W, bl);
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

static void ref_update(const Case& cs, const PsfArgs& g, float* out) {
    const int f = g.f, Wc = g.W / f;
    const size_t hw = (size_t)g.H * g.W, chw = hw / (f * f);
    std::vector<float> nh, nv, w(hw), bl, s(chw);
    std::vector<float> hyr(cs.hy.rbegin(), cs.hy.rend()), hxr(cs.hx.rbegin(), cs.hx.rend());
    ref_norm(cs.hx.data(), cs.rx, g.W, nh);
    ref_norm(cs.hy.data(), cs.ry, g.H, nv);
    for (int b = 0; b < g.B; ++b)
        for (int c = 0; c < g.C; ++c) {
            const float* p = g.p + ((size_t)b * g.C + c) * hw;
            float* o = out + ((size_t)b * g.C + c) * hw;
            if (!cs.mixed && g.kof[c] < 0) { memcpy(o, p, hw * sizeof(float)); continue; }
            const float* qb = g.q + (size_t)b * g.K * chw;
            if (cs.mixed) {
                for (size_t i = 0; i < chw; ++i) {
                    float acc = cs.G[(size_t)c * g.K] * qb[i];
                    for (int k = 1; k < g.K; ++k) {
                        const float pr = cs.G[(size_t)c * g.K + k] * qb[(size_t)k * chw + i];
                        acc = acc + pr;
                    }
                    s[i] = acc;
                }
            } else {
                memcpy(s.data(), qb + (size_t)g.kof[c] * chw, chw * sizeof(float));
            }
            for (int y = 0; y < g.H; ++y)
                for (int x = 0; x < g.W; ++x) {
                    const float ts = s[(size_t)(y / f) * Wc + x / f] * g.step;
                    const float n = nv[y] * nh[x];
                    w[(size_t)y * g.W + x] = ts / n;
                }
            ref_blur(hyr.data(), cs.ry, hxr.data(), cs.rx, w.data(), g.H, g.W, bl);
            for (size_t i = 0; i < hw; ++i) o[i] = p[i] - bl[i];
        }
}

// ------------------------------------------------------------------------------------------------ the kernels' bodies, as the kernels run them
template <bool VEC, bool VECQ, bool MIX>
static void run_residual(const PsfArgs& g, const PsfTapsXy& tt, const PsfMix* mx) {
    PsfResLds* s = (PsfResLds*)malloc(sizeof(PsfResLds));
    const long long items = (long long)g.B * g.K * g.tiles_x * g.tiles_y;
    for (long long item = 0; item < items; ++item) {
        memset(s, 0xff, sizeof(*s));   // NaN: nothing may depend on what an earlier tile left behind
        for (int phase = 0; phase < 4; ++phase)
            for (int tid = 0; tid < PSF_THREADS; ++tid) psf_residual_xy_phase<VEC, VECQ, MIX>(phase, g, tt, mx, *s, item, tid);
    }
    free(s);
}
template <bool VEC, bool VECQ, bool MIX>
static void run_update(const PsfArgs& g, const PsfTapsXy& tt, const PsfMix* mx) {
    PsfUpdLds* s = (PsfUpdLds*)malloc(sizeof(PsfUpdLds));
    const long long items = (long long)g.B * g.C * g.tiles_x * g.tiles_y;
    for (long long item = 0; item < items; ++item) {
        memset(s, 0xff, sizeof(*s));
        for (int phase = 0; phase < 5; ++phase)
            for (int tid = 0; tid < PSF_THREADS; ++tid) psf_update_xy_phase<VEC, VECQ, MIX>(phase, g, tt, mx, *s, item, tid);
    }
    free(s);
}
// the one-vector bodies (g.r and t: the radius and the taps of both axes)
template <bool VEC, bool VECQ, bool MIX>
static void run_residual_one(const PsfArgs& g, const PsfTaps& t, const PsfMix* mx) {
    PsfResLds* s = (PsfResLds*)malloc(sizeof(PsfResLds));
    const long long items = (long long)g.B * g.K * g.tiles_x * g.tiles_y;
    for (long long item = 0; item < items; ++item) {
        memset(s, 0xff, sizeof(*s));
        for (int phase = 0; phase < 4; ++phase)
            for (int tid = 0; tid < PSF_THREADS; ++tid) {
                if (MIX) psf_residual_mix_phase<VEC, VECQ>(phase, g, t, *mx, *s, item, tid);
                else psf_residual_phase<VEC, VECQ>(phase, g, t, *s, item, tid);
            }
    }
    free(s);
}
template <bool VEC, bool VECQ, bool MIX>
static void run_update_one(const PsfArgs& g, const PsfTaps& t, const PsfMix* mx) {
    PsfUpdLds* s = (PsfUpdLds*)malloc(sizeof(PsfUpdLds));
    const long long items = (long long)g.B * g.C * g.tiles_x * g.tiles_y;
    for (long long item = 0; item < items; ++item) {
        memset(s, 0xff, sizeof(*s));
        for (int phase = 0; phase < 5; ++phase)
            for (int tid = 0; tid < PSF_THREADS; ++tid) {
                if (MIX) psf_update_mix_phase<VEC, VECQ>(phase, g, t, *mx, *s, item, tid);
                else psf_update_phase<VEC, VECQ>(phase, g, t, *s, item, tid);
            }
    }
    free(s);
}
template <bool MIX>
static void residual_one_form(int form, const PsfArgs& g, const PsfTaps& t, const PsfMix* mx) {
    if (form == 0) run_residual_one<false, false, MIX>(g, t, mx);
    else if (form == 1) run_residual_one<true, false, MIX>(g, t, mx);
    else if (form == 2) run_residual_one<false, true, MIX>(g, t, mx);
    else run_residual_one<true, true, MIX>(g, t, mx);
}
template <bool MIX>
static void update_one_form(int form, const PsfArgs& g, const PsfTaps& t, const PsfMix* mx) {
    if (form == 0) run_update_one<false, false, MIX>(g, t, mx);
    else if (form == 1) run_update_one<true, false, MIX>(g, t, mx);
    else if (form == 2) run_update_one<false, true, MIX>(g, t, mx);
    else run_update_one<true, true, MIX>(g, t, mx);
}

template <bool MIX>
static void residual_form(int form, const PsfArgs& g, const PsfTapsXy& tt, const PsfMix* mx) {
    if (form == 0) run_residual<false, false, MIX>(g, tt, mx);
    else if (form == 1) run_residual<true, false, MIX>(g, tt, mx);
    else if (form == 2) run_residual<false, true, MIX>(g, tt, mx);
    else run_residual<true, true, MIX>(g, tt, mx);
}
template <bool MIX>
static void update_form(int form, const PsfArgs& g, const PsfTapsXy& tt, const PsfMix* mx) {
    if (form == 0) run_update<false, false, MIX>(g, tt, mx);
    else if (form == 1) run_update<true, false, MIX>(g, tt, mx);
    else if (form == 2) run_update<false, true, MIX>(g, tt, mx);
    else run_update<true, true, MIX>(g, tt, mx);
}

static int failures = 0, cases = 0;
static void same(const char* what, const float* a, const float* b, long long n, const Case& c, int form) {
    ++cases;
    if (memcmp(a, b, (size_t)n * sizeof(float)) == 0) return;
    long long bad = 0, first = -1;
    for (long long i = 0; i < n; ++i)
        if (memcmp(a + i, b + i, sizeof(float))) { if (first < 0) first = i; ++bad; }
    printf("MISMATCH %s f=%d ry=%d rx=%d %dx%d mixed=%d form=%d: %lld of %lld differ, first at %lld (%g vs %g)\n", what, c.f, c.ry, c.rx, c.H, c.W,
           c.mixed, form, bad, n, first, (double)a[first], (double)b[first]);
    ++failures;
}

// the three tap families along one axis
static std::vector<float> taps_of(int family, int r, int f, double mtf, double shift) {
    std::vector<float> h(2 * r + 1, 0.0f);
    if (family == 2) {                                    // one-sided: [0 .. 0 .6 .4]
        if (r == 0) h[0] = 1.0f; else { h[r] = 0.6f; h[r + 1] = 0.4f; }
        return h;
    }
    const double sigma = f * sqrt(-2.0 * log(mtf)) / 3.14159265358979323846;
    std::vector<double> g(2 * r + 1);
    double sum = 0.0;
    for (int i = 0; i <= 2 * r; ++i) {
        const double k = i - r - (family == 1 ? shift : 0.0);
        g[i] = exp(-(k * k) / (2.0 * sigma * sigma));
        sum += g[i];
    }
    for (int i = 0; i <= 2 * r; ++i) h[i] = (float)(g[i] / sum);
    if (family == 0) for (int i = 0; i < r; ++i) h[2 * r - i] = h[i];
    return h;
}

static void put(FILE* fp, const void* p, size_t bytes) { if (fp && fwrite(p, 1, bytes, fp) != bytes) { printf("write failed\n"); exit(2); } }

static void one_case(Case cs, int family, const char* dir, int number) {
    const int B = cs.B, C = cs.C, K = cs.K, f = cs.f, H = cs.H, W = cs.W;
    cs.hy = taps_of(family, cs.ry, f, 0.3, 0.37 * f);
    cs.hx = cs.one ? cs.hy : taps_of(family, cs.rx, f, 0.5, -0.37 * f);
    PsfArgs g;
    memset(&g, 0, sizeof(g));
    PsfTapsXy fw, rv;
    memset(&fw, 0, sizeof(fw));
    memset(&rv, 0, sizeof(rv));
    fw.ry = rv.ry = cs.ry;
    fw.rx = rv.rx = cs.rx;
    for (int i = 0; i <= 2 * cs.ry; ++i) { fw.y.h[i] = cs.hy[i]; rv.y.h[i] = cs.hy[2 * cs.ry - i]; }
    for (int i = 0; i <= 2 * cs.rx; ++i) { fw.x.h[i] = cs.hx[i]; rv.x.h[i] = cs.hx[2 * cs.rx - i]; }
    g.r = cs.ry > cs.rx ? cs.ry : cs.rx; g.f = f; g.K = K; g.B = B; g.C = C; g.H = H; g.W = W;
    g.lambda = 0.75f; g.step = 0.9f;
    PsfMix mr, mg;
    memset(&mr, 0, sizeof(mr));
    memset(&mg, 0, sizeof(mg));
    if (cs.mixed) {
        cs.M.resize((size_t)K * C);
        cs.G.resize((size_t)C * K);
        for (auto& v : cs.M) v = rnd();
        for (auto& v : cs.G) v = rnd();
        for (int k = 0; k < K; ++k)
            for (int c = 0; c < C; ++c) { mr.m[k * PSF_MAXC + c] = cs.M[(size_t)k * C + c]; mg.m[c * PSF_MAXK + k] = cs.G[(size_t)c * K + k]; }
        for (int c = 0; c < PSF_MAXC; ++c) g.kof[c] = 0;
        for (int k = 0; k < K; ++k) g.ch[k] = (unsigned char)k;
    } else {
        for (int c = 0; c < PSF_MAXC; ++c) g.kof[c] = -1;
        g.ch[0] = 0; g.ch[1] = 2; g.kof[0] = 0; g.kof[2] = 1;
    }
    g.tc = psf_tile_coarse(f);
    const int ft = g.tc * f;
    g.tiles_x = (W + ft - 1) / ft;
    g.tiles_y = (H + ft - 1) / ft;
    const long long hw = (long long)H * W, chw = hw / (f * f);
    const int mask_form = cs.mixed ? (cs.mask_form == 0 ? 2 : cs.mask_form | 2) : cs.mask_form;   // mixed: one mask plane (2) or none (3)
    cs.mask_form = mask_form;
    g.values_b1 = mask_form == 1;
    g.mask_b1 = mask_form == 1 || mask_form == 2;
    g.mask_c1 = mask_form == 2 || cs.mixed;
    Buf p(B * C * hw), values((g.values_b1 ? 1 : B) * K * chw), mask((g.mask_b1 ? 1 : B) * (g.mask_c1 ? 1 : K) * chw);
    Buf q(B * K * chw), qr(B * K * chw), ar(B * K * chw), out(B * C * hw), outr(B * C * hw), q1(B * K * chw), out1(B * C * hw);
    p.fill(); values.fill(); mask.fill();
    g.p = p.p; g.values = values.p; g.mask = mask_form == 3 ? nullptr : mask.p;
    const bool vec = W % 4 == 0, vecq = (W / f) % 4 == 0;
    for (int apply = 0; apply < 2; ++apply) {
        PsfArgs a = g;
        if (apply) { a.values = nullptr; a.mask = nullptr; }
        float* want = apply ? ar.p : qr.p;
        ref_residual(cs, a, want);
        for (int form = 0; form < 4; ++form) {
            if (((form & 1) && !vec) || ((form & 2) && !vecq)) continue;
            q.nan();
            a.out = q.p;
            if (cs.mixed) residual_form<true>(form, a, fw, &mr);
            else residual_form<false>(form, a, fw, nullptr);
            same(apply ? "apply" : "residual", q.p, want, q.n, cs, form);
            if (!cs.one) continue;
            q1.nan();
            a.out = q1.p;
            if (cs.mixed) residual_one_form<true>(form, a, fw.x, &mr);
            else residual_one_form<false>(form, a, fw.x, nullptr);
            same(apply ? "apply, one vector against two" : "residual, one vector against two", q1.p, q.p, q.n, cs, form);
        }
    }
    g.q = qr.p;
    ref_update(cs, g, outr.p);
    for (int form = 0; form < 4; ++form) {
        if (((form & 1) && !vec) || ((form & 2) && !vecq)) continue;
        out.nan();
        g.out = out.p;
        if (cs.mixed) update_form<true>(form, g, rv, &mg);
        else update_form<false>(form, g, rv, nullptr);
        same("update", out.p, outr.p, out.n, cs, form);
        if (!cs.one) continue;
        out1.nan();
        g.out = out1.p;
        if (cs.mixed) update_one_form<true>(form, g, fw.x, &mg);       // (a symmetric array is its own reverse)
        else update_one_form<false>(form, g, fw.x, nullptr);
        same("update, one vector against two", out1.p, out.p, out.n, cs, form);
    }
    if (!dir) return;
    // int32 [f ry rx H W B C K mixed mask_form], then fp32: hy, hx, lambda, step, p, values, mask (unless mask_form 3), R and G (mixed), and
    // what the bodies gave in the last access form: apply, q, out
    const std::string path = std::string(dir) + "/case" + std::to_string(number) + ".bin";
    FILE* fp = fopen(path.c_str(), "wb");
    if (!fp) { printf("cannot write %s\n", path.c_str()); exit(2); }
    const int head[10] = {f, cs.ry, cs.rx, H, W, B, C, K, cs.mixed, mask_form};
    put(fp, head, sizeof(head));
    put(fp, cs.hy.data(), cs.hy.size() * 4);
    put(fp, cs.hx.data(), cs.hx.size() * 4);
    put(fp, &g.lambda, 4);
    put(fp, &g.step, 4);
    put(fp, p.p, p.n * 4);
    put(fp, values.p, values.n * 4);
    if (mask_form != 3) put(fp, mask.p, mask.n * 4);
    if (cs.mixed) { put(fp, cs.M.data(), cs.M.size() * 4); put(fp, cs.G.data(), cs.G.size() * 4); }
    {   // the dumped outputs come from the bodies, not from the whole-plane evaluation above
        PsfArgs a = g;
        a.values = nullptr; a.mask = nullptr; a.out = q.p;
        q.nan();
        if (cs.mixed) residual_form<true>(0, a, fw, &mr); else residual_form<false>(0, a, fw, nullptr);
        put(fp, q.p, q.n * 4);
        a = g; a.out = q.p;
        q.nan();
        if (cs.mixed) residual_form<true>(0, a, fw, &mr); else residual_form<false>(0, a, fw, nullptr);
        put(fp, q.p, q.n * 4);
        put(fp, out.p, out.n * 4);
    }
    fclose(fp);
}

int main(int argc, char** argv) {
    const char* dir = argc > 1 ? argv[1] : nullptr;
    const int shapes[8][5] = {{1, 0, 12, 6, 7}, {1, 12, 0, 40, 72}, {2, 3, 7, 12, 28}, {3, 5, 2, 48, 30},
                              {4, 1, 12, 32, 64}, {5, 7, 4, 35, 70}, {6, 12, 9, 24, 30}, {8, 12, 3, 24, 168}};
    int number = 0;
    for (int s = 0; s < 8; ++s)
        for (int family = 0; family < 3; ++family)
            for (int mixed = 0; mixed < 2; ++mixed) {
                Case cs;
                cs.f = shapes[s][0]; cs.ry = shapes[s][1]; cs.rx = shapes[s][2]; cs.H = shapes[s][3]; cs.W = shapes[s][4];
                cs.B = 2; cs.C = 3; cs.K = 2; cs.mixed = mixed; cs.mask_form = (s + family) % 4; cs.one = 0;
                one_case(cs, family, dir, number++);
            }
    const int equal[3][3] = {{1, 6, 7}, {2, 12, 28}, {4, 32, 64}};       // f, H, W: the one-vector bodies against the per-axis ones (nothing is dumped)
    for (int s = 0; s < 3; ++s)
        for (int mixed = 0; mixed < 2; ++mixed) {
            Case cs;
            cs.f = equal[s][0]; cs.ry = cs.rx = PSF_MAXR; cs.H = equal[s][1]; cs.W = equal[s][2];
            cs.B = 2; cs.C = 3; cs.K = 2; cs.mixed = mixed; cs.mask_form = s; cs.one = 1;
            one_case(cs, 0, nullptr, 0);
        }
    if (failures) { printf("FAILED %d of %d\n", failures, cases); return 1; }
    printf("ok %d\n", cases);
    return 0;
}
