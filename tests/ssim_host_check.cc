// Host walk of csrc/ssim_body.h (tests/test_metrics_host.py builds this with -fsanitize=address,undefined and runs it as a child process): the
// tile phases of eod_ssim, thread number by thread number with a barrier's worth of separation between the phases, on exactly sized heap
// buffers, against a plain double loop over the whole plane written from the lines of include/eodiff.h.  The map must agree bit for bit, n
// exactly, and the sum within the reordering bound n * 2^-53 * sum |ssim|.  Prints "ok <cases>" and exits 0, or the mismatches and 1.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../eo_diffusion_amd/csrc/ssim_body.h"

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static float rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (float)((rng_state >> 40) & 0xFFFFFF) / 16777216.0f;
}

template <typename T> struct Buf {  // an exactly sized heap buffer: one element past either end is the sanitizer's
    T* p;
    size_t n;
    explicit Buf(size_t n_) : p((T*)malloc(n_ * sizeof(T) ? n_ * sizeof(T) : 1)), n(n_) {}
    ~Buf() { free(p); }
    Buf(const Buf&) = delete;
};

static int failures = 0, cases = 0;

// the contract, position by position
static double ref_value(const SsimArgs& g, const SsimTaps& k, const float* pred, const float* ref, int y, int x) {
    const int L = 2 * g.r + 1;
    double E[5];
    for (int q = 0; q < 5; ++q) {
        double v = 0.0;
        for (int u = 0; u < L; ++u) {
            double h = 0.0;
            for (int j = 0; j < L; ++j) {
                const long long o = (long long)(y + u) * g.W + (x + j);
                const double mp = g.a * (double)pred[o], mt = g.a * (double)ref[o];
                const double p = mp + g.b, t = mt + g.b;
                const double val = q == 0 ? p : q == 1 ? t : q == 2 ? p * p : q == 3 ? t * t : p * t;
                const double m = k.g[j] * val;
                h = j == 0 ? m : h + m;
            }
            const double m = k.g[u] * h;
            v = u == 0 ? m : v + m;
        }
        E[q] = v;
    }
    const double mpp = E[0] * E[0], mtt = E[1] * E[1], mpt = E[0] * E[1];
    const double spp = E[2] - mpp, stt = E[3] - mtt, spt = E[4] - mpt;
    return (((2.0 * mpt) + g.c1) * ((2.0 * spt) + g.c2)) / (((mpp + mtt) + g.c1) * ((spp + stt) + g.c2));
}

// B = 2 members of C = 2 bands, ref and where with one member: every plane offset is in play
static void one_case(int r, int H, int W, int where_form, bool with_map, double a, double b) {
    ++cases;
    const int B = 2, C = 2;
    const long long HW = (long long)H * W;
    Buf<float> pred(B * C * HW), ref(C * HW), where(HW), map(B * C * HW);
    for (size_t i = 0; i < pred.n; ++i) pred.p[i] = 0.9f + 1e-3f * rnd();
    for (size_t i = 0; i < ref.n; ++i) ref.p[i] = 0.9f + 1e-3f * rnd();
    for (size_t i = 0; i < where.n; ++i) where.p[i] = where_form == 1 ? 1.0f : (rnd() < 0.5f ? 0.0f : 2.0f);
    for (size_t i = 0; i < map.n; ++i) map.p[i] = -7.0f;
    SsimTaps k;
    double tot = 0.0;
    for (int i = 0; i < 2 * r + 1; ++i) { k.g[i] = exp(-0.5 * (i - r) * (i - r) / 2.25); tot += k.g[i]; }
    for (int i = 0; i < 2 * SSIM_MAXR + 1; ++i) k.g[i] = i < 2 * r + 1 ? k.g[i] / tot : 0.0;
    SsimArgs g;
    g.pred = pred.p; g.ref = ref.p; g.where = where_form ? where.p : nullptr; g.map = with_map ? map.p : nullptr;
    g.B = B; g.C = C; g.H = H; g.W = W; g.r = r; g.ref_B = 1; g.where_B = 1;
    g.tiles_x = (W - 2 * r + SSIM_TILE - 1) / SSIM_TILE;
    g.tiles_y = (H - 2 * r + SSIM_TILE - 1) / SSIM_TILE;
    g.a = a; g.b = b; g.c1 = 1e-4; g.c2 = 9e-4;
    const long long tiles = (long long)g.tiles_x * g.tiles_y;
    Buf<double> part(B * C * tiles * 2);
    g.part = part.p;
    const int E = SSIM_TILE + 2 * r;
    Buf<double> P(E * E), T(E * E), hb(E * SSIM_TILE), m(SSIM_THREADS * 5 * SSIM_PER);  // sized as the launch sizes the LDS
    for (long long bc = 0; bc < B * C; ++bc) {
        const long long c = bc % C;
        for (long long tile = 0; tile < tiles; ++tile) {
            const int ty = (int)(tile / g.tiles_x), tx = (int)(tile % g.tiles_x), y0 = ty * SSIM_TILE, x0 = tx * SSIM_TILE;
            for (size_t i = 0; i < P.n; ++i) P.p[i] = T.p[i] = NAN;  // (what a phase does not write must not be read)
            for (size_t i = 0; i < hb.n; ++i) hb.p[i] = NAN;
            for (int t = 0; t < SSIM_THREADS; ++t) ssim_load(g, t, bc * HW, c * HW, y0, x0, P.p, T.p);
            for (int q = 0; q < 5; ++q) {
                for (int t = 0; t < SSIM_THREADS; ++t) ssim_hpass(g, k, q, t, P.p, T.p, hb.p);
                for (int t = 0; t < SSIM_THREADS; ++t) ssim_vpass(g, k, t, hb.p, m.p + (t * 5 + q) * SSIM_PER);
            }
            double s = 0.0, n = 0.0;
            for (int t = 0; t < SSIM_THREADS; ++t) {
                double ts, tn;
                ssim_finish(g, t, bc * HW, 0, y0, x0, m.p + t * 5 * SSIM_PER, &ts, &tn);
                s += ts;
                n += tn;
            }
            part.p[(bc * tiles + tile) * 2] = s;
            part.p[(bc * tiles + tile) * 2 + 1] = n;
        }
    }
    for (long long bc = 0; bc < B * C; ++bc) {
        const long long c = bc % C;
        double s = 0.0, n = 0.0, want = 0.0, wn = 0.0, mag = 0.0;
        for (long long tile = 0; tile < tiles; ++tile) { s += part.p[(bc * tiles + tile) * 2]; n += part.p[(bc * tiles + tile) * 2 + 1]; }
        for (int y = 0; y < H; ++y) {
            for (int x = 0; x < W; ++x) {
                const long long o = bc * HW + (long long)y * W + x;
                const bool valid = y >= r && y < H - r && x >= r && x < W - r;
                if (!valid) {
                    if (with_map && map.p[o] != -7.0f) { ++failures; printf("r %d %dx%d: map written outside the valid region at (%d, %d)\n", r, H, W, y, x); }
                    continue;
                }
                const double v = ref_value(g, k, pred.p + bc * HW, ref.p + c * HW, y - r, x - r);
                const float f = (float)v;
                if (with_map && memcmp(&f, &map.p[o], 4) != 0) {
                    if (++failures < 20) printf("r %d %dx%d plane %lld: map (%d, %d) = %.9g, expected %.9g\n", r, H, W, bc, y, x, (double)map.p[o], (double)f);
                }
                if (!where_form || where.p[(long long)y * W + x] != 0.0f) { want += v; wn += 1.0; mag += fabs(v); }
            }
        }
        if (n != wn || !(fabs(s - want) <= wn * ldexp(1.0, -53) * mag)) {
            ++failures;
            printf("r %d %dx%d plane %lld: sum %.17g n %.0f, expected %.17g n %.0f\n", r, H, W, bc, s, n, want, wn);
        }
    }
}

int main() {
    // valid-region extents 1, one below / at / one above the tile edge, and two tiles plus one, on both axes independently
    const int ext[5] = {1, SSIM_TILE - 1, SSIM_TILE, SSIM_TILE + 1, 2 * SSIM_TILE + 1};
    int form = 0;
    for (int iy = 0; iy < 5; ++iy)
        for (int ix = 0; ix < 5; ++ix, ++form) one_case(5, ext[iy] + 10, ext[ix] + 10, form % 3, form % 2 == 0, 1.0, 0.0);
    const int rs[3] = {0, 1, 12};
    for (int ir = 0; ir < 3; ++ir) {
        const int r = rs[ir];
        one_case(r, 1 + 2 * r, 1 + 2 * r, 0, true, 0.5, 0.5);
        one_case(r, SSIM_TILE + 1 + 2 * r, SSIM_TILE - 1 + 2 * r, 2, true, 0.5, 0.5);
        one_case(r, SSIM_TILE + 2 * r, 2 * SSIM_TILE + 1 + 2 * r, 1, false, 1.0, 0.0);
    }
    if (failures) {
        printf("FAILED: %d mismatches in %d cases\n", failures, cases);
        return 1;
    }
    printf("ok %d\n", cases);
    return 0;
}
