// Whole-scene sampling: the two streaming kernels between a scene-sized diffusion state and the UNet-sized tiles
// (eo_diffusion_amd/tiling.py builds the plan: origins and separable fp32 blend weights per axis).
//
//   scene_gather   scene [C][H][W] -> tiles [nty*ntx][C][s][s]                      (a copy: bit-exact by construction)
//   scene_blend    tiles [nty*ntx][C][s][s] -> scene [C][H][W],  e = sum_i w_i e_i  over the tiles covering each pixel
//
// THIS FILE IS COMPILED WITH -ffp-contract=off (like sampler.hip): the blend forms w = wy * wx, p = w * e and the left-to-right
// sum over the covering tiles in ascending (iy, ix) as separately rounded fp32 operations, so its result is a pure function of
// its inputs (no atomics, nothing depends on the launch geometry) and a plain torch emulation reproduces it bit for bit
// (tests/test_gpu_scene.py).  A pixel covered by one tile has weight 1.0f * 1.0f: the estimate passes through unchanged.
//
// Both are HBM-bound: one 16-byte access per lane wherever W, s, the origins and the pointers allow it, a wave covers 1 KiB of
// one row.  The scalar forms serve odd W, odd origins and unaligned views; the vector kernels fall back to them per tile
// (gather) or per 4-pixel group (blend), so a plan with SOME odd origins still moves most of its bytes 16 at a time.
// Indices are 64-bit: a 10980 x 10980 x 13 scene has 1.57e9 elements.
#include "common.h"

// Tiles are numbered row-major, origins are non-decreasing per axis and tile i covers [o[i], o[i] + s): the tiles covering a
// coordinate v are the contiguous index range [cover_first, cover_last] (empty when first > last: v is covered by no tile).
__device__ __forceinline__ int cover_first(const int* __restrict__ o, int n, int s, int v) {  // smallest i with o[i] + s > v
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (o[mid] + s > v) hi = mid; else lo = mid + 1;
    }
    return lo;
}
__device__ __forceinline__ int cover_last(const int* __restrict__ o, int n, int v) {  // largest i with o[i] <= v
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (o[mid] <= v) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ------------------------------------------------------------------------------------------------------------------------------
// A tile SUBSET: the tiles whose window holds a hole pixel of a RePaint mask (tiling.py TileSubset).  Only they go through the
// network, in a compact buffer tiles [n_list][C][s][s]; `index` [n_list] names the tile in each slot (ascending), `slot_of`
// [nty * ntx] the slot of each tile or -1.  A pixel is ESTIMATED when every tile covering it is listed: there the list blend is the
// full blend's arithmetic (same weights, same ascending order, same roundings); everywhere else it writes 0.0f.
//
//   scene_tile_active   mask [Cm][H][W] -> active [nty*ntx]: 1 iff a value of the tile's window is != 1.0f (NaN counts)
//   scene_gather_list   scene -> tiles[k] = the window of tile index[k]                  (scene_gather_kernel<V, LIST = true>)
//   scene_blend_list    tiles -> scene at estimated pixels, 0.0f elsewhere               (scene_blend_kernel<V, LIST = true>)
//   scene_keep_known    out = x at estimated pixels, known elsewhere
//
// None of them trusts the tables with an address: an index / slot outside its range reads nothing (NaN tile, absent tile).
//
// The gather and the blend are ONE kernel each, templated on LIST: at compile time the flag picks where a tile's number comes from
// (the plane / tile number, or `index` / `slot_of`; the full-plan instantiations carry those tables as unused null arguments) and
// what a pixel gets that nobody estimates (NaN, loud, or 0.0f behind the estimated_at gate).

// A STACK of B scenes of one plan (tiling.py TileStack): scene / x / known / out are [B][C][H][W], mask is [B][Cm][H][W], and a tile has
// the global number g = b * nty * ntx + i.  Every kernel below takes B; the single-scene entry points are its B = 1 case.  `index` holds
// global numbers, `slot_of` is [B * nty * ntx], and "estimated" is asked per scene, of that scene's nty * ntx entries of slot_of.

// grid (bx, by): blockIdx.y strides the planes p = k * C + c, the x dimension strides the s * s / V items of one plane; plane k holds
// tile g = k (LIST: g = index[k]) = tile i of scene b.
// V = 4: s % 4 == 0 and `tiles` is 16-byte aligned (vector stores); the loads are vector loads where src_vec (W % 4 == 0 and an
// aligned scene) and the tile's x origin allow it.  An origin outside the scene never reads behind it: that tile is NaN-filled.
template <int V, bool LIST>
__global__ void scene_gather_kernel(const float* __restrict__ scene, float* __restrict__ tiles, const int* __restrict__ oy,
                                    const int* __restrict__ ox, const int* __restrict__ index, int B, int C, int H, int W, int s, int nty,
                                    int ntx, long long planes, int src_vec) {
    const unsigned sq = (unsigned)s / V, per = sq * (unsigned)s;
    for (long long p = blockIdx.y; p < planes; p += gridDim.y) {
        const long long k = p / C;
        const int c = (int)(p - k * C);
        const int nt = nty * ntx;
        const long long g = LIST ? (long long)index[k] : k;
        const bool listed = !LIST || (g >= 0 && g < (long long)B * nt);
        const int b = listed ? (int)(g / nt) : 0;
        const int i = listed ? (int)(g - (long long)b * nt) : 0;
        const int iy = i / ntx, ix = i - iy * ntx;
        const int y0 = oy[iy], x0 = ox[ix];
        const bool bad = !listed || y0 < 0 || x0 < 0 || (long long)y0 + s > H || (long long)x0 + s > W;
        const float* src = scene + (((long long)b * C + c) * H + (bad ? 0 : y0)) * W + (bad ? 0 : x0);
        float* dst = tiles + p * (long long)s * s;
        const bool vec = src_vec && (x0 & 3) == 0;
        for (unsigned j = blockIdx.x * blockDim.x + threadIdx.x; j < per; j += gridDim.x * blockDim.x) {
            const unsigned ly = j / sq, lq = j - ly * sq;
            const float* a = src + (long long)ly * W + lq * V;
            if (V == 4) {
                f32x4 v;
                if (bad) {
                    v = f32x4{__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
                } else if (vec) {
                    v = *reinterpret_cast<const f32x4*>(a);
                } else {
                    v = f32x4{a[0], a[1], a[2], a[3]};
                }
                *reinterpret_cast<f32x4*>(dst + (long long)j * 4) = v;
            } else {
                dst[j] = bad ? __builtin_nanf("") : a[0];
            }
        }
    }
}

// is (y, x) estimated: covered by at least one tile, and every covering tile has a slot in [0, n_list)
__device__ __forceinline__ bool estimated_at(const int* __restrict__ slot_of, const int* __restrict__ oy, const int* __restrict__ ox,
                                             int y, int x, int s, int ntx, int n_list, int fy, int ly, int fx, int lx) {
    bool any = false, all = true;
    for (int iy = fy; iy <= ly; ++iy) {
        if ((unsigned)(y - oy[iy]) >= (unsigned)s) continue;
        for (int ix = fx; ix <= lx; ++ix) {
            if ((unsigned)(x - ox[ix]) >= (unsigned)s) continue;
            any = true;
            all = all && (unsigned)slot_of[(long long)iy * ntx + ix] < (unsigned)n_list;
        }
    }
    return any && all;
}

// one scene element: the covering tiles in ascending (iy, ix); w = wy * wx, p = w * e, left-to-right sum.
// LIST: only called at an estimated pixel (every slot read is in [0, n_list)).
template <bool LIST>
__device__ __forceinline__ float blend_one(const float* __restrict__ tiles, const float* __restrict__ wy, const float* __restrict__ wx,
                                           const int* __restrict__ oy, const int* __restrict__ ox, const int* __restrict__ slot_of,
                                           int c, int y, int x, int C, int s, int ntx, int fy, int ly, int fx, int lx) {
    const long long plane = (long long)s * s;
    float acc = LIST ? 0.0f : __builtin_nanf("");  // full plan: covered by no tile (a plan from tiling.py covers everything): loud
    bool first = true;
    for (int iy = fy; iy <= ly; ++iy) {
        const int dy = y - oy[iy];
        if ((unsigned)dy >= (unsigned)s) continue;  // (only a table that is not non-decreasing gets here: never read outside a tile)
        const float a = wy[(long long)iy * s + dy];
        for (int ix = fx; ix <= lx; ++ix) {
            const int dx = x - ox[ix];
            if ((unsigned)dx >= (unsigned)s) continue;
            const float w = a * wx[(long long)ix * s + dx];
            const long long i = (long long)iy * ntx + ix;  // the tile's place in `tiles`: its number, or (LIST) its slot
            const float p = w * tiles[((LIST ? slot_of[i] : i) * C + c) * plane + (long long)dy * s + dx];
            acc = first ? p : acc + p;
            first = false;
        }
    }
    return acc;
}

// block (64, 4): threadIdx.x -> a group of V pixels of a row (a wave = 64 consecutive groups), threadIdx.y -> the row r = (b * C + c) * H + y;
// both dimensions are grid-strided.  The x cover ranges are found once per thread, before the row loop.
// V = 4: W % 4 == 0, s % 4 == 0, tiles / scene / wx 16-byte aligned.  A group whose 4 pixels share their covering tiles at x offsets
// that are multiples of 4 takes the vector form; any other group (an odd origin) the scalar form, pixel by pixel -- same arithmetic.
// LIST: every (row, group) first asks whether its pixels are estimated, and writes 0.0f where they are not.
// Scene b sees its own tiles only: the full plan's `tiles` and LIST's `slot_of` are advanced to scene b's nty * ntx entries per row, and
// the arithmetic below is the single scene's.
template <int V, bool LIST>
__global__ void scene_blend_kernel(const float* __restrict__ tiles0, float* __restrict__ scene, const float* __restrict__ wy,
                                   const float* __restrict__ wx, const int* __restrict__ oy, const int* __restrict__ ox,
                                   const int* __restrict__ slot0, int B, int C, int H, int W, int s, int nty, int ntx, int n_list) {
    const int groups = (W + V - 1) / V;
    const long long rows = (long long)B * C * H, plane = (long long)s * s, nt = (long long)nty * ntx;
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < groups; q += gridDim.x * blockDim.x) {
        const int x = q * V;
        int fx[V], lx[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            fx[j] = cover_first(ox, ntx, s, x + j);
            lx[j] = cover_last(ox, ntx, x + j);
        }
        // a vector access must end inside its tile (dx <= s - 4).  LIST tests that here, once per group, because its gate
        // (estimated_at) has to see every covering tile; the full plan skips such a tile inside the row loop.
        bool uni = V == 4;
        if (V == 4) {
#pragma unroll
            for (int j = 1; j < V; ++j) uni = uni && fx[j] == fx[0] && lx[j] == lx[0];
            for (int ix = fx[0]; ix <= lx[0]; ++ix)
                uni = uni && ((x - ox[ix]) & 3) == 0 && (!LIST || (unsigned)(x - ox[ix]) <= (unsigned)(s - 4));
            uni = uni && fx[0] <= lx[0];
        }
        for (long long r = (long long)blockIdx.y * blockDim.y + threadIdx.y; r < rows; r += (long long)gridDim.y * blockDim.y) {
            const long long bc = r / H;
            const int y = (int)(r - bc * H), b = (int)(bc / C), c = (int)(bc - (long long)b * C);
            const float* tiles = LIST ? tiles0 : tiles0 + b * nt * C * plane;
            const int* slot_of = LIST ? slot0 + b * nt : slot0;
            const int fy = cover_first(oy, nty, s, y), ly = cover_last(oy, nty, y);
            float* out = scene + r * W + x;
            if (V == 4 && uni && fy <= ly) {  // the 4 pixels share their covering tiles (LIST: and therefore one verdict)
                f32x4 acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                bool first = true;
                if (!LIST || estimated_at(slot_of, oy, ox, y, x, s, ntx, n_list, fy, ly, fx[0], lx[0])) {
                    for (int iy = fy; iy <= ly; ++iy) {
                        const int dy = y - oy[iy];
                        if ((unsigned)dy >= (unsigned)s) continue;
                        const float a = wy[(long long)iy * s + dy];
                        for (int ix = fx[0]; ix <= lx[0]; ++ix) {
                            const int dx = x - ox[ix];
                            if (!LIST && (unsigned)dx > (unsigned)(s - 4)) continue;
                            const f32x4 w = a * *reinterpret_cast<const f32x4*>(wx + (long long)ix * s + dx);
                            const long long i = (long long)iy * ntx + ix;
                            const f32x4 p = w * *reinterpret_cast<const f32x4*>(tiles + ((LIST ? slot_of[i] : i) * C + c) * plane + (long long)dy * s + dx);
                            acc = first ? p : acc + p;
                            first = false;
                        }
                    }
                }
                if (!LIST && first) acc = f32x4{__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
                *reinterpret_cast<f32x4*>(out) = acc;
            } else {
#pragma unroll
                for (int j = 0; j < V; ++j)
                    if (x + j < W)
                        out[j] = (!LIST || estimated_at(slot_of, oy, ox, y, x + j, s, ntx, n_list, fy, ly, fx[j], lx[j]))
                                     ? blend_one<LIST>(tiles, wy, wx, oy, ox, slot_of, c, y, x + j, C, s, ntx, fy, ly, fx[j], lx[j])
                                     : 0.0f;
            }
        }
    }
}

// one block per tile g of the stack (grid-strided); the block's verdict is formed by __syncthreads_or and stored by thread 0.
template <int V>
__global__ void scene_tile_active_kernel(const float* __restrict__ mask, int* __restrict__ active, const int* __restrict__ oy,
                                         const int* __restrict__ ox, int Cm, int H, int W, int s, int ntx, int nt, int n_tiles, int src_vec) {
    const unsigned sq = (unsigned)s / V, per = sq * (unsigned)s;
    for (int g = blockIdx.x; g < n_tiles; g += gridDim.x) {  // n_tiles = B * nt
        const int b = g / nt, i = g - b * nt;
        const int iy = i / ntx, ix = i - iy * ntx;
        const int y0 = oy[iy], x0 = ox[ix];
        const bool bad = y0 < 0 || x0 < 0 || (long long)y0 + s > H || (long long)x0 + s > W;
        const bool vec = src_vec && (x0 & 3) == 0;
        int hole = bad ? 1 : 0;  // a window that cannot be read is never skipped
        if (!bad) {
            for (int c = 0; c < Cm; ++c) {
                const float* src = mask + (((long long)b * Cm + c) * H + y0) * W + x0;
                for (unsigned j = threadIdx.x; j < per; j += blockDim.x) {
                    const unsigned ly = j / sq, lq = j - ly * sq;
                    const float* a = src + (long long)ly * W + lq * V;
                    if (V == 4) {
                        const f32x4 v = vec ? *reinterpret_cast<const f32x4*>(a) : f32x4{a[0], a[1], a[2], a[3]};
                        hole |= (v.x != 1.0f) | (v.y != 1.0f) | (v.z != 1.0f) | (v.w != 1.0f);
                    } else {
                        hole |= a[0] != 1.0f;
                    }
                }
            }
        }
        const int any = __syncthreads_or(hole);
        if (threadIdx.x == 0) active[g] = any ? 1 : 0;
    }
}

// out = x where estimated, known elsewhere.  V = 4: W % 4 == 0 and the three tensors 16-byte aligned; a group reads x only, known
// only, or both, by the verdicts of its 4 pixels.
template <int V>
__global__ void scene_keep_known_kernel(const float* __restrict__ xs, const float* __restrict__ known, float* __restrict__ out,
                                        const int* __restrict__ oy, const int* __restrict__ ox, const int* __restrict__ slot0, int B, int C,
                                        int H, int W, int s, int nty, int ntx, int n_list) {
    const int groups = (W + V - 1) / V;
    const long long rows = (long long)B * C * H, nt = (long long)nty * ntx;
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < groups; q += gridDim.x * blockDim.x) {
        const int x = q * V;
        int fx[V], lx[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            fx[j] = cover_first(ox, ntx, s, x + j);
            lx[j] = cover_last(ox, ntx, x + j);
        }
        for (long long r = (long long)blockIdx.y * blockDim.y + threadIdx.y; r < rows; r += (long long)gridDim.y * blockDim.y) {
            const int y = (int)(r % H);
            const int* slot_of = slot0 + (r / ((long long)C * H)) * nt;  // scene b's entries
            const int fy = cover_first(oy, nty, s, y), ly = cover_last(oy, nty, y);
            bool est[V];
            bool any = false, all = true;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                est[j] = x + j < W && estimated_at(slot_of, oy, ox, y, x + j, s, ntx, n_list, fy, ly, fx[j], lx[j]);
                any = any || est[j];
                all = all && est[j];
            }
            const long long at = r * W + x;
            if (V == 4) {
                f32x4 v;
                if (all) {
                    v = *reinterpret_cast<const f32x4*>(xs + at);
                } else {
                    v = *reinterpret_cast<const f32x4*>(known + at);
                    if (any) {
                        const f32x4 a = *reinterpret_cast<const f32x4*>(xs + at);
                        v = f32x4{est[0] ? a.x : v.x, est[1] ? a.y : v.y, est[2] ? a.z : v.z, est[3] ? a.w : v.w};
                    }
                }
                *reinterpret_cast<f32x4*>(out + at) = v;
            } else {
                out[at] = est[0] ? xs[at] : known[at];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Per-pixel mean and spread of a stack x [B][n] (n = C * H * W): one pass, every operation separately rounded in fp32
//   s = x_0; s = s + x_b (ascending b);  mean = s / (float)B;  q = sum_b d * d, d = x_b - mean, left to right;
//   std = sqrtf(q / (float)(B - 1)),  B = 1: std = 0.
// The division and the square root are the correctly rounded ones, so a plain fp32 emulation on the host reproduces both outputs bit
// for bit: hipcc's fp32 `/` is (v_div_scale / v_div_fmas / v_div_fixup); its sqrtf compiles to a bare v_sqrt_f32, which the ISA specifies
// to 1 ulp only, hence sqrt_rn below.  The first STATS_REG members stay in registers between the two sums (HBM is read once); a
// deeper stack re-reads the rest.  V = 4: n % 4 == 0 and x / mean / std 16-byte aligned (then every x_b is); the scalar form otherwise,
// for the WHOLE array: x_b = x + b * n, so with n % 4 != 0 the members are misaligned against each other and a vector body with a
// scalar tail could serve 16-byte loads to one member in four only.
// sqrtf rounded to nearest: the fp64 root, rounded once more.  The exact root of an fp32 number is never within 2^-50 (relative) of
// the midpoint of two fp32 numbers -- y = sqrt(x), m a midpoint: |x - m^2| is an odd multiple of 2^-48 of x's binade, so
// |y - m| = |x - m^2| / (y + m) >= 2^-50 -- and the fp64 root is within 2^-52 of it, so both round to the same fp32 number.
__device__ __forceinline__ float sqrt_rn(float q) { return (float)sqrt((double)q); }

constexpr int STATS_REG = 16;
template <int V>
__global__ void scene_stats_kernel(const float* __restrict__ x, float* __restrict__ mean, float* __restrict__ sd, int B, long long n) {
    typedef float vec __attribute__((ext_vector_type(V)));
    const long long items = n / V;
    const float fB = (float)B, fB1 = (float)(B - 1);
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < items; j += (long long)gridDim.x * blockDim.x) {
        const vec* px = reinterpret_cast<const vec*>(x) + j;
        vec v[STATS_REG];
#pragma unroll
        for (int b = 0; b < STATS_REG; ++b)
            if (b < B) v[b] = px[(long long)b * items];
        vec sum = v[0];
#pragma unroll
        for (int b = 1; b < STATS_REG; ++b)
            if (b < B) sum = sum + v[b];
        for (int b = STATS_REG; b < B; ++b) sum = sum + px[(long long)b * items];
        const vec m = sum / fB;
        vec d = v[0] - m;
        vec q = d * d;
#pragma unroll
        for (int b = 1; b < STATS_REG; ++b)
            if (b < B) {
                d = v[b] - m;
                q = q + d * d;
            }
        for (int b = STATS_REG; b < B; ++b) {
            d = px[(long long)b * items] - m;
            q = q + d * d;
        }
        vec r = vec(0.0f);  // B = 1
        if (B > 1) {
            q = q / fB1;
#pragma unroll
            for (int e = 0; e < V; ++e) r[e] = sqrt_rn(q[e]);
        }
        reinterpret_cast<vec*>(mean)[j] = m;
        reinterpret_cast<vec*>(sd)[j] = r;
    }
}

static inline unsigned grid_cap(long long n, long long cap) { return (unsigned)(n < 1 ? 1 : (n > cap ? cap : n)); }

// n_tiles: how many tiles `tiles` receives (the stack's B * nty * ntx, or LIST: the list's); index: LIST only
template <bool LIST>
static int launch_gather(const char* what, const float* scene, float* tiles, int B, int C, int H, int W, int s, const int32_t* oy,
                         const int32_t* ox, int nty, int ntx, const int32_t* index, long long n_tiles, void* stream) {
    const long long planes = n_tiles * C;
    const bool v4 = (s % 4 == 0) && eod_aligned16(tiles);
    const int src_vec = v4 && (W % 4 == 0) && eod_aligned16(scene);
    const long long per = (long long)s * s / (v4 ? 4 : 1);
    const unsigned gx = grid_cap((per + 255) / 256, 32);
    dim3 grid(gx, grid_cap(planes, 2048 / gx));
    if (v4)
        hipLaunchKernelGGL((scene_gather_kernel<4, LIST>), grid, dim3(256), 0, (hipStream_t)stream, scene, tiles, oy, ox, index, B, C, H, W, s, nty, ntx, planes, src_vec);
    else
        hipLaunchKernelGGL((scene_gather_kernel<1, LIST>), grid, dim3(256), 0, (hipStream_t)stream, scene, tiles, oy, ox, index, B, C, H, W, s, nty, ntx, planes, 0);
    EOD_CHECK_LAUNCH(what);
    return EOD_OK;
}

template <bool LIST>
static int launch_blend(const char* what, const float* tiles, float* scene, const float* wy, const float* wx, const int32_t* oy,
                        const int32_t* ox, const int32_t* slot_of, int n_list, int B, int C, int H, int W, int s, int nty, int ntx,
                        void* stream) {
    const bool v4 = (W % 4 == 0) && (s % 4 == 0) && eod_aligned16(tiles) && eod_aligned16(scene) && eod_aligned16(wx);
    const long long groups = v4 ? W / 4 : W, rows = (long long)B * C * H;
    const unsigned gx = grid_cap((groups + 63) / 64, 8);
    dim3 grid(gx, grid_cap((rows + 3) / 4, 2048 / gx)), block(64, 4);
    if (v4)
        hipLaunchKernelGGL((scene_blend_kernel<4, LIST>), grid, block, 0, (hipStream_t)stream, tiles, scene, wy, wx, oy, ox, slot_of, B, C, H, W, s, nty, ntx, n_list);
    else
        hipLaunchKernelGGL((scene_blend_kernel<1, LIST>), grid, block, 0, (hipStream_t)stream, tiles, scene, wy, wx, oy, ox, slot_of, B, C, H, W, s, nty, ntx, n_list);
    EOD_CHECK_LAUNCH(what);
    return EOD_OK;
}

static int launch_tile_active(const char* what, const float* mask, int32_t* active, int B, int Cm, int H, int W, int s, const int32_t* oy,
                              const int32_t* ox, int nty, int ntx, void* stream) {
    const int nt = nty * ntx, n_tiles = B * nt;
    const bool v4 = s % 4 == 0;
    const int src_vec = v4 && (W % 4 == 0) && eod_aligned16(mask);
    dim3 grid(grid_cap(n_tiles, 4096));
    if (v4)
        hipLaunchKernelGGL(scene_tile_active_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, mask, active, oy, ox, Cm, H, W, s, ntx, nt, n_tiles, src_vec);
    else
        hipLaunchKernelGGL(scene_tile_active_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, mask, active, oy, ox, Cm, H, W, s, ntx, nt, n_tiles, 0);
    EOD_CHECK_LAUNCH(what);
    return EOD_OK;
}

static int launch_keep_known(const char* what, const float* x, const float* known, const int32_t* slot_of, int n_list, const int32_t* oy,
                             const int32_t* ox, int B, int C, int H, int W, int s, int nty, int ntx, float* out, void* stream) {
    const bool v4 = (W % 4 == 0) && eod_aligned16(x) && eod_aligned16(known) && eod_aligned16(out);
    const long long groups = v4 ? W / 4 : W, rows = (long long)B * C * H;
    const unsigned gx = grid_cap((groups + 63) / 64, 8);
    dim3 grid(gx, grid_cap((rows + 3) / 4, 2048 / gx)), block(64, 4);
    if (v4)
        hipLaunchKernelGGL(scene_keep_known_kernel<4>, grid, block, 0, (hipStream_t)stream, x, known, out, oy, ox, slot_of, B, C, H, W, s, nty, ntx, n_list);
    else
        hipLaunchKernelGGL(scene_keep_known_kernel<1>, grid, block, 0, (hipStream_t)stream, x, known, out, oy, ox, slot_of, B, C, H, W, s, nty, ntx, n_list);
    EOD_CHECK_LAUNCH(what);
    return EOD_OK;
}

// what every entry point asks of its plan (and of B: the stack's tiles are numbered in an int)
#define SCENE_REQUIRE_PLAN(what, B, C, H, W, s, nty, ntx)                                                                              \
    EOD_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && s > 0 && nty > 0 && ntx > 0, what ": bad args");                                      \
    EOD_REQUIRE(s <= H && s <= W && s <= 32768, what ": tile %d does not fit the %d x %d scene", s, H, W);                                 \
    EOD_REQUIRE((long long)B * nty * ntx <= 0x7fffffffLL, what ": %d scenes of %d x %d tiles", B, nty, ntx)
#define SCENE_REQUIRE_LIST(what, n_list, B, nty, ntx)                                                                                   \
    EOD_REQUIRE(n_list >= 1 && n_list <= (long long)B * nty * ntx, what ": a list of %d tiles for %d scene(s) of %d x %d", n_list, B, nty, ntx)

extern "C" int eod_scene_gather(const float* scene, float* tiles, int C, int H, int W, int s, const int32_t* origins_y,
                                const int32_t* origins_x, int nty, int ntx, void* stream) {
    EOD_REQUIRE(scene && tiles && origins_y && origins_x && C > 0 && H > 0 && W > 0 && s > 0 && nty > 0 && ntx > 0, "scene_gather: bad args");
    EOD_REQUIRE(s <= H && s <= W && s <= 32768, "scene_gather: tile %d does not fit the %d x %d scene", s, H, W);
    return launch_gather<false>("scene_gather", scene, tiles, 1, C, H, W, s, origins_y, origins_x, nty, ntx, nullptr, (long long)nty * ntx, stream);
}

extern "C" int eod_scene_blend(const float* tiles, float* scene, const float* wy, const float* wx, const int32_t* origins_y,
                               const int32_t* origins_x, int C, int H, int W, int s, int nty, int ntx, void* stream) {
    EOD_REQUIRE(tiles && scene && wy && wx && origins_y && origins_x && C > 0 && H > 0 && W > 0 && s > 0 && nty > 0 && ntx > 0, "scene_blend: bad args");
    EOD_REQUIRE(s <= H && s <= W && s <= 32768, "scene_blend: tile %d does not fit the %d x %d scene", s, H, W);
    return launch_blend<false>("scene_blend", tiles, scene, wy, wx, origins_y, origins_x, nullptr, 0, 1, C, H, W, s, nty, ntx, stream);
}

extern "C" int eod_scene_gather_list(const float* scene, float* tiles, int C, int H, int W, int s, const int32_t* origins_y,
                                     const int32_t* origins_x, int nty, int ntx, const int32_t* index, int n_list, void* stream) {
    EOD_REQUIRE(scene && tiles && origins_y && origins_x && index, "scene_gather_list: bad args");
    SCENE_REQUIRE_PLAN("scene_gather_list", 1, C, H, W, s, nty, ntx);
    SCENE_REQUIRE_LIST("scene_gather_list", n_list, 1, nty, ntx);
    return launch_gather<true>("scene_gather_list", scene, tiles, 1, C, H, W, s, origins_y, origins_x, nty, ntx, index, n_list, stream);
}

extern "C" int eod_scene_blend_list(const float* tiles, float* scene, const float* wy, const float* wx, const int32_t* origins_y,
                                    const int32_t* origins_x, const int32_t* slot_of, int n_list, int C, int H, int W, int s, int nty,
                                    int ntx, void* stream) {
    EOD_REQUIRE(tiles && scene && wy && wx && origins_y && origins_x && slot_of, "scene_blend_list: bad args");
    SCENE_REQUIRE_PLAN("scene_blend_list", 1, C, H, W, s, nty, ntx);
    SCENE_REQUIRE_LIST("scene_blend_list", n_list, 1, nty, ntx);
    return launch_blend<true>("scene_blend_list", tiles, scene, wy, wx, origins_y, origins_x, slot_of, n_list, 1, C, H, W, s, nty, ntx, stream);
}

extern "C" int eod_scene_tile_active(const float* mask, int32_t* active, int Cm, int H, int W, int s, const int32_t* origins_y,
                                     const int32_t* origins_x, int nty, int ntx, void* stream) {
    EOD_REQUIRE(mask && active && origins_y && origins_x, "scene_tile_active: bad args");
    SCENE_REQUIRE_PLAN("scene_tile_active", 1, Cm, H, W, s, nty, ntx);
    return launch_tile_active("scene_tile_active", mask, active, 1, Cm, H, W, s, origins_y, origins_x, nty, ntx, stream);
}

extern "C" int eod_scene_keep_known(const float* x, const float* known, const int32_t* slot_of, int n_list, const int32_t* origins_y,
                                    const int32_t* origins_x, int C, int H, int W, int s, int nty, int ntx, float* out, void* stream) {
    EOD_REQUIRE(x && known && out && slot_of && origins_y && origins_x, "scene_keep_known: bad args");
    SCENE_REQUIRE_PLAN("scene_keep_known", 1, C, H, W, s, nty, ntx);
    SCENE_REQUIRE_LIST("scene_keep_known", n_list, 1, nty, ntx);
    return launch_keep_known("scene_keep_known", x, known, slot_of, n_list, origins_y, origins_x, 1, C, H, W, s, nty, ntx, out, stream);
}

// ---- the same four on a stack of B scenes; a null index / slot_of selects the full form (n_list is then ignored)
extern "C" int eod_scene_stack_gather(const float* scene, float* tiles, int B, int C, int H, int W, int s, const int32_t* origins_y,
                                      const int32_t* origins_x, int nty, int ntx, const int32_t* index, int n_list, void* stream) {
    EOD_REQUIRE(scene && tiles && origins_y && origins_x, "scene_stack_gather: bad args");
    SCENE_REQUIRE_PLAN("scene_stack_gather", B, C, H, W, s, nty, ntx);
    if (!index)
        return launch_gather<false>("scene_stack_gather", scene, tiles, B, C, H, W, s, origins_y, origins_x, nty, ntx, nullptr, (long long)B * nty * ntx, stream);
    SCENE_REQUIRE_LIST("scene_stack_gather", n_list, B, nty, ntx);
    return launch_gather<true>("scene_stack_gather", scene, tiles, B, C, H, W, s, origins_y, origins_x, nty, ntx, index, n_list, stream);
}

extern "C" int eod_scene_stack_blend(const float* tiles, float* scene, const float* wy, const float* wx, const int32_t* origins_y,
                                     const int32_t* origins_x, const int32_t* slot_of, int n_list, int B, int C, int H, int W, int s,
                                     int nty, int ntx, void* stream) {
    EOD_REQUIRE(tiles && scene && wy && wx && origins_y && origins_x, "scene_stack_blend: bad args");
    SCENE_REQUIRE_PLAN("scene_stack_blend", B, C, H, W, s, nty, ntx);
    if (!slot_of)
        return launch_blend<false>("scene_stack_blend", tiles, scene, wy, wx, origins_y, origins_x, nullptr, 0, B, C, H, W, s, nty, ntx, stream);
    SCENE_REQUIRE_LIST("scene_stack_blend", n_list, B, nty, ntx);
    return launch_blend<true>("scene_stack_blend", tiles, scene, wy, wx, origins_y, origins_x, slot_of, n_list, B, C, H, W, s, nty, ntx, stream);
}

extern "C" int eod_scene_stack_tile_active(const float* mask, int32_t* active, int B, int Cm, int H, int W, int s, const int32_t* origins_y,
                                           const int32_t* origins_x, int nty, int ntx, void* stream) {
    EOD_REQUIRE(mask && active && origins_y && origins_x, "scene_stack_tile_active: bad args");
    SCENE_REQUIRE_PLAN("scene_stack_tile_active", B, Cm, H, W, s, nty, ntx);
    return launch_tile_active("scene_stack_tile_active", mask, active, B, Cm, H, W, s, origins_y, origins_x, nty, ntx, stream);
}

extern "C" int eod_scene_stack_keep_known(const float* x, const float* known, const int32_t* slot_of, int n_list, const int32_t* origins_y,
                                          const int32_t* origins_x, int B, int C, int H, int W, int s, int nty, int ntx, float* out,
                                          void* stream) {
    EOD_REQUIRE(x && known && out && slot_of && origins_y && origins_x, "scene_stack_keep_known: bad args");
    SCENE_REQUIRE_PLAN("scene_stack_keep_known", B, C, H, W, s, nty, ntx);
    SCENE_REQUIRE_LIST("scene_stack_keep_known", n_list, B, nty, ntx);
    return launch_keep_known("scene_stack_keep_known", x, known, slot_of, n_list, origins_y, origins_x, B, C, H, W, s, nty, ntx, out, stream);
}

extern "C" int eod_scene_stats(const float* x, float* mean, float* std_out, int B, int64_t n, void* stream) {
    EOD_REQUIRE(x && mean && std_out && B > 0 && n > 0, "scene_stats: bad args");
    const bool v4 = (n % 4 == 0) && eod_aligned16(x) && eod_aligned16(mean) && eod_aligned16(std_out);
    const long long items = v4 ? n / 4 : n;
    dim3 grid(grid_cap((items + 255) / 256, 2048));
    if (v4)
        hipLaunchKernelGGL(scene_stats_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, x, mean, std_out, B, (long long)n);
    else
        hipLaunchKernelGGL(scene_stats_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, x, mean, std_out, B, (long long)n);
    EOD_CHECK_LAUNCH("scene_stats");
    return EOD_OK;
}
