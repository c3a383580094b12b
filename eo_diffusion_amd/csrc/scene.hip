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

// grid (bx, by): blockIdx.y strides the planes p = tile * C + c, the x dimension strides the s * s / V items of one plane.
// V = 4: s % 4 == 0 and `tiles` is 16-byte aligned (vector stores); the loads are vector loads where src_vec (W % 4 == 0 and an
// aligned scene) and the tile's x origin allow it.  An origin outside the scene never reads behind it: that tile is NaN-filled.
template <int V>
__global__ void scene_gather_kernel(const float* __restrict__ scene, float* __restrict__ tiles, const int* __restrict__ oy,
                                    const int* __restrict__ ox, int C, int H, int W, int s, int ntx, long long planes, int src_vec) {
    const unsigned sq = (unsigned)s / V, per = sq * (unsigned)s;
    for (long long p = blockIdx.y; p < planes; p += gridDim.y) {
        const long long i = p / C;
        const int c = (int)(p - i * C);
        const int iy = (int)(i / ntx), ix = (int)(i - (long long)iy * ntx);
        const int y0 = oy[iy], x0 = ox[ix];
        const bool bad = y0 < 0 || x0 < 0 || (long long)y0 + s > H || (long long)x0 + s > W;
        const float* src = scene + ((long long)c * H + (bad ? 0 : y0)) * W + (bad ? 0 : x0);
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

// one scene element: the covering tiles in ascending (iy, ix); w = wy * wx, p = w * e, left-to-right sum.
__device__ __forceinline__ float blend_one(const float* __restrict__ tiles, const float* __restrict__ wy, const float* __restrict__ wx,
                                           const int* __restrict__ oy, const int* __restrict__ ox, int c, int y, int x, int C, int s,
                                           int ntx, int fy, int ly, int fx, int lx) {
    const long long plane = (long long)s * s;
    float acc = __builtin_nanf("");  // covered by no tile (a plan from tiling.py covers everything): loud
    bool first = true;
    for (int iy = fy; iy <= ly; ++iy) {
        const int dy = y - oy[iy];
        if ((unsigned)dy >= (unsigned)s) continue;  // (only a table that is not non-decreasing gets here: never read outside a tile)
        const float a = wy[(long long)iy * s + dy];
        for (int ix = fx; ix <= lx; ++ix) {
            const int dx = x - ox[ix];
            if ((unsigned)dx >= (unsigned)s) continue;
            const float w = a * wx[(long long)ix * s + dx];
            const float p = w * tiles[(((long long)iy * ntx + ix) * C + c) * plane + (long long)dy * s + dx];
            acc = first ? p : acc + p;
            first = false;
        }
    }
    return acc;
}

// block (64, 4): threadIdx.x -> a group of V pixels of a row (a wave = 64 consecutive groups), threadIdx.y -> the row r = c * H + y;
// both dimensions are grid-strided.  The x cover ranges are found once per thread, before the row loop.
// V = 4: W % 4 == 0, s % 4 == 0, tiles / scene / wx 16-byte aligned.  A group whose 4 pixels share their covering tiles at x offsets
// that are multiples of 4 takes the vector form; any other group (an odd origin) the scalar form, pixel by pixel -- same arithmetic.
template <int V>
__global__ void scene_blend_kernel(const float* __restrict__ tiles, float* __restrict__ scene, const float* __restrict__ wy,
                                   const float* __restrict__ wx, const int* __restrict__ oy, const int* __restrict__ ox, int C, int H,
                                   int W, int s, int nty, int ntx) {
    const int groups = (W + V - 1) / V;
    const long long rows = (long long)C * H, plane = (long long)s * s;
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < groups; q += gridDim.x * blockDim.x) {
        const int x = q * V;
        int fx[V], lx[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            fx[j] = cover_first(ox, ntx, s, x + j);
            lx[j] = cover_last(ox, ntx, x + j);
        }
        bool uni = V == 4;
        if (V == 4) {
#pragma unroll
            for (int j = 1; j < V; ++j) uni = uni && fx[j] == fx[0] && lx[j] == lx[0];
            for (int ix = fx[0]; ix <= lx[0]; ++ix) uni = uni && ((x - ox[ix]) & 3) == 0;
            uni = uni && fx[0] <= lx[0];
        }
        for (long long r = (long long)blockIdx.y * blockDim.y + threadIdx.y; r < rows; r += (long long)gridDim.y * blockDim.y) {
            const int c = (int)(r / H), y = (int)(r - (long long)c * H);
            const int fy = cover_first(oy, nty, s, y), ly = cover_last(oy, nty, y);
            float* out = scene + r * W + x;
            if (V == 4 && uni && fy <= ly) {
                f32x4 acc;
                bool first = true;
                for (int iy = fy; iy <= ly; ++iy) {
                    const int dy = y - oy[iy];
                    if ((unsigned)dy >= (unsigned)s) continue;
                    const float a = wy[(long long)iy * s + dy];
                    for (int ix = fx[0]; ix <= lx[0]; ++ix) {
                        const int dx = x - ox[ix];
                        if ((unsigned)dx > (unsigned)(s - 4)) continue;
                        const f32x4 w = a * *reinterpret_cast<const f32x4*>(wx + (long long)ix * s + dx);
                        const f32x4 p = w * *reinterpret_cast<const f32x4*>(tiles + (((long long)iy * ntx + ix) * C + c) * plane + (long long)dy * s + dx);
                        acc = first ? p : acc + p;
                        first = false;
                    }
                }
                if (first) acc = f32x4{__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
                *reinterpret_cast<f32x4*>(out) = acc;
            } else {
#pragma unroll
                for (int j = 0; j < V; ++j)
                    if (x + j < W) out[j] = blend_one(tiles, wy, wx, oy, ox, c, y, x + j, C, s, ntx, fy, ly, fx[j], lx[j]);
            }
        }
    }
}

static inline unsigned grid_cap(long long n, long long cap) { return (unsigned)(n < 1 ? 1 : (n > cap ? cap : n)); }

extern "C" int eod_scene_gather(const float* scene, float* tiles, int C, int H, int W, int s, const int32_t* origins_y,
                                const int32_t* origins_x, int nty, int ntx, void* stream) {
    EOD_REQUIRE(scene && tiles && origins_y && origins_x && C > 0 && H > 0 && W > 0 && s > 0 && nty > 0 && ntx > 0, "scene_gather: bad args");
    EOD_REQUIRE(s <= H && s <= W && s <= 32768, "scene_gather: tile %d does not fit the %d x %d scene", s, H, W);
    const long long planes = (long long)nty * ntx * C;
    const bool v4 = (s % 4 == 0) && eod_aligned16(tiles);
    const int src_vec = v4 && (W % 4 == 0) && eod_aligned16(scene);
    const long long per = (long long)s * s / (v4 ? 4 : 1);
    const unsigned gx = grid_cap((per + 255) / 256, 32);
    dim3 grid(gx, grid_cap(planes, 2048 / gx));
    if (v4)
        hipLaunchKernelGGL(scene_gather_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, scene, tiles, origins_y, origins_x, C, H, W, s, ntx, planes, src_vec);
    else
        hipLaunchKernelGGL(scene_gather_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, scene, tiles, origins_y, origins_x, C, H, W, s, ntx, planes, 0);
    EOD_CHECK_LAUNCH("scene_gather");
    return EOD_OK;
}

extern "C" int eod_scene_blend(const float* tiles, float* scene, const float* wy, const float* wx, const int32_t* origins_y,
                               const int32_t* origins_x, int C, int H, int W, int s, int nty, int ntx, void* stream) {
    EOD_REQUIRE(tiles && scene && wy && wx && origins_y && origins_x && C > 0 && H > 0 && W > 0 && s > 0 && nty > 0 && ntx > 0, "scene_blend: bad args");
    EOD_REQUIRE(s <= H && s <= W && s <= 32768, "scene_blend: tile %d does not fit the %d x %d scene", s, H, W);
    const bool v4 = (W % 4 == 0) && (s % 4 == 0) && eod_aligned16(tiles) && eod_aligned16(scene) && eod_aligned16(wx);
    const long long groups = v4 ? W / 4 : W, rows = (long long)C * H;
    const unsigned gx = grid_cap((groups + 63) / 64, 8);
    dim3 grid(gx, grid_cap((rows + 3) / 4, 2048 / gx)), block(64, 4);
    if (v4)
        hipLaunchKernelGGL(scene_blend_kernel<4>, grid, block, 0, (hipStream_t)stream, tiles, scene, wy, wx, origins_y, origins_x, C, H, W, s, nty, ntx);
    else
        hipLaunchKernelGGL(scene_blend_kernel<1>, grid, block, 0, (hipStream_t)stream, tiles, scene, wy, wx, origins_y, origins_x, C, H, W, s, nty, ntx);
    EOD_CHECK_LAUNCH("scene_blend");
    return EOD_OK;
}
