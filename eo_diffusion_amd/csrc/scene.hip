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

// grid (bx, by): blockIdx.y strides the planes p = k * C + c, the x dimension strides the s * s / V items of one plane; plane k holds
// tile k (LIST: tile index[k]).
// V = 4: s % 4 == 0 and `tiles` is 16-byte aligned (vector stores); the loads are vector loads where src_vec (W % 4 == 0 and an
// aligned scene) and the tile's x origin allow it.  An origin outside the scene never reads behind it: that tile is NaN-filled.
template <int V, bool LIST>
__global__ void scene_gather_kernel(const float* __restrict__ scene, float* __restrict__ tiles, const int* __restrict__ oy,
                                    const int* __restrict__ ox, const int* __restrict__ index, int C, int H, int W, int s, int nty,
                                    int ntx, long long planes, int src_vec) {
    const unsigned sq = (unsigned)s / V, per = sq * (unsigned)s;
    for (long long p = blockIdx.y; p < planes; p += gridDim.y) {
        const long long k = p / C;
        const int c = (int)(p - k * C);
        const int i = LIST ? index[k] : 0;
        const bool listed = !LIST || (i >= 0 && i < nty * ntx);
        const int iy = !LIST ? (int)(k / ntx) : listed ? i / ntx : 0;
        const int ix = !LIST ? (int)(k - (long long)iy * ntx) : listed ? i - iy * ntx : 0;
        const int y0 = oy[iy], x0 = ox[ix];
        const bool bad = !listed || y0 < 0 || x0 < 0 || (long long)y0 + s > H || (long long)x0 + s > W;
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

// block (64, 4): threadIdx.x -> a group of V pixels of a row (a wave = 64 consecutive groups), threadIdx.y -> the row r = c * H + y;
// both dimensions are grid-strided.  The x cover ranges are found once per thread, before the row loop.
// V = 4: W % 4 == 0, s % 4 == 0, tiles / scene / wx 16-byte aligned.  A group whose 4 pixels share their covering tiles at x offsets
// that are multiples of 4 takes the vector form; any other group (an odd origin) the scalar form, pixel by pixel -- same arithmetic.
// LIST: every (row, group) first asks whether its pixels are estimated, and writes 0.0f where they are not.
template <int V, bool LIST>
__global__ void scene_blend_kernel(const float* __restrict__ tiles, float* __restrict__ scene, const float* __restrict__ wy,
                                   const float* __restrict__ wx, const int* __restrict__ oy, const int* __restrict__ ox,
                                   const int* __restrict__ slot_of, int C, int H, int W, int s, int nty, int ntx, int n_list) {
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
            const int c = (int)(r / H), y = (int)(r - (long long)c * H);
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

// one block per tile (grid-strided); the block's verdict is formed by __syncthreads_or and stored by thread 0.
template <int V>
__global__ void scene_tile_active_kernel(const float* __restrict__ mask, int* __restrict__ active, const int* __restrict__ oy,
                                         const int* __restrict__ ox, int Cm, int H, int W, int s, int ntx, int n_tiles, int src_vec) {
    const unsigned sq = (unsigned)s / V, per = sq * (unsigned)s;
    for (int i = blockIdx.x; i < n_tiles; i += gridDim.x) {
        const int iy = i / ntx, ix = i - iy * ntx;
        const int y0 = oy[iy], x0 = ox[ix];
        const bool bad = y0 < 0 || x0 < 0 || (long long)y0 + s > H || (long long)x0 + s > W;
        const bool vec = src_vec && (x0 & 3) == 0;
        int hole = bad ? 1 : 0;  // a window that cannot be read is never skipped
        if (!bad) {
            for (int c = 0; c < Cm; ++c) {
                const float* src = mask + ((long long)c * H + y0) * W + x0;
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
        if (threadIdx.x == 0) active[i] = any ? 1 : 0;
    }
}

// out = x where estimated, known elsewhere.  V = 4: W % 4 == 0 and the three tensors 16-byte aligned; a group reads x only, known
// only, or both, by the verdicts of its 4 pixels.
template <int V>
__global__ void scene_keep_known_kernel(const float* __restrict__ xs, const float* __restrict__ known, float* __restrict__ out,
                                        const int* __restrict__ oy, const int* __restrict__ ox, const int* __restrict__ slot_of, int C,
                                        int H, int W, int s, int nty, int ntx, int n_list) {
    const int groups = (W + V - 1) / V;
    const long long rows = (long long)C * H;
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

static inline unsigned grid_cap(long long n, long long cap) { return (unsigned)(n < 1 ? 1 : (n > cap ? cap : n)); }

// n_tiles: how many tiles `tiles` receives (the plan's, or LIST: the list's); index: LIST only
template <bool LIST>
static int launch_gather(const char* what, const float* scene, float* tiles, int C, int H, int W, int s, const int32_t* oy,
                         const int32_t* ox, int nty, int ntx, const int32_t* index, long long n_tiles, void* stream) {
    const long long planes = n_tiles * C;
    const bool v4 = (s % 4 == 0) && eod_aligned16(tiles);
    const int src_vec = v4 && (W % 4 == 0) && eod_aligned16(scene);
    const long long per = (long long)s * s / (v4 ? 4 : 1);
    const unsigned gx = grid_cap((per + 255) / 256, 32);
    dim3 grid(gx, grid_cap(planes, 2048 / gx));
    if (v4)
        hipLaunchKernelGGL((scene_gather_kernel<4, LIST>), grid, dim3(256), 0, (hipStream_t)stream, scene, tiles, oy, ox, index, C, H, W, s, nty, ntx, planes, src_vec);
    else
        hipLaunchKernelGGL((scene_gather_kernel<1, LIST>), grid, dim3(256), 0, (hipStream_t)stream, scene, tiles, oy, ox, index, C, H, W, s, nty, ntx, planes, 0);
    EOD_CHECK_LAUNCH(what);
    return EOD_OK;
}

template <bool LIST>
static int launch_blend(const char* what, const float* tiles, float* scene, const float* wy, const float* wx, const int32_t* oy,
                        const int32_t* ox, const int32_t* slot_of, int n_list, int C, int H, int W, int s, int nty, int ntx, void* stream) {
    const bool v4 = (W % 4 == 0) && (s % 4 == 0) && eod_aligned16(tiles) && eod_aligned16(scene) && eod_aligned16(wx);
    const long long groups = v4 ? W / 4 : W, rows = (long long)C * H;
    const unsigned gx = grid_cap((groups + 63) / 64, 8);
    dim3 grid(gx, grid_cap((rows + 3) / 4, 2048 / gx)), block(64, 4);
    if (v4)
        hipLaunchKernelGGL((scene_blend_kernel<4, LIST>), grid, block, 0, (hipStream_t)stream, tiles, scene, wy, wx, oy, ox, slot_of, C, H, W, s, nty, ntx, n_list);
    else
        hipLaunchKernelGGL((scene_blend_kernel<1, LIST>), grid, block, 0, (hipStream_t)stream, tiles, scene, wy, wx, oy, ox, slot_of, C, H, W, s, nty, ntx, n_list);
    EOD_CHECK_LAUNCH(what);
    return EOD_OK;
}

extern "C" int eod_scene_gather(const float* scene, float* tiles, int C, int H, int W, int s, const int32_t* origins_y,
                                const int32_t* origins_x, int nty, int ntx, void* stream) {
    EOD_REQUIRE(scene && tiles && origins_y && origins_x && C > 0 && H > 0 && W > 0 && s > 0 && nty > 0 && ntx > 0, "scene_gather: bad args");
    EOD_REQUIRE(s <= H && s <= W && s <= 32768, "scene_gather: tile %d does not fit the %d x %d scene", s, H, W);
    return launch_gather<false>("scene_gather", scene, tiles, C, H, W, s, origins_y, origins_x, nty, ntx, nullptr, (long long)nty * ntx, stream);
}

extern "C" int eod_scene_blend(const float* tiles, float* scene, const float* wy, const float* wx, const int32_t* origins_y,
                               const int32_t* origins_x, int C, int H, int W, int s, int nty, int ntx, void* stream) {
    EOD_REQUIRE(tiles && scene && wy && wx && origins_y && origins_x && C > 0 && H > 0 && W > 0 && s > 0 && nty > 0 && ntx > 0, "scene_blend: bad args");
    EOD_REQUIRE(s <= H && s <= W && s <= 32768, "scene_blend: tile %d does not fit the %d x %d scene", s, H, W);
    return launch_blend<false>("scene_blend", tiles, scene, wy, wx, origins_y, origins_x, nullptr, 0, C, H, W, s, nty, ntx, stream);
}

extern "C" int eod_scene_gather_list(const float* scene, float* tiles, int C, int H, int W, int s, const int32_t* origins_y,
                                     const int32_t* origins_x, int nty, int ntx, const int32_t* index, int n_list, void* stream) {
    EOD_REQUIRE(scene && tiles && origins_y && origins_x && index && C > 0 && H > 0 && W > 0 && s > 0 && nty > 0 && ntx > 0, "scene_gather_list: bad args");
    EOD_REQUIRE(s <= H && s <= W && s <= 32768, "scene_gather_list: tile %d does not fit the %d x %d scene", s, H, W);
    EOD_REQUIRE(n_list >= 1 && n_list <= (long long)nty * ntx && (long long)nty * ntx <= 0x7fffffffLL,
                "scene_gather_list: a list of %d tiles for a plan of %d x %d", n_list, nty, ntx);
    return launch_gather<true>("scene_gather_list", scene, tiles, C, H, W, s, origins_y, origins_x, nty, ntx, index, n_list, stream);
}

extern "C" int eod_scene_blend_list(const float* tiles, float* scene, const float* wy, const float* wx, const int32_t* origins_y,
                                    const int32_t* origins_x, const int32_t* slot_of, int n_list, int C, int H, int W, int s, int nty,
                                    int ntx, void* stream) {
    EOD_REQUIRE(tiles && scene && wy && wx && origins_y && origins_x && slot_of && C > 0 && H > 0 && W > 0 && s > 0 && nty > 0 && ntx > 0,
                "scene_blend_list: bad args");
    EOD_REQUIRE(s <= H && s <= W && s <= 32768, "scene_blend_list: tile %d does not fit the %d x %d scene", s, H, W);
    EOD_REQUIRE(n_list >= 1 && n_list <= (long long)nty * ntx && (long long)nty * ntx <= 0x7fffffffLL,
                "scene_blend_list: a list of %d tiles for a plan of %d x %d", n_list, nty, ntx);
    return launch_blend<true>("scene_blend_list", tiles, scene, wy, wx, origins_y, origins_x, slot_of, n_list, C, H, W, s, nty, ntx, stream);
}

extern "C" int eod_scene_tile_active(const float* mask, int32_t* active, int Cm, int H, int W, int s, const int32_t* origins_y,
                                     const int32_t* origins_x, int nty, int ntx, void* stream) {
    EOD_REQUIRE(mask && active && origins_y && origins_x && Cm > 0 && H > 0 && W > 0 && s > 0 && nty > 0 && ntx > 0, "scene_tile_active: bad args");
    EOD_REQUIRE(s <= H && s <= W && s <= 32768, "scene_tile_active: tile %d does not fit the %d x %d mask", s, H, W);
    EOD_REQUIRE((long long)nty * ntx <= 0x7fffffffLL, "scene_tile_active: %d x %d tiles", nty, ntx);
    const int n_tiles = nty * ntx;
    const bool v4 = s % 4 == 0;
    const int src_vec = v4 && (W % 4 == 0) && eod_aligned16(mask);
    dim3 grid(grid_cap(n_tiles, 4096));
    if (v4)
        hipLaunchKernelGGL(scene_tile_active_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, mask, active, origins_y, origins_x, Cm, H, W, s, ntx, n_tiles, src_vec);
    else
        hipLaunchKernelGGL(scene_tile_active_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, mask, active, origins_y, origins_x, Cm, H, W, s, ntx, n_tiles, 0);
    EOD_CHECK_LAUNCH("scene_tile_active");
    return EOD_OK;
}

extern "C" int eod_scene_keep_known(const float* x, const float* known, const int32_t* slot_of, int n_list, const int32_t* origins_y,
                                    const int32_t* origins_x, int C, int H, int W, int s, int nty, int ntx, float* out, void* stream) {
    EOD_REQUIRE(x && known && out && slot_of && origins_y && origins_x && C > 0 && H > 0 && W > 0 && s > 0 && nty > 0 && ntx > 0,
                "scene_keep_known: bad args");
    EOD_REQUIRE(s <= H && s <= W && s <= 32768, "scene_keep_known: tile %d does not fit the %d x %d scene", s, H, W);
    EOD_REQUIRE(n_list >= 1 && n_list <= (long long)nty * ntx && (long long)nty * ntx <= 0x7fffffffLL,
                "scene_keep_known: a list of %d tiles for a plan of %d x %d", n_list, nty, ntx);
    const bool v4 = (W % 4 == 0) && eod_aligned16(x) && eod_aligned16(known) && eod_aligned16(out);
    const long long groups = v4 ? W / 4 : W, rows = (long long)C * H;
    const unsigned gx = grid_cap((groups + 63) / 64, 8);
    dim3 grid(gx, grid_cap((rows + 3) / 4, 2048 / gx)), block(64, 4);
    if (v4)
        hipLaunchKernelGGL(scene_keep_known_kernel<4>, grid, block, 0, (hipStream_t)stream, x, known, out, origins_y, origins_x, slot_of, C, H, W, s, nty, ntx, n_list);
    else
        hipLaunchKernelGGL(scene_keep_known_kernel<1>, grid, block, 0, (hipStream_t)stream, x, known, out, origins_y, origins_x, slot_of, C, H, W, s, nty, ntx, n_list);
    EOD_CHECK_LAUNCH("scene_keep_known");
    return EOD_OK;
}
