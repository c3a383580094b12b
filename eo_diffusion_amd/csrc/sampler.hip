// Fused DDPM / DDIM sampler updates.  HBM-bound elementwise kernels, one pass
// over x_t, 16-byte accesses where the shape allows.
//
// THIS FILE IS COMPILED WITH -ffp-contract=off: every multiply/add/div/sqrt below is a separately
// rounded IEEE fp32 operation in exactly the order of the reference's torch expression, so the
// results are bit-identical to the torch CPU path (tests/test_gpu_sampler.py checks bits).
// hipcc's default correctly-rounded fp32 divide and sqrt are relied upon (no fast-math here).
//
//   q_sample      diffusion/model.py:94-98
//   repaint_mix   diffusion/model.py:58-60
//   ddpm_step     diffusion/model.py:101-122 (clip=0), :126-150 (clip=1)
//   ddim_step     diffusion/ddim.py:192-206
//   renoise       (no reference line: the forward move of RePaint resampling)
#include "common.h"
// (clamp_pm1, and the bodies of the split DDPM step further down)
#define DDPM_P0_FN __device__ __host__ __forceinline__
#include "ddpm_p0_body.h"
// (the bodies of the x0 / v prediction kernels at the end of the chain section)
#define PARAM_FN __device__ __host__ __forceinline__
#include "param_body.h"
// (the bodies of the learned-variance prediction and step kernels after them)
#define VAR_FN __device__ __host__ __forceinline__
#include "var_body.h"

// Caller-supplied timesteps index the schedule tables: an index outside [0, T) would read behind them (the reference's gather
// raises there).  Such a sample is computed with index 0 and its whole output is poisoned with NaN -- loud, but memory-safe.
__device__ __forceinline__ long long checked_t(long long tn, int T, bool& bad) {
    bad = tn < 0 || tn >= (long long)T;
    return bad ? 0 : tn;
}
#define EOD_POISON(bad, v) ((bad) ? __builtin_nanf("") : (v))

__device__ __forceinline__ long long tmin_of(const long long* t, int N) {
    long long m = t[0];
    for (int i = 1; i < N; ++i) m = t[i] < m ? t[i] : m;
    return m;
}

// grid (blocks, N): blockIdx.y = sample, so per-sample coefficients are computed once per thread.
__global__ void q_sample_kernel(const float* __restrict__ x0, const float* __restrict__ noise, const long long* __restrict__ t,
                                const float* __restrict__ sa, const float* __restrict__ sb, float* __restrict__ out, long long chw, int T) {
    const int n = blockIdx.y;
    bool bad;
    const long long tn = checked_t(t[n], T, bad);
    const float a = sa[tn], b = sb[tn];
    const long long base = (long long)n * chw;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < chw; i += (long long)gridDim.x * blockDim.x) {
        const float p = a * x0[base + i];
        const float q = b * noise[base + i];
        out[base + i] = EOD_POISON(bad, p + q);
    }
}

__global__ void repaint_mix_kernel(const float* __restrict__ x_t, const float* __restrict__ gt, const float* __restrict__ mask,
                                   const float* __restrict__ noise, const long long* __restrict__ t, const float* __restrict__ sa,
                                   const float* __restrict__ sb, float* __restrict__ out, int C, long long hw, int T) {
    const int n = blockIdx.y;
    bool bad;
    const long long tn = checked_t(t[n], T, bad);
    const float a = sa[tn], b = sb[tn];
    const long long chw = (long long)C * hw, base = (long long)n * chw;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < chw; i += (long long)gridDim.x * blockDim.x) {
        const float m = mask[(long long)n * hw + (i % hw)];
        const float p = a * gt[base + i];
        const float q = b * noise[base + i];
        const float gn = p + q;              // gt_noised = _forward_diffusion(gt, t, noise)
        const float l = m * gn;              // mask*gt_noised
        const float om = 1.0f - m;           // (1-mask)
        const float r = om * x_t[base + i];  // (1-mask)*x_t
        out[base + i] = EOD_POISON(bad, l + r);
    }
}

template <bool CLIP>
__global__ void ddpm_step_kernel(const float* __restrict__ x_t, const float* __restrict__ pred, const float* __restrict__ noise,
                                 const long long* __restrict__ t, const float* __restrict__ betas, const float* __restrict__ alphas,
                                 const float* __restrict__ acp, const float* __restrict__ s1m, float* __restrict__ out, int N,
                                 long long chw, int T) {
    const int n = blockIdx.y;
    bool bad;
    const long long tn = checked_t(t[n], T, bad);
    const bool all_pos = tmin_of(t, N) > 0;  // the reference branches on the BATCH minimum (model.py:113,140)
    const float alpha_t = alphas[tn], acp_t = acp[tn], beta_t = betas[tn];
    float c_x0 = 0.f, c_pred = 0.f, m_x0 = 0.f, m_xt = 0.f, std = 0.0f, k_mean = 0.f, k_pred = 0.f;
    if (CLIP) {
        c_x0 = sqrtf(1.0f / acp_t);           // torch.sqrt(1. / alpha_t_cumprod)
        c_pred = sqrtf(1.0f / acp_t - 1.0f);  // torch.sqrt(1. / alpha_t_cumprod - 1.)
        if (all_pos) {
            const float acp_prev = acp[tn > 0 ? tn - 1 : 0];  // (tn == 0 here: a sample out of range, whose output is NaN)
            m_x0 = beta_t * sqrtf(acp_prev) / (1.0f - acp_t);
            m_xt = (1.0f - acp_prev) * sqrtf(alpha_t) / (1.0f - acp_t);
            std = sqrtf(beta_t * (1.0f - acp_prev) / (1.0f - acp_t));
        } else {
            m_x0 = beta_t / (1.0f - acp_t);
        }
    } else {
        k_mean = 1.0f / sqrtf(alpha_t);          // (1./torch.sqrt(alpha_t))
        k_pred = (1.0f - alpha_t) / s1m[tn];     // ((1.0-alpha_t)/sqrt_one_minus_alpha_cumprod_t)
        if (all_pos) {
            const float acp_prev = acp[tn > 0 ? tn - 1 : 0];  // (tn == 0 here: a sample out of range, whose output is NaN)
            std = sqrtf(beta_t * (1.0f - acp_prev) / (1.0f - acp_t));
        }
    }
    const long long base = (long long)n * chw;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < chw; i += (long long)gridDim.x * blockDim.x) {
        const float x = x_t[base + i], e = pred[base + i], z = noise[base + i];
        float mean;
        if (CLIP) {
            const float u = c_x0 * x;
            const float v = c_pred * e;
            float x0 = u - v;
            x0 = clamp_pm1(x0);              // x0.clamp(-1, 1): a NaN stays NaN
            if (all_pos) {
                const float p = m_x0 * x0;
                const float q = m_xt * x;
                mean = p + q;
            } else {
                mean = m_x0 * x0;
            }
        } else {
            const float v = k_pred * e;
            const float d = x - v;
            mean = k_mean * d;
        }
        const float sz = std * z;
        out[base + i] = EOD_POISON(bad, mean + sz);
    }
}

__global__ void ddim_step_kernel(const float* __restrict__ x, const float* __restrict__ e_t, const float* __restrict__ noise,
                                 float a_t, float a_prev, float sigma_t, float s1m_at, float temperature,
                                 float* __restrict__ x_prev, float* __restrict__ pred_x0, long long numel) {
    const float sq_at = sqrtf(a_t);
    const float sig2 = sigma_t * sigma_t;                // sigma_t**2
    const float dcoef = sqrtf((1.0f - a_prev) - sig2);   // (1. - a_prev - sigma_t**2).sqrt()
    const float sq_ap = sqrtf(a_prev);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < numel; i += (long long)gridDim.x * blockDim.x) {
        const float xv = x[i], e = e_t[i];
        const float se = s1m_at * e;
        const float p0 = (xv - se) / sq_at;              // pred_x0
        const float dir = dcoef * e;                     // dir_xt
        float nz = 0.0f;
        if (noise) {
            const float sn = sigma_t * noise[i];
            nz = sn * temperature;                       // sigma_t * noise * temperature
        } else {
            nz = (sigma_t * 0.0f) * temperature;
        }
        const float a = sq_ap * p0;
        const float b = a + dir;
        x_prev[i] = b + nz;
        if (pred_x0) pred_x0[i] = p0;
    }
}

// classifier-free guidance (ddim.py:177-181): e = e_uncond + scale * (e_cond - e_uncond)
__global__ void cfg_combine_kernel(const float* __restrict__ eu, const float* __restrict__ ec, float scale, float* __restrict__ out,
                                   long long numel) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < numel; i += (long long)gridDim.x * blockDim.x) {
        const float d = ec[i] - eu[i];
        const float m = scale * d;
        out[i] = eu[i] + m;
    }
}

// table-driven DDPM step of the LDM-derived sampler (ddpm.py:221-255): predict_start_from_noise, clamp, q_posterior,
// noise scaled by exp(0.5 * posterior_log_variance_clipped) and masked out at t == 0 (per sample, not per batch).
template <bool CLIP>
__global__ void ldm_p_sample_kernel(const float* __restrict__ x, const float* __restrict__ eps, const float* __restrict__ noise,
                                    const long long* __restrict__ t, const float* __restrict__ sr, const float* __restrict__ srm1,
                                    const float* __restrict__ c1, const float* __restrict__ c2, const float* __restrict__ lv,
                                    float* __restrict__ out, long long chw, int T) {
    const int n = blockIdx.y;
    bool bad;
    const long long tn = checked_t(t[n], T, bad);
    const float a = sr[tn], b = srm1[tn], k1 = c1[tn], k2 = c2[tn];
    const float nonzero = 1.0f - (tn == 0 ? 1.0f : 0.0f);
    const float sd = expf(0.5f * lv[tn]);
    const float ns = nonzero * sd;
    const long long base = (long long)n * chw;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < chw; i += (long long)gridDim.x * blockDim.x) {
        const float xv = x[base + i];
        const float u = a * xv;
        const float v = b * eps[base + i];
        float x0 = u - v;
        if (CLIP) x0 = clamp_pm1(x0);
        const float p = k1 * x0;
        const float q = k2 * xv;
        const float mean = p + q;
        const float z = ns * noise[base + i];
        out[base + i] = EOD_POISON(bad, mean + z);
    }
}

static inline unsigned blocks_for(long long n, int cap) {
    long long b = (n + 255) / 256;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (unsigned)b;
}

extern "C" int eod_q_sample(const float* x0, const float* noise, const int64_t* t, const float* sqrt_acp, const float* sqrt_1m_acp,
                            float* out, int N, int64_t chw, int T, void* stream) {
    EOD_REQUIRE(x0 && noise && t && sqrt_acp && sqrt_1m_acp && out && N > 0 && chw > 0 && T > 0, "q_sample: bad args");
    hipLaunchKernelGGL(q_sample_kernel, dim3(blocks_for(chw, 512), N), dim3(256), 0, (hipStream_t)stream, x0, noise, (const long long*)t, sqrt_acp, sqrt_1m_acp, out, (long long)chw, T);
    EOD_CHECK_LAUNCH("q_sample");
    return EOD_OK;
}

extern "C" int eod_repaint_mix(const float* x_t, const float* gt, const float* mask, const float* noise, const int64_t* t,
                               const float* sqrt_acp, const float* sqrt_1m_acp, float* out, int N, int C, int64_t hw, int T,
                               void* stream) {
    EOD_REQUIRE(x_t && gt && mask && noise && t && sqrt_acp && sqrt_1m_acp && out && N > 0 && C > 0 && hw > 0 && T > 0, "repaint_mix: bad args");
    hipLaunchKernelGGL(repaint_mix_kernel, dim3(blocks_for((long long)C * hw, 512), N), dim3(256), 0, (hipStream_t)stream, x_t, gt, mask, noise, (const long long*)t, sqrt_acp, sqrt_1m_acp, out, C, (long long)hw, T);
    EOD_CHECK_LAUNCH("repaint_mix");
    return EOD_OK;
}

extern "C" int eod_ddpm_step(const float* x_t, const float* pred, const float* noise, const int64_t* t, const float* betas,
                             const float* alphas, const float* acp, const float* sqrt_1m_acp, float* out, int N, int64_t chw, int T,
                             int clip, void* stream) {
    EOD_REQUIRE(x_t && pred && noise && t && betas && alphas && acp && sqrt_1m_acp && out && N > 0 && chw > 0 && T > 0, "ddpm_step: bad args");
    dim3 grid(blocks_for(chw, 512), N);
    if (clip)
        hipLaunchKernelGGL(ddpm_step_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x_t, pred, noise, (const long long*)t, betas, alphas, acp, sqrt_1m_acp, out, N, (long long)chw, T);
    else
        hipLaunchKernelGGL(ddpm_step_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x_t, pred, noise, (const long long*)t, betas, alphas, acp, sqrt_1m_acp, out, N, (long long)chw, T);
    EOD_CHECK_LAUNCH("ddpm_step");
    return EOD_OK;
}

extern "C" int eod_ddim_step(const float* x, const float* e_t, const float* noise, float a_t, float a_prev, float sigma_t,
                             float sqrt_1m_at, float temperature, float* x_prev, float* pred_x0, int64_t numel, void* stream) {
    EOD_REQUIRE(x && e_t && x_prev && numel > 0, "ddim_step: bad args");
    hipLaunchKernelGGL(ddim_step_kernel, dim3(blocks_for(numel, 4096)), dim3(256), 0, (hipStream_t)stream, x, e_t, noise, a_t, a_prev, sigma_t, sqrt_1m_at, temperature, x_prev, pred_x0, (long long)numel);
    EOD_CHECK_LAUNCH("ddim_step");
    return EOD_OK;
}

// ---------------------------------------------------------------------------------------------
// k15: Philox4x32-10 + Box-Muller.  counter = (element_index/4, global sample index, step, stream_id),
// key = seed.  Each thread produces 4 normals (one 16-byte store).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void philox_round(unsigned& c0, unsigned& c1, unsigned& c2, unsigned& c3, unsigned k0, unsigned k1) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0;
    const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0;
    const unsigned n1 = (unsigned)p1;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    const unsigned n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
}

__device__ __forceinline__ float u01(unsigned u) { return ((float)(u >> 8) + 0.5f) * (1.0f / 16777216.0f); }

// the four normals of quad `qd` (elements 4 qd .. 4 qd + 3) of sample `sample` for the key (seed, step, stream_id): the ONE statement of
// the generator, shared by randn_philox_kernel and the in-register form of renoise_kernel so that both yield the same bits
__device__ __forceinline__ void philox_normal4(long long qd, unsigned long long seed, long long sample, int step, int stream_id, float z[4]) {
    unsigned c0 = (unsigned)qd, c1 = (unsigned)sample, c2 = (unsigned)step, c3 = (unsigned)stream_id ^ (unsigned)(qd >> 32);
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c0, c1, c2, c3, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    const float r0 = sqrtf(-2.0f * logf(u01(c0))), r1 = sqrtf(-2.0f * logf(u01(c2)));
    const float a0 = 6.28318530717958647692f * u01(c1), a1 = 6.28318530717958647692f * u01(c3);
    z[0] = r0 * cosf(a0);
    z[1] = r0 * sinf(a0);
    z[2] = r1 * cosf(a1);
    z[3] = r1 * sinf(a1);
}

__global__ void randn_philox_kernel(float* __restrict__ out, long long chw, unsigned long long seed, long long sample0, int step,
                                    int stream_id) {
    const int n = blockIdx.y;
    const long long quads = (chw + 3) / 4;
    float* o = out + (long long)n * chw;
    for (long long qd = (long long)blockIdx.x * blockDim.x + threadIdx.x; qd < quads; qd += (long long)gridDim.x * blockDim.x) {
        float z[4];
        philox_normal4(qd, seed, sample0 + n, step, stream_id, z);
        const long long e = qd * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (e + j < chw) o[e + j] = z[j];
    }
}

// ---------------------------------------------------------------------------------------------
// RePaint resampling: the forward move x_a -> x_b (b > a) between two levels of a chain, q(x_b | x_a) collapsed over the b - a single
// steps: out = sqrt(r) * x + sqrt(1 - r) * z, r = acp_b / acp_a.  All samples of a call share the level (scalars by value, like
// ddim_step).  GEN: z is generated in registers (philox_normal4, the bits eod_randn_philox would write for the same key) and never
// passes through HBM; otherwise it is read from `noise`.  VEC: one 16-byte access per tensor and quad (chw % 4 == 0, aligned
// pointers); the scalar form does the same arithmetic element by element.
// ---------------------------------------------------------------------------------------------
template <bool VEC, bool GEN>
__global__ void renoise_kernel(const float* __restrict__ x, const float* __restrict__ noise, float acp_from, float acp_to,
                               float* __restrict__ out, long long chw, unsigned long long seed, long long sample0, int step,
                               int stream_id) {
    const int n = blockIdx.y;
    const float r = acp_to / acp_from;
    const float ca = sqrtf(r);
    const float cb = sqrtf(1.0f - r);
    const long long quads = (chw + 3) / 4, base = (long long)n * chw;
    for (long long qd = (long long)blockIdx.x * blockDim.x + threadIdx.x; qd < quads; qd += (long long)gridDim.x * blockDim.x) {
        const long long e = base + qd * 4;
        float z[4];
        if (GEN) philox_normal4(qd, seed, sample0 + n, step, stream_id, z);
        if (VEC) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(x + e);
            if (!GEN) {
                const f32x4 zv = *reinterpret_cast<const f32x4*>(noise + e);
                z[0] = zv[0]; z[1] = zv[1]; z[2] = zv[2]; z[3] = zv[3];
            }
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float p = ca * xv[j];
                const float q = cb * z[j];
                o[j] = p + q;
            }
            *reinterpret_cast<f32x4*>(out + e) = o;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (qd * 4 + j < chw) {
                    const float p = ca * x[e + j];
                    const float q = cb * (GEN ? z[j] : noise[e + j]);
                    out[e + j] = p + q;
                }
            }
        }
    }
}

extern "C" int eod_randn_philox(float* out, int N, int64_t chw, uint64_t seed, int64_t sample0, int32_t step, int32_t stream_id,
                                void* stream) {
    EOD_REQUIRE(out && N > 0 && chw > 0, "randn_philox: bad args");
    hipLaunchKernelGGL(randn_philox_kernel, dim3(blocks_for((chw + 3) / 4, 512), N), dim3(256), 0, (hipStream_t)stream, out, (long long)chw, (unsigned long long)seed, (long long)sample0, step, stream_id);
    EOD_CHECK_LAUNCH("randn_philox");
    return EOD_OK;
}

extern "C" int eod_renoise(const float* x, const float* noise, float acp_from, float acp_to, float* out, int N, int64_t chw, uint64_t seed,
                           int64_t sample0, int32_t step, int32_t stream_id, void* stream) {
    EOD_REQUIRE(x && out && N > 0 && chw > 0, "renoise: bad args");
    EOD_REQUIRE(acp_to > 0.0f && acp_to <= acp_from, "renoise: needs 0 < acp_to <= acp_from (a move UP the chain), got %g -> %g", (double)acp_from, (double)acp_to);
    const bool vec = chw % 4 == 0 && eod_aligned16(x) && eod_aligned16(out) && (!noise || eod_aligned16(noise));
    const dim3 grid(blocks_for((chw + 3) / 4, 512), N), block(256);
#define EOD_RENOISE(V, G)                                                                                                             \
    hipLaunchKernelGGL((renoise_kernel<V, G>), grid, block, 0, (hipStream_t)stream, x, noise, acp_from, acp_to, out, (long long)chw, \
                       (unsigned long long)seed, (long long)sample0, step, stream_id)
    if (noise) {
        if (vec) EOD_RENOISE(true, false); else EOD_RENOISE(false, false);
    } else {
        if (vec) EOD_RENOISE(true, true); else EOD_RENOISE(false, true);
    }
#undef EOD_RENOISE
    EOD_CHECK_LAUNCH("renoise");
    return EOD_OK;
}

// ---------------------------------------------------------------------------------------------
// DPM-Solver++ (2M), one step of the data-prediction multistep solver (no reference line):
//   se = s1m_as * e;  p0 = (x - se) / sqrtf(a_s)          -- ddim_step_kernel's very operations: the same pred_x0 bits
//   [CLIP] p0 = clamp_pm1(p0)                            -- ddpm_step_kernel<true>'s clamp, torch.clamp(p0, -1, 1) (a NaN stays NaN)
//   D = SECOND ? (w_cur * p0) + (w_prev * d_prev) : p0
//   x_next = (c_x * x) + (c_d * D);  pred_x0 = p0
// every operation rounded once (-ffp-contract=off).  The level is shared by all samples: scalars by value, computed on the host in
// float64 (diffusion/util.py dpm_coefficients).  VEC: one 16-byte access per tensor and quad; the scalar form does the same arithmetic.
// ---------------------------------------------------------------------------------------------
template <bool CLIP, bool SECOND>
__device__ __forceinline__ void dpmpp_one(float xv, float e, float d, float sq_as, float s1m_as, float c_x, float c_d, float w_cur,
                                          float w_prev, float& xn, float& p0) {
    const float se = s1m_as * e;
    p0 = (xv - se) / sq_as;
    if (CLIP) p0 = clamp_pm1(p0);
    float D = p0;
    if (SECOND) {
        const float u = w_cur * p0;
        const float v = w_prev * d;
        D = u + v;
    }
    const float p = c_x * xv;
    const float q = c_d * D;
    xn = p + q;
}

template <bool VEC, bool CLIP, bool SECOND>
__global__ void dpmpp_step_kernel(const float* __restrict__ x, const float* __restrict__ e_t, const float* __restrict__ d_prev, float a_s,
                                  float s1m_as, float c_x, float c_d, float w_cur, float w_prev, float* __restrict__ x_next,
                                  float* __restrict__ pred_x0, long long numel) {
    const float sq_as = sqrtf(a_s);
    const long long quads = (numel + 3) / 4;
    for (long long qd = (long long)blockIdx.x * blockDim.x + threadIdx.x; qd < quads; qd += (long long)gridDim.x * blockDim.x) {
        const long long i0 = qd * 4;
        if (VEC) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(x + i0);
            const f32x4 ev = *reinterpret_cast<const f32x4*>(e_t + i0);
            f32x4 dv = {0.0f, 0.0f, 0.0f, 0.0f};
            if (SECOND) dv = *reinterpret_cast<const f32x4*>(d_prev + i0);
            f32x4 xn, p0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float a, b;
                dpmpp_one<CLIP, SECOND>(xv[j], ev[j], dv[j], sq_as, s1m_as, c_x, c_d, w_cur, w_prev, a, b);
                xn[j] = a;
                p0[j] = b;
            }
            *reinterpret_cast<f32x4*>(x_next + i0) = xn;
            *reinterpret_cast<f32x4*>(pred_x0 + i0) = p0;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (i0 + j < numel) {
                    float a, b;
                    dpmpp_one<CLIP, SECOND>(x[i0 + j], e_t[i0 + j], SECOND ? d_prev[i0 + j] : 0.0f, sq_as, s1m_as, c_x, c_d, w_cur, w_prev, a, b);
                    x_next[i0 + j] = a;
                    pred_x0[i0 + j] = b;
                }
            }
        }
    }
}

static inline bool eod_overlap(const float* a, const float* b, long long n) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b, bytes = (uintptr_t)n * sizeof(float);
    return pa < pb + bytes && pb < pa + bytes;
}

extern "C" int eod_dpmpp_step(const float* x, const float* e_t, const float* d_prev, float a_s, float sqrt_1m_as, float c_x, float c_d,
                              float w_cur, float w_prev, int clip, float* x_next, float* pred_x0, int64_t numel, void* stream) {
    EOD_REQUIRE(x && e_t && x_next && pred_x0 && numel > 0, "dpmpp_step: bad args");
    EOD_REQUIRE(a_s > 0.0f && a_s <= 1.0f, "dpmpp_step: needs 0 < a_s <= 1, got %g", (double)a_s);
    EOD_REQUIRE(!eod_overlap(x_next, pred_x0, numel), "dpmpp_step: x_next and pred_x0 overlap");
    EOD_REQUIRE(!d_prev || (!eod_overlap(x_next, d_prev, numel) && !eod_overlap(pred_x0, d_prev, numel)),
                "dpmpp_step: x_next / pred_x0 must not alias d_prev (the history is read while they are written)");
    const bool vec = numel % 4 == 0 && eod_aligned16(x) && eod_aligned16(e_t) && eod_aligned16(x_next) && eod_aligned16(pred_x0) &&
                     (!d_prev || eod_aligned16(d_prev));
    const dim3 grid(blocks_for((numel + 3) / 4, 2048)), block(256);
#define EOD_DPMPP(V, C, S)                                                                                                              \
    hipLaunchKernelGGL((dpmpp_step_kernel<V, C, S>), grid, block, 0, (hipStream_t)stream, x, e_t, d_prev, a_s, sqrt_1m_as, c_x, c_d, \
                       w_cur, w_prev, x_next, pred_x0, (long long)numel)
#define EOD_DPMPP_CS(V)                                           \
    do {                                                          \
        if (clip) {                                               \
            if (d_prev) EOD_DPMPP(V, true, true); else EOD_DPMPP(V, true, false);   \
        } else {                                                  \
            if (d_prev) EOD_DPMPP(V, false, true); else EOD_DPMPP(V, false, false); \
        }                                                         \
    } while (0)
    if (vec) EOD_DPMPP_CS(true); else EOD_DPMPP_CS(false);
#undef EOD_DPMPP_CS
#undef EOD_DPMPP
    EOD_CHECK_LAUNCH("dpmpp_step");
    return EOD_OK;
}

// ---------------------------------------------------------------------------------------------
// Observation consistency (no reference line): the data prediction of a DDIM / DPM-Solver++ step is moved towards
// an observation of per-channel block means before the update uses it.  blk(i) = the f_c x f_c block of pixel i, anchored at the plane's
// origin; per pixel, every operation rounded once (-ffp-contract=off):
//   s     = p0 of the block's first pixel; then + p0 of every other pixel of the block, row by row, left to right (sequential fp32 adds)
//   mean  = s / float(f_c * f_c)
//   lm    = lambda * m                       (mask NULL: m = 1.0f)
//   p0c   = p0 - (lm * (mean - values))
// One thread owns one block and keeps its f^2 predictions (and the e_t / x the update needs) in registers; the lanes of a wave take
// neighbouring blocks of a block-row, so a wave reads 64 f contiguous floats per image row.  One launch per factor that occurs among the
// channels (registers sized to that factor), grid.y = (sample, channel with that factor).  VEC: 16-byte (f = 4, 8; quads of f = 1) or
// 8-byte (f = 2, 6) accesses; otherwise, and always for odd f, element by element: same arithmetic, same order.  The order of the block
// sum is a property of the block alone: it does not depend on B, on the launch geometry, on alignment, or on what the plane belongs to.
// ---------------------------------------------------------------------------------------------
typedef float f32x2 __attribute__((ext_vector_type(2)));
enum { OBS_DDIM = 0, OBS_DPMPP = 1, OBS_MEAN = 2, OBS_PROJECT = 3, OBS_APPLY = 4 };   // PROJECT: the projection of a given p; APPLY: spec_kernel's
#define OBS_STEP(KIND) ((KIND) == OBS_DDIM || (KIND) == OBS_DPMPP)                       // the kinds that form p0 from (x, e_t) and finish a step

struct ObsArgs {
    const float *x, *e, *noise, *d_prev, *values, *mask;
    float *out0, *out1;                // x_prev / x_next / the block means;  pred_x0
    float a, s1m, lambda;              // a_t (a_s), sqrt(1 - a), the weight
    float k0, k1, k2, k3;              // DDIM: a_prev, sigma_t, temperature, -;  DPM-Solver++: c_x, c_d, w_cur, w_prev
    int clip, B, C, H, W;
    int values_b1, mask_b1, mask_c1;   // broadcast: values [1, C, H, W]; mask [1, ., H, W]; mask [., 1, H, W]
};
struct ObsChannels {
    unsigned char c[32];
    int n;
};
struct ObsK {                          // what a step needs per pixel, computed once per thread
    float sq_a, s1m, lambda, u0, u1, u2, u3;
    bool clip, second, noisy;
};

template <int KIND>
__device__ __forceinline__ ObsK obs_scalars(const ObsArgs& g) {
    ObsK k;
    k.s1m = g.s1m; k.lambda = g.lambda; k.clip = g.clip != 0; k.second = g.d_prev != nullptr; k.noisy = g.noise != nullptr;
    k.sq_a = OBS_STEP(KIND) ? sqrtf(g.a) : 1.0f;
    k.u0 = g.k0; k.u1 = g.k1; k.u2 = g.k2; k.u3 = g.k3;
    if (KIND == OBS_DDIM) {            // ddim_step_kernel's scalars
        const float sig2 = g.k1 * g.k1;
        k.u0 = sqrtf((1.0f - g.k0) - sig2);   // dcoef
        k.u3 = sqrtf(g.k0);                   // sq_ap
    }
    return k;
}

// p0 as ddim_step_kernel / dpmpp_one form it (no step kind: the input itself)
template <int KIND>
__device__ __forceinline__ float obs_p0(float xv, float e, const ObsK& k) {
    if (!OBS_STEP(KIND)) return xv;
    const float se = k.s1m * e;
    float p0 = (xv - se) / k.sq_a;
    if (KIND == OBS_DPMPP && k.clip) p0 = clamp_pm1(p0);
    return p0;
}

// the update of one pixel from its projected prediction; aux = e_t (DDIM: the direction) or x (DPM-Solver++: the state term)
template <int KIND>
__device__ __forceinline__ void obs_update(float p0c, float aux, float z, float d, const ObsK& k, float& o0, float& o1) {
    if (KIND == OBS_DDIM) {
        const float dir = k.u0 * aux;
        float nz;
        if (k.noisy) {
            const float sn = k.u1 * z;
            nz = sn * k.u2;
        } else {
            nz = (k.u1 * 0.0f) * k.u2;
        }
        const float a = k.u3 * p0c;
        const float b = a + dir;
        o0 = b + nz;
    } else {
        float D = p0c;
        if (k.second) {
            const float u = k.u2 * p0c;
            const float w = k.u3 * d;
            D = u + w;
        }
        const float p = k.u0 * aux;
        const float q = k.u1 * D;
        o0 = p + q;
    }
    o1 = p0c;
}

// the projection and the update of one pixel (OBS_PROJECT: the projection alone)
template <int KIND>
__device__ __forceinline__ void obs_finish(float p0, float aux, float mean, float v, float m, float z, float d, const ObsK& k, float& o0,
                                           float& o1) {
    if (KIND == OBS_MEAN) { o0 = mean; o1 = 0.0f; return; }
    const float lm = k.lambda * m;
    const float df = mean - v;
    const float t = lm * df;
    const float p0c = p0 - t;
    if (KIND == OBS_PROJECT) { o0 = p0c; o1 = 0.0f; return; }
    obs_update<KIND>(p0c, aux, z, d, k, o0, o1);
}

template <int F, bool VEC> struct obs_width { static constexpr int v = !VEC || (F & 1) ? 1 : (F % 4 == 0 ? 4 : 2); };

template <int N, int V>
__device__ __forceinline__ void obs_load(const float* p, float* r) {
#pragma unroll
    for (int j = 0; j < N; j += V) {
        if (V == 4) { const f32x4 t = *reinterpret_cast<const f32x4*>(p + j); r[j] = t[0]; r[j + 1] = t[1]; r[j + 2] = t[2]; r[j + 3] = t[3]; }
        else if (V == 2) { const f32x2 t = *reinterpret_cast<const f32x2*>(p + j); r[j] = t[0]; r[j + 1] = t[1]; }
        else r[j] = p[j];
    }
}
template <int N, int V>
__device__ __forceinline__ void obs_store(float* p, const float* r) {
#pragma unroll
    for (int j = 0; j < N; j += V) {
        if (V == 4) { f32x4 t = {r[j], r[j + 1], r[j + 2], r[j + 3]}; *reinterpret_cast<f32x4*>(p + j) = t; }
        else if (V == 2) { f32x2 t = {r[j], r[j + 1]}; *reinterpret_cast<f32x2*>(p + j) = t; }
        else p[j] = r[j];
    }
}

template <int KIND, int F, bool VEC>
__global__ void __launch_bounds__(256) obs_kernel(ObsArgs g, ObsChannels ch) {
    const int b = blockIdx.y / ch.n, c = ch.c[blockIdx.y % ch.n];
    const long long hw = (long long)g.H * g.W;
    const long long off = ((long long)b * g.C + c) * hw;                                           // x, e_t, noise, d_prev, outputs
    const long long voff = ((long long)(g.values_b1 ? 0 : b) * g.C + c) * hw;
    const long long moff = ((long long)(g.mask_b1 ? 0 : b) * (g.mask_c1 ? 1 : g.C) + (g.mask_c1 ? 0 : c)) * hw;
    const ObsK k = obs_scalars<KIND>(g);
    const bool masked = g.mask != nullptr;
    const long long stride = (long long)gridDim.x * blockDim.x;
    if (F == 1) {
        // f = 1: the mean is p0 / 1.0f.  Quads of the plane; the last one is cut at the plane's end (VEC: hw % 4 == 0, checked by the host)
        const long long quads = (hw + 3) / 4;
        for (long long qd = (long long)blockIdx.x * blockDim.x + threadIdx.x; qd < quads; qd += stride) {
            const long long i0 = qd * 4;
            float xv[4] = {0.f, 0.f, 0.f, 0.f}, ev[4] = {0.f, 0.f, 0.f, 0.f}, vv[4] = {0.f, 0.f, 0.f, 0.f}, mv[4] = {1.0f, 1.0f, 1.0f, 1.0f};
            float zv[4] = {0.f, 0.f, 0.f, 0.f}, dv[4] = {0.f, 0.f, 0.f, 0.f}, o0[4], o1[4];
            if (VEC) {
                obs_load<4, 4>(g.x + off + i0, xv);
                if (KIND != OBS_MEAN) {
                    if (OBS_STEP(KIND)) obs_load<4, 4>(g.e + off + i0, ev);
                    obs_load<4, 4>(g.values + voff + i0, vv);
                    if (masked) obs_load<4, 4>(g.mask + moff + i0, mv);
                    if (KIND == OBS_DDIM && k.noisy) obs_load<4, 4>(g.noise + off + i0, zv);
                    if (KIND == OBS_DPMPP && k.second) obs_load<4, 4>(g.d_prev + off + i0, dv);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (i0 + j < hw) {
                        xv[j] = g.x[off + i0 + j];
                        if (KIND != OBS_MEAN) {
                            if (OBS_STEP(KIND)) ev[j] = g.e[off + i0 + j];
                            vv[j] = g.values[voff + i0 + j];
                            if (masked) mv[j] = g.mask[moff + i0 + j];
                            if (KIND == OBS_DDIM && k.noisy) zv[j] = g.noise[off + i0 + j];
                            if (KIND == OBS_DPMPP && k.second) dv[j] = g.d_prev[off + i0 + j];
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float p0 = obs_p0<KIND>(xv[j], ev[j], k);
                const float mean = p0 / 1.0f;
                obs_finish<KIND>(p0, KIND == OBS_DDIM ? ev[j] : xv[j], mean, vv[j], mv[j], zv[j], dv[j], k, o0[j], o1[j]);
            }
            if (VEC) {
                obs_store<4, 4>(g.out0 + off + i0, o0);
                if (OBS_STEP(KIND)) obs_store<4, 4>(g.out1 + off + i0, o1);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (i0 + j < hw) {
                        g.out0[off + i0 + j] = o0[j];
                        if (OBS_STEP(KIND)) g.out1[off + i0 + j] = o1[j];
                    }
                }
            }
        }
        return;
    }
    constexpr int V = obs_width<F, VEC>::v;
    const int nbx = g.W / F;
    const long long blocks = (long long)nbx * (g.H / F);
    for (long long blk = (long long)blockIdx.x * blockDim.x + threadIdx.x; blk < blocks; blk += stride) {
        const long long by = blk / nbx, bx = blk % nbx;
        const long long at = by * F * g.W + bx * F;       // the block's first pixel in its plane; every row of it lies inside the plane
        float P[F * F], A[OBS_STEP(KIND) ? F * F : 1];
#pragma unroll
        for (int r = 0; r < F; ++r) {
            float xr[F], er[F];
            obs_load<F, V>(g.x + off + at + (long long)r * g.W, xr);
            if (OBS_STEP(KIND)) obs_load<F, V>(g.e + off + at + (long long)r * g.W, er);
#pragma unroll
            for (int j = 0; j < F; ++j) {
                P[r * F + j] = obs_p0<KIND>(xr[j], OBS_STEP(KIND) ? er[j] : 0.0f, k);
                if (OBS_STEP(KIND)) A[r * F + j] = KIND == OBS_DDIM ? er[j] : xr[j];
            }
        }
        float s = P[0];
#pragma unroll
        for (int i = 1; i < F * F; ++i) s = s + P[i];     // row by row, left to right
        const float mean = s / (float)(F * F);
#pragma unroll
        for (int r = 0; r < F; ++r) {
            const long long row = at + (long long)r * g.W;
            float vr[F], mr[F], zr[F], dr[F], o0[F], o1[F];
#pragma unroll
            for (int j = 0; j < F; ++j) { vr[j] = 0.0f; mr[j] = 1.0f; zr[j] = 0.0f; dr[j] = 0.0f; }
            if (KIND != OBS_MEAN) {
                obs_load<F, V>(g.values + voff + row, vr);
                if (masked) obs_load<F, V>(g.mask + moff + row, mr);
                if (KIND == OBS_DDIM && k.noisy) obs_load<F, V>(g.noise + off + row, zr);
                if (KIND == OBS_DPMPP && k.second) obs_load<F, V>(g.d_prev + off + row, dr);
            }
#pragma unroll
            for (int j = 0; j < F; ++j)
                obs_finish<KIND>(P[r * F + j], OBS_STEP(KIND) ? A[r * F + j] : 0.0f, mean, vr[j], mr[j], zr[j], dr[j], k, o0[j], o1[j]);
            obs_store<F, V>(g.out0 + off + row, o0);
            if (OBS_STEP(KIND)) obs_store<F, V>(g.out1 + off + row, o1);
        }
    }
}

static inline bool eod_overlap2(const float* a, long long na, const float* b, long long nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + (uintptr_t)nb * sizeof(float) && pb < pa + (uintptr_t)na * sizeof(float);
}

template <int KIND, int F>
static void obs_launch_f(const ObsArgs& g, const ObsChannels& ch, bool vec, hipStream_t stream) {
    const long long hw = (long long)g.H * g.W;
    const long long units = F == 1 ? (hw + 3) / 4 : hw / (F * F);
    const int planes = g.B * ch.n;
    const dim3 grid(blocks_for(units, planes >= 4096 ? 1 : 4096 / planes), planes), block(256);
    if (vec && (F != 1 || hw % 4 == 0))
        hipLaunchKernelGGL((obs_kernel<KIND, F, true>), grid, block, 0, stream, g, ch);
    else
        hipLaunchKernelGGL((obs_kernel<KIND, F, false>), grid, block, 0, stream, g, ch);
}

// checks what the three entry points share, then one launch per factor that occurs
template <int KIND>
static int obs_launch(const char* what, ObsArgs g, const int32_t* factors, void* stream) {
    EOD_REQUIRE(g.x && g.out0 && factors && g.B > 0 && g.C > 0 && g.H > 0 && g.W > 0, "%s: bad args", what);
    EOD_REQUIRE(g.C <= 32, "%s: at most 32 channels (the factors travel by value), got %d", what, g.C);
    EOD_REQUIRE((long long)g.B * g.C <= 65535, "%s: B * C = %lld planes exceed one launch", what, (long long)g.B * g.C);
    for (int c = 0; c < g.C; ++c) {
        EOD_REQUIRE(factors[c] >= 1 && factors[c] <= 8, "%s: factors[%d] = %d is outside 1..8", what, c, factors[c]);
        EOD_REQUIRE(g.H % factors[c] == 0 && g.W % factors[c] == 0, "%s: factors[%d] = %d does not divide %d x %d", what, c, factors[c], g.H, g.W);
    }
    const long long n = (long long)g.B * g.C * g.H * g.W;
    EOD_REQUIRE(OBS_STEP(KIND) || !eod_overlap2(g.out0, n, g.x, n), "%s: out overlaps %s", what, KIND == OBS_MEAN ? "x" : "p");
    if (KIND != OBS_MEAN) {
        EOD_REQUIRE(g.values && (!OBS_STEP(KIND) || (g.e && g.out1)), "%s: bad args", what);
        EOD_REQUIRE(!OBS_STEP(KIND) || (g.a > 0.0f && g.a <= 1.0f), "%s: needs 0 < a <= 1, got %g", what, (double)g.a);
        EOD_REQUIRE(g.lambda >= 0.0f && g.lambda <= 1.0f, "%s: the weight must lie in [0, 1], got %g", what, (double)g.lambda);
        const long long nv = (long long)(g.values_b1 ? 1 : g.B) * g.C * g.H * g.W;
        const long long nm = (long long)(g.mask_b1 ? 1 : g.B) * (g.mask_c1 ? 1 : g.C) * g.H * g.W;
        EOD_REQUIRE(!g.out1 || !eod_overlap2(g.out0, n, g.out1, n), "%s: the two outputs overlap", what);
        float* const outs[2] = {g.out0, g.out1};
        for (float* o : outs) {
            if (!o) continue;
            EOD_REQUIRE(!eod_overlap2(o, n, g.values, nv), "%s: an output overlaps values", what);
            EOD_REQUIRE(!g.mask || !eod_overlap2(o, n, g.mask, nm), "%s: an output overlaps mask", what);
            EOD_REQUIRE(!g.d_prev || !eod_overlap2(o, n, g.d_prev, n), "%s: an output overlaps d_prev (the history is read while it is written)", what);
        }
    }
    const bool vec = eod_aligned16(g.x) && eod_aligned16(g.out0) && (!g.e || eod_aligned16(g.e)) && (!g.noise || eod_aligned16(g.noise)) &&
                     (!g.d_prev || eod_aligned16(g.d_prev)) && (!g.values || eod_aligned16(g.values)) && (!g.mask || eod_aligned16(g.mask)) &&
                     (!g.out1 || eod_aligned16(g.out1));
    for (int f = 1; f <= 8; ++f) {
        ObsChannels ch;
        ch.n = 0;
        for (int c = 0; c < g.C; ++c)
            if (factors[c] == f) ch.c[ch.n++] = (unsigned char)c;
        if (!ch.n) continue;
        switch (f) {
            case 1: obs_launch_f<KIND, 1>(g, ch, vec, (hipStream_t)stream); break;
            case 2: obs_launch_f<KIND, 2>(g, ch, vec, (hipStream_t)stream); break;
            case 3: obs_launch_f<KIND, 3>(g, ch, vec, (hipStream_t)stream); break;
            case 4: obs_launch_f<KIND, 4>(g, ch, vec, (hipStream_t)stream); break;
            case 5: obs_launch_f<KIND, 5>(g, ch, vec, (hipStream_t)stream); break;
            case 6: obs_launch_f<KIND, 6>(g, ch, vec, (hipStream_t)stream); break;
            case 7: obs_launch_f<KIND, 7>(g, ch, vec, (hipStream_t)stream); break;
            default: obs_launch_f<KIND, 8>(g, ch, vec, (hipStream_t)stream); break;
        }
        EOD_CHECK_LAUNCH(what);
    }
    return EOD_OK;
}

extern "C" int eod_ddim_step_obs(const float* x, const float* e_t, const float* noise, float a_t, float a_prev, float sigma_t,
                                 float sqrt_1m_at, float temperature, const float* values, const float* mask, float lambda,
                                 const int32_t* factors, int B, int C, int H, int W, int values_b1, int mask_b1, int mask_c1, float* x_prev,
                                 float* pred_x0, void* stream) {
    ObsArgs g = {x, e_t, noise, nullptr, values, mask, x_prev, pred_x0, a_t, sqrt_1m_at, lambda, a_prev, sigma_t, temperature, 0.0f,
                 0, B, C, H, W, values_b1, mask_b1, mask_c1};
    return obs_launch<OBS_DDIM>("ddim_step_obs", g, factors, stream);
}

extern "C" int eod_dpmpp_step_obs(const float* x, const float* e_t, const float* d_prev, float a_s, float sqrt_1m_as, float c_x, float c_d,
                                  float w_cur, float w_prev, int clip, const float* values, const float* mask, float lambda,
                                  const int32_t* factors, int B, int C, int H, int W, int values_b1, int mask_b1, int mask_c1, float* x_next,
                                  float* pred_x0, void* stream) {
    ObsArgs g = {x, e_t, nullptr, d_prev, values, mask, x_next, pred_x0, a_s, sqrt_1m_as, lambda, c_x, c_d, w_cur, w_prev,
                 clip, B, C, H, W, values_b1, mask_b1, mask_c1};
    return obs_launch<OBS_DPMPP>("dpmpp_step_obs", g, factors, stream);
}

extern "C" int eod_block_mean(const float* x, const int32_t* factors, float* out, int B, int C, int H, int W, void* stream) {
    ObsArgs g = {x, nullptr, nullptr, nullptr, nullptr, nullptr, out, nullptr, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0, B, C, H, W, 0, 0, 0};
    return obs_launch<OBS_MEAN>("block_mean", g, factors, stream);
}

extern "C" int eod_obs_project(const float* p, const float* values, const float* mask, float lambda, const int32_t* factors, int B, int C,
                               int H, int W, int values_b1, int mask_b1, int mask_c1, float* out, void* stream) {
    ObsArgs g = {p, nullptr, nullptr, nullptr, values, mask, out, nullptr, 1.0f, 0.0f, lambda, 0.0f, 0.0f, 0.0f, 0.0f,
                 0, B, C, H, W, values_b1, mask_b1, mask_c1};
    return obs_launch<OBS_PROJECT>("obs_project", g, factors, stream);
}

// ---------------------------------------------------------------------------------------------
// Cross-band observations (no reference line): A = R (x) D_f, R [K][C] mixing the channels' f x f block means into
// K observed bands, A+ = G (x) replication with G = pinv(R) [C][K].  Per pixel i, every operation rounded once (-ffp-contract=off):
//   mean_c = the block mean of section 9.5 for channel c and blk(i)           (f = 1: p0 / 1.0f)
//   d_k    = R[k][0] * mean_0;  then for c = 1 .. C-1 in order  d_k = d_k + (R[k][c] * mean_c)
//   r_k    = d_k - values_k(i)
//   t_c    = G[c][0] * r_0;     then for k = 1 .. K-1 in order  t_c = t_c + (G[c][k] * r_k)
//   lm     = lambda * m(i)                                                     (mask NULL: m = 1.0f)
//   p0c_c  = p0_c - (lm * t_c)
// One launch, grid.y = sample.  A thread owns one f x f block across all channels (f = 1: a quad of pixels, four blocks).  Pass 1 walks
// the channels, forms p0 and folds each block mean into K running dots (a statically indexed register array; the loop over k is
// unrolled to 8 and guarded by the wave-uniform k < K: no zero padding, a + 0 * r term would turn a non-finite r into NaN and flip the
// sign of a zero).  Pass 2 walks the block's rows: the K residuals of the row's pixels, then per channel the row of x / e_t again (the
// same wave fetched it moments ago), the same p0 bits, t_c, the update.  R and G stay in the kernel arguments: indexed by the
// wave-uniform channel they are scalar loads.  The access widths are obs_kernel's.
// ---------------------------------------------------------------------------------------------
#define EOD_SPEC_MAXK 8
struct SpecMat {
    float R[EOD_SPEC_MAXK][32];
    float G[32][EOD_SPEC_MAXK];
};

// N floats of a row, the first nv of them valid (V > 1: all are); the others keep what r holds
template <int N, int V>
__device__ __forceinline__ void spec_load(const float* p, float* r, int nv) {
    if (V > 1) { obs_load<N, V>(p, r); return; }
#pragma unroll
    for (int j = 0; j < N; ++j)
        if (j < nv) r[j] = p[j];
}
template <int N, int V>
__device__ __forceinline__ void spec_store(float* p, const float* r, int nv) {
    if (V > 1) { obs_store<N, V>(p, r); return; }
#pragma unroll
    for (int j = 0; j < N; ++j)
        if (j < nv) p[j] = r[j];
}

template <int KIND, int F, bool VEC>
__global__ void __launch_bounds__(256) spec_kernel(ObsArgs g, int K, SpecMat m) {
    constexpr bool STEP = OBS_STEP(KIND);
    constexpr int WID = F == 1 ? 4 : F;        // the floats of an image row this thread owns
    constexpr int NB = F == 1 ? 4 : 1;         // the blocks they belong to
    constexpr int V = F == 1 ? (VEC ? 4 : 1) : obs_width<F, VEC>::v;
    const int b = blockIdx.y;
    const long long hw = (long long)g.H * g.W;
    const long long off = (long long)b * g.C * hw;                                  // x, e_t, noise, d_prev, the step's outputs
    const long long voff = (long long)(g.values_b1 ? 0 : b) * K * hw;
    const long long moff = (long long)(g.mask_b1 ? 0 : b) * hw;
    const ObsK k = obs_scalars<KIND>(g);
    const bool masked = g.mask != nullptr;
    const int nbx = g.W / F;
    const long long units = F == 1 ? (hw + 3) / 4 : (long long)nbx * (g.H / F);
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x; u < units; u += stride) {
        long long at;                          // the first pixel in its plane; every row read below lies inside the plane
        int nv = WID;                          // f = 1: the last quad is cut at the plane's end (VEC: hw % 4 == 0, checked by the host)
        if (F == 1) {
            at = u * 4;
            if (!VEC && hw - at < 4) nv = (int)(hw - at);
        } else {
            at = (u / nbx) * F * g.W + (u % nbx) * F;
        }
        float d[EOD_SPEC_MAXK][NB];
#pragma unroll
        for (int kk = 0; kk < EOD_SPEC_MAXK; ++kk)
#pragma unroll
            for (int n = 0; n < NB; ++n) d[kk][n] = 0.0f;
        // pass 1: the block means of every channel, folded into the K dots
        for (int c = 0; c < g.C; ++c) {
            const long long pc = off + (long long)c * hw + at;
            float s[NB];
#pragma unroll
            for (int n = 0; n < NB; ++n) s[n] = 0.0f;
#pragma unroll
            for (int r = 0; r < F; ++r) {
                float xr[WID], er[WID];
#pragma unroll
                for (int j = 0; j < WID; ++j) { xr[j] = 0.0f; er[j] = 0.0f; }
                spec_load<WID, V>(g.x + pc + (long long)r * g.W, xr, nv);
                if (STEP) spec_load<WID, V>(g.e + pc + (long long)r * g.W, er, nv);
#pragma unroll
                for (int j = 0; j < WID; ++j) {
                    const float p0 = obs_p0<KIND>(xr[j], er[j], k);
                    if (F == 1) s[j] = p0;
                    else s[0] = (r == 0 && j == 0) ? p0 : s[0] + p0;      // row by row, left to right
                }
            }
#pragma unroll
            for (int n = 0; n < NB; ++n) {
                const float mean = s[n] / (float)(F * F);
#pragma unroll
                for (int kk = 0; kk < EOD_SPEC_MAXK; ++kk) {
                    if (kk < K) {
                        const float pr = m.R[kk][c] * mean;
                        d[kk][n] = c == 0 ? pr : d[kk][n] + pr;
                    }
                }
            }
        }
        if (KIND == OBS_APPLY) {               // the operator alone: d_k on the full-resolution grid
            const long long ooff = (long long)b * K * hw;
            for (int r = 0; r < F; ++r) {
#pragma unroll
                for (int kk = 0; kk < EOD_SPEC_MAXK; ++kk) {
                    if (kk < K) {
                        float o[WID];
#pragma unroll
                        for (int j = 0; j < WID; ++j) o[j] = d[kk][F == 1 ? j : 0];
                        spec_store<WID, V>(g.out0 + ooff + (long long)kk * hw + at + (long long)r * g.W, o, nv);
                    }
                }
            }
            continue;
        }
        // pass 2: row by row the residuals of the row's pixels, then every channel's projection and update
        for (int r = 0; r < F; ++r) {
            const long long row = at + (long long)r * g.W;
            float rk[EOD_SPEC_MAXK][WID], lm[WID];
#pragma unroll
            for (int kk = 0; kk < EOD_SPEC_MAXK; ++kk) {
                if (kk < K) {
                    float vr[WID];
#pragma unroll
                    for (int j = 0; j < WID; ++j) vr[j] = 0.0f;
                    spec_load<WID, V>(g.values + voff + (long long)kk * hw + row, vr, nv);
#pragma unroll
                    for (int j = 0; j < WID; ++j) rk[kk][j] = d[kk][F == 1 ? j : 0] - vr[j];
                } else {
#pragma unroll
                    for (int j = 0; j < WID; ++j) rk[kk][j] = 0.0f;     // (never read: the sums below are guarded alike)
                }
            }
            {
                float mr[WID];
#pragma unroll
                for (int j = 0; j < WID; ++j) mr[j] = 1.0f;
                if (masked) spec_load<WID, V>(g.mask + moff + row, mr, nv);
#pragma unroll
                for (int j = 0; j < WID; ++j) lm[j] = k.lambda * mr[j];
            }
            for (int c = 0; c < g.C; ++c) {
                const long long pc = off + (long long)c * hw + row;
                float xr[WID], er[WID], zr[WID], dr[WID], o0[WID], o1[WID];
#pragma unroll
                for (int j = 0; j < WID; ++j) { xr[j] = 0.0f; er[j] = 0.0f; zr[j] = 0.0f; dr[j] = 0.0f; }
                spec_load<WID, V>(g.x + pc, xr, nv);
                if (STEP) spec_load<WID, V>(g.e + pc, er, nv);
                if (KIND == OBS_DDIM && k.noisy) spec_load<WID, V>(g.noise + pc, zr, nv);
                if (KIND == OBS_DPMPP && k.second) spec_load<WID, V>(g.d_prev + pc, dr, nv);
#pragma unroll
                for (int j = 0; j < WID; ++j) {
                    const float p0 = obs_p0<KIND>(xr[j], er[j], k);
                    float t = m.G[c][0] * rk[0][j];
#pragma unroll
                    for (int kk = 1; kk < EOD_SPEC_MAXK; ++kk) {
                        if (kk < K) {
                            const float pr = m.G[c][kk] * rk[kk][j];
                            t = t + pr;
                        }
                    }
                    const float q = lm[j] * t;
                    const float p0c = p0 - q;
                    if (STEP) obs_update<KIND>(p0c, KIND == OBS_DDIM ? er[j] : xr[j], zr[j], dr[j], k, o0[j], o1[j]);
                    else o0[j] = p0c;
                }
                spec_store<WID, V>(g.out0 + pc, o0, nv);
                if (STEP) spec_store<WID, V>(g.out1 + pc, o1, nv);
            }
        }
    }
}

// the blocks of 256 threads of one spec_kernel launch, over all samples (EOD_SPEC_GRID_BLOCKS of include/eodiff.h): beyond it the
// threads stride over the plane
template <int KIND, int F>
static void spec_launch_f(const ObsArgs& g, int K, const SpecMat& m, bool vec, hipStream_t stream) {
    const long long hw = (long long)g.H * g.W;
    const long long units = F == 1 ? (hw + 3) / 4 : hw / (F * F);
    const dim3 grid(blocks_for(units, g.B >= EOD_SPEC_GRID_BLOCKS ? 1 : EOD_SPEC_GRID_BLOCKS / g.B), g.B), block(256);
    if (vec && (F != 1 || hw % 4 == 0))
        hipLaunchKernelGGL((spec_kernel<KIND, F, true>), grid, block, 0, stream, g, K, m);
    else
        hipLaunchKernelGGL((spec_kernel<KIND, F, false>), grid, block, 0, stream, g, K, m);
}

// checks what the four cross-band entry points share, then the one launch.  OBS_APPLY: out0 is [B][K][H][W] and G is not read.
template <int KIND>
static int spec_launch(const char* what, ObsArgs g, const float* R, const float* G, int K, int f, void* stream) {
    EOD_REQUIRE(g.x && g.out0 && R && g.B > 0 && g.C > 0 && g.H > 0 && g.W > 0, "%s: bad args", what);
    EOD_REQUIRE(g.C <= 32, "%s: at most 32 channels (the matrices travel by value), got %d", what, g.C);
    EOD_REQUIRE(K >= 1 && K <= EOD_SPEC_MAXK && K <= g.C, "%s: needs 1 <= K <= min(C, %d), got K = %d, C = %d", what, EOD_SPEC_MAXK, K, g.C);
    EOD_REQUIRE(g.B <= 65535, "%s: B = %d samples exceed one launch", what, g.B);
    EOD_REQUIRE(f >= 1 && f <= 8, "%s: f = %d is outside 1..8", what, f);
    EOD_REQUIRE(g.H % f == 0 && g.W % f == 0, "%s: f = %d does not divide %d x %d", what, f, g.H, g.W);
    const long long hw = (long long)g.H * g.W, n = (long long)g.B * g.C * hw;
    const long long n0 = KIND == OBS_APPLY ? (long long)g.B * K * hw : n;
    EOD_REQUIRE(KIND != OBS_APPLY || !eod_overlap2(g.out0, n0, g.x, n), "%s: out overlaps x", what);
    if (KIND != OBS_APPLY) {
        EOD_REQUIRE(G && g.values && (!OBS_STEP(KIND) || (g.e && g.out1)), "%s: bad args", what);
        EOD_REQUIRE(!OBS_STEP(KIND) || (g.a > 0.0f && g.a <= 1.0f), "%s: needs 0 < a <= 1, got %g", what, (double)g.a);
        EOD_REQUIRE(g.lambda >= 0.0f && g.lambda <= 1.0f, "%s: the weight must lie in [0, 1], got %g", what, (double)g.lambda);
        const long long nv = (long long)(g.values_b1 ? 1 : g.B) * K * hw, nm = (long long)(g.mask_b1 ? 1 : g.B) * hw;
        EOD_REQUIRE(!g.out1 || !eod_overlap2(g.out0, n, g.out1, n), "%s: the two outputs overlap", what);
        float* const outs[2] = {g.out0, g.out1};
        for (float* o : outs) {
            if (!o) continue;
            EOD_REQUIRE(!eod_overlap2(o, n, g.x, n), "%s: an output overlaps %s", what, (KIND == OBS_PROJECT ? "p" : "x"));
            EOD_REQUIRE(!g.e || !eod_overlap2(o, n, g.e, n), "%s: an output overlaps e_t", what);
            EOD_REQUIRE(!g.noise || !eod_overlap2(o, n, g.noise, n), "%s: an output overlaps noise", what);
            EOD_REQUIRE(!g.d_prev || !eod_overlap2(o, n, g.d_prev, n), "%s: an output overlaps d_prev", what);
            EOD_REQUIRE(!eod_overlap2(o, n, g.values, nv), "%s: an output overlaps values", what);
            EOD_REQUIRE(!g.mask || !eod_overlap2(o, n, g.mask, nm), "%s: an output overlaps mask", what);
        }
    }
    SpecMat m;
    memset(&m, 0, sizeof m);
    for (int kk = 0; kk < K; ++kk)
        for (int c = 0; c < g.C; ++c) {
            m.R[kk][c] = R[kk * g.C + c];
            if (KIND != OBS_APPLY) m.G[c][kk] = G[c * K + kk];
        }
    const bool vec = eod_aligned16(g.x) && eod_aligned16(g.out0) && (!g.e || eod_aligned16(g.e)) && (!g.noise || eod_aligned16(g.noise)) &&
                     (!g.d_prev || eod_aligned16(g.d_prev)) && (!g.values || eod_aligned16(g.values)) && (!g.mask || eod_aligned16(g.mask)) &&
                     (!g.out1 || eod_aligned16(g.out1));
    switch (f) {
        case 1: spec_launch_f<KIND, 1>(g, K, m, vec, (hipStream_t)stream); break;
        case 2: spec_launch_f<KIND, 2>(g, K, m, vec, (hipStream_t)stream); break;
        case 3: spec_launch_f<KIND, 3>(g, K, m, vec, (hipStream_t)stream); break;
        case 4: spec_launch_f<KIND, 4>(g, K, m, vec, (hipStream_t)stream); break;
        case 5: spec_launch_f<KIND, 5>(g, K, m, vec, (hipStream_t)stream); break;
        case 6: spec_launch_f<KIND, 6>(g, K, m, vec, (hipStream_t)stream); break;
        case 7: spec_launch_f<KIND, 7>(g, K, m, vec, (hipStream_t)stream); break;
        default: spec_launch_f<KIND, 8>(g, K, m, vec, (hipStream_t)stream); break;
    }
    EOD_CHECK_LAUNCH(what);
    return EOD_OK;
}

extern "C" int eod_ddim_step_spec(const float* x, const float* e_t, const float* noise, float a_t, float a_prev, float sigma_t,
                                  float sqrt_1m_at, float temperature, const float* values, const float* mask, float lambda, const float* R,
                                  const float* G, int K, int f, int B, int C, int H, int W, int values_b1, int mask_b1, float* x_prev,
                                  float* pred_x0, void* stream) {
    ObsArgs g = {x, e_t, noise, nullptr, values, mask, x_prev, pred_x0, a_t, sqrt_1m_at, lambda, a_prev, sigma_t, temperature, 0.0f,
                 0, B, C, H, W, values_b1, mask_b1, 1};
    return spec_launch<OBS_DDIM>("ddim_step_spec", g, R, G, K, f, stream);
}

extern "C" int eod_dpmpp_step_spec(const float* x, const float* e_t, const float* d_prev, float a_s, float sqrt_1m_as, float c_x, float c_d,
                                   float w_cur, float w_prev, int clip, const float* values, const float* mask, float lambda, const float* R,
                                   const float* G, int K, int f, int B, int C, int H, int W, int values_b1, int mask_b1, float* x_next,
                                   float* pred_x0, void* stream) {
    ObsArgs g = {x, e_t, nullptr, d_prev, values, mask, x_next, pred_x0, a_s, sqrt_1m_as, lambda, c_x, c_d, w_cur, w_prev,
                 clip, B, C, H, W, values_b1, mask_b1, 1};
    return spec_launch<OBS_DPMPP>("dpmpp_step_spec", g, R, G, K, f, stream);
}

extern "C" int eod_spec_project(const float* p, const float* values, const float* mask, float lambda, const float* R, const float* G, int K,
                                int f, int B, int C, int H, int W, int values_b1, int mask_b1, float* out, void* stream) {
    ObsArgs g = {p, nullptr, nullptr, nullptr, values, mask, out, nullptr, 1.0f, 0.0f, lambda, 0.0f, 0.0f, 0.0f, 0.0f,
                 0, B, C, H, W, values_b1, mask_b1, 1};
    return spec_launch<OBS_PROJECT>("spec_project", g, R, G, K, f, stream);
}

extern "C" int eod_spec_apply(const float* x, const float* R, int K, int f, float* out, int B, int C, int H, int W, void* stream) {
    ObsArgs g = {x, nullptr, nullptr, nullptr, nullptr, nullptr, out, nullptr, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0, B, C, H, W, 0, 0, 1};
    return spec_launch<OBS_APPLY>("spec_apply", g, R, nullptr, K, f, stream);
}

// ---------------------------------------------------------------------------------------------
// The ends of a chain of observations: the prediction alone (obs_p0's operations), and the update from a given
// projected prediction (obs_update's operations).  pred_x0 -> projections -> step_p0 has the bits of the fused kernels.  Quads of the
// tensor, 16-byte accesses where numel % 4 == 0 and every pointer is aligned, element by element otherwise.
// ---------------------------------------------------------------------------------------------
enum { END_P0 = 0, END_DDIM = 1, END_DPMPP = 2 };

template <int END, bool VEC>
__global__ void __launch_bounds__(256) chain_end_kernel(ObsArgs g, long long numel) {
    constexpr int KIND = END == END_DDIM ? OBS_DDIM : OBS_DPMPP;
    const ObsK k = obs_scalars<KIND>(g);
    const long long quads = (numel + 3) / 4;
    for (long long qd = (long long)blockIdx.x * blockDim.x + threadIdx.x; qd < quads; qd += (long long)gridDim.x * blockDim.x) {
        const long long i0 = qd * 4;
        const int nv = VEC || numel - i0 >= 4 ? 4 : (int)(numel - i0);
        float xv[4] = {0.f, 0.f, 0.f, 0.f}, ev[4] = {0.f, 0.f, 0.f, 0.f}, pv[4] = {0.f, 0.f, 0.f, 0.f}, zv[4] = {0.f, 0.f, 0.f, 0.f};
        float dv[4] = {0.f, 0.f, 0.f, 0.f}, o0[4], o1[4];
        constexpr int V = VEC ? 4 : 1;
        if (END != END_DDIM) spec_load<4, V>(g.x + i0, xv, nv);
        if (END != END_DPMPP) spec_load<4, V>(g.e + i0, ev, nv);
        if (END != END_P0) spec_load<4, V>(g.values + i0, pv, nv);           // (values: the given p0c)
        if (END == END_DDIM && k.noisy) spec_load<4, V>(g.noise + i0, zv, nv);
        if (END == END_DPMPP && k.second) spec_load<4, V>(g.d_prev + i0, dv, nv);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (END == END_P0) o0[j] = obs_p0<OBS_DPMPP>(xv[j], ev[j], k);
            else obs_update<KIND>(pv[j], END == END_DDIM ? ev[j] : xv[j], zv[j], dv[j], k, o0[j], o1[j]);
        }
        spec_store<4, V>(g.out0 + i0, o0, nv);
    }
}

template <int END>
static int chain_end_launch(const char* what, const ObsArgs& g, int64_t numel, void* stream) {
    EOD_REQUIRE(g.out0 && numel > 0, "%s: bad args", what);
    const float* const ins[5] = {g.x, g.e, g.values, g.noise, g.d_prev};
    bool vec = numel % 4 == 0 && eod_aligned16(g.out0);
    for (const float* p : ins) {
        if (!p) continue;
        EOD_REQUIRE(!eod_overlap(g.out0, p, numel), "%s: the output overlaps an input", what);
        vec = vec && eod_aligned16(p);
    }
    const dim3 grid(blocks_for((numel + 3) / 4, 2048)), block(256);
    if (vec) hipLaunchKernelGGL((chain_end_kernel<END, true>), grid, block, 0, (hipStream_t)stream, g, (long long)numel);
    else hipLaunchKernelGGL((chain_end_kernel<END, false>), grid, block, 0, (hipStream_t)stream, g, (long long)numel);
    EOD_CHECK_LAUNCH(what);
    return EOD_OK;
}

extern "C" int eod_pred_x0(const float* x, const float* e_t, float a, float sqrt_1m_a, int clip, float* p0, int64_t numel, void* stream) {
    EOD_REQUIRE(x && e_t, "pred_x0: bad args");
    EOD_REQUIRE(a > 0.0f && a <= 1.0f, "pred_x0: needs 0 < a <= 1, got %g", (double)a);
    ObsArgs g = {x, e_t, nullptr, nullptr, nullptr, nullptr, p0, nullptr, a, sqrt_1m_a, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, clip, 1, 1, 1, 1, 0, 0, 0};
    return chain_end_launch<END_P0>("pred_x0", g, numel, stream);
}

extern "C" int eod_ddim_step_p0(const float* e_t, const float* p0c, const float* noise, float a_prev, float sigma_t, float temperature,
                                float* x_prev, int64_t numel, void* stream) {
    EOD_REQUIRE(e_t && p0c, "ddim_step_p0: bad args");
    ObsArgs g = {nullptr, e_t, noise, nullptr, p0c, nullptr, x_prev, nullptr, 1.0f, 0.0f, 0.0f, a_prev, sigma_t, temperature, 0.0f,
                 0, 1, 1, 1, 1, 0, 0, 0};
    return chain_end_launch<END_DDIM>("ddim_step_p0", g, numel, stream);
}

extern "C" int eod_dpmpp_step_p0(const float* x, const float* p0c, const float* d_prev, float c_x, float c_d, float w_cur, float w_prev,
                                 float* x_next, int64_t numel, void* stream) {
    EOD_REQUIRE(x && p0c, "dpmpp_step_p0: bad args");
    ObsArgs g = {x, nullptr, nullptr, d_prev, p0c, nullptr, x_next, nullptr, 1.0f, 0.0f, 0.0f, c_x, c_d, w_cur, w_prev, 0, 1, 1, 1, 1, 0, 0, 0};
    return chain_end_launch<END_DPMPP>("dpmpp_step_p0", g, numel, stream);
}

// ---------------------------------------------------------------------------------------------
// The clipped DDPM step cut where its data prediction is complete: ddpm_step_kernel<true>'s operations up to x0
// (eod_ddpm_pred_x0) and from x0 on (eod_ddpm_step_p0), so that the links of an observation can project the prediction in between.  The
// bodies are ddpm_p0_body.h (a host program compiles them, too).  grid (blocks, N) as ddpm_step_kernel; quads of a sample, 16-byte
// accesses where chw % 4 == 0 and every pointer is aligned, element by element otherwise.
// ---------------------------------------------------------------------------------------------
template <bool STEP, bool VEC>
__global__ void __launch_bounds__(256) ddpm_p0_kernel(DdpmP0Args g) {
    const long long first = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
    if (STEP) ddpm_step_p0_thread<VEC>(g, blockIdx.y, first, stride);
    else ddpm_pred_x0_thread<VEC>(g, blockIdx.y, first, stride);
}

template <bool STEP>
static int ddpm_p0_launch(const char* what, const DdpmP0Args& g, void* stream) {
    EOD_REQUIRE(g.x && g.t && g.acp && g.out && g.N > 0 && g.chw > 0 && g.T > 0, "%s: bad args", what);
    const long long n = (long long)g.N * g.chw;
    const float* const tensors[4] = {g.x, g.e, g.p0c, g.z};
    const float* const tables[3] = {g.betas, g.alphas, g.acp};
    bool vec = g.chw % 4 == 0 && eod_aligned16(g.out);
    for (const float* p : tensors) {
        if (!p) continue;
        EOD_REQUIRE(!eod_overlap2(g.out, n, p, n), "%s: the output overlaps an input", what);
        vec = vec && eod_aligned16(p);
    }
    for (const float* p : tables) EOD_REQUIRE(!p || !eod_overlap2(g.out, n, p, g.T), "%s: the output overlaps a schedule table", what);
    EOD_REQUIRE(!eod_overlap2(g.out, n, reinterpret_cast<const float*>(g.t), 2LL * g.N), "%s: the output overlaps t", what);
    const dim3 grid(blocks_for((g.chw + 3) / 4, 2048), g.N), block(256);
    if (vec) hipLaunchKernelGGL((ddpm_p0_kernel<STEP, true>), grid, block, 0, (hipStream_t)stream, g);
    else hipLaunchKernelGGL((ddpm_p0_kernel<STEP, false>), grid, block, 0, (hipStream_t)stream, g);
    EOD_CHECK_LAUNCH(what);
    return EOD_OK;
}

extern "C" int eod_ddpm_pred_x0(const float* x_t, const float* pred, const int64_t* t, const float* acp, float* p0, int N, int64_t chw, int T,
                                int clip, void* stream) {
    EOD_REQUIRE(pred, "ddpm_pred_x0: bad args");
    DdpmP0Args g = {x_t, pred, nullptr, nullptr, (const long long*)t, nullptr, nullptr, acp, p0, N, (long long)chw, T, clip};
    return ddpm_p0_launch<false>("ddpm_pred_x0", g, stream);
}

extern "C" int eod_ddpm_step_p0(const float* x_t, const float* p0c, const float* noise, const int64_t* t, const float* betas,
                                const float* alphas, const float* acp, float* out, int N, int64_t chw, int T, void* stream) {
    EOD_REQUIRE(p0c && noise && betas && alphas, "ddpm_step_p0: bad args");
    DdpmP0Args g = {x_t, nullptr, p0c, noise, (const long long*)t, betas, alphas, acp, out, N, (long long)chw, T, 0};
    return ddpm_p0_launch<true>("ddpm_step_p0", g, stream);
}

// ---------------------------------------------------------------------------------------------
// Prediction targets other than the noise (DESIGN.md sections 8.2 and 9.16): the model output read as x0 or as v.  The data prediction is
// formed directly from (x, o), never through a noise estimate, and the chain route goes on from it (the links, then the _p0 steps).  The
// bodies are param_body.h (a host program compiles them, too).  Streaming kernels in ddpm_p0_kernel's shape: grid (blocks, N), quads of a
// sample, 16-byte accesses where chw % 4 == 0 and every pointer is aligned, element by element otherwise; the scalar-level form is N = 1.
// ---------------------------------------------------------------------------------------------
template <bool PAIR, bool VEC>
__global__ void __launch_bounds__(256) param_kernel(ParamArgs g) {
    const long long first = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
    if (PAIR) q_sample_v_thread<VEC>(g, blockIdx.y, first, stride);
    else param_pred_thread<VEC>(g, blockIdx.y, first, stride);
}

template <bool PAIR>
static int param_launch(const char* what, const ParamArgs& g, void* stream) {
    EOD_REQUIRE(g.x && g.o && g.out0 && g.N > 0 && g.chw > 0, "%s: bad args", what);
    EOD_REQUIRE(!g.t || (g.sa_tab && g.s1_tab && g.T > 0), "%s: bad args", what);
    const long long n = (long long)g.N * g.chw;
    float* const outs[2] = {g.out0, g.out1};
    const float* const ins[2] = {g.x, g.o};
    const float* const tables[2] = {g.sa_tab, g.s1_tab};
    bool vec = g.chw % 4 == 0 && eod_aligned16(g.x) && eod_aligned16(g.o);
    EOD_REQUIRE(!g.out1 || !eod_overlap2(g.out0, n, g.out1, n), "%s: the two outputs overlap", what);
    for (float* o : outs) {
        if (!o) continue;
        for (const float* p : ins) EOD_REQUIRE(!eod_overlap2(o, n, p, n), "%s: an output overlaps an input", what);
        if (g.t) {
            for (const float* p : tables) EOD_REQUIRE(!eod_overlap2(o, n, p, g.T), "%s: an output overlaps a schedule table", what);
            EOD_REQUIRE(!eod_overlap2(o, n, reinterpret_cast<const float*>(g.t), 2LL * g.N), "%s: an output overlaps t", what);
        }
        vec = vec && eod_aligned16(o);
    }
    const dim3 grid(blocks_for((g.chw + 3) / 4, 2048), g.N), block(256);
    if (vec) hipLaunchKernelGGL((param_kernel<PAIR, true>), grid, block, 0, (hipStream_t)stream, g);
    else hipLaunchKernelGGL((param_kernel<PAIR, false>), grid, block, 0, (hipStream_t)stream, g);
    EOD_CHECK_LAUNCH(what);
    return EOD_OK;
}

extern "C" int eod_param_pred(const float* x, const float* o, int kind, float a, float sqrt_1m_a, int clip, float* p0, float* e_t, int64_t numel,
                              void* stream) {
    EOD_REQUIRE(kind == PARAM_X0 || kind == PARAM_V, "param_pred: kind is 1 (x0) or 2 (v), got %d (the noise form is eod_pred_x0)", kind);
    EOD_REQUIRE(a >= 0.0f && a <= 1.0f, "param_pred: needs 0 <= a <= 1, got %g", (double)a);
    EOD_REQUIRE(kind != PARAM_X0 || !e_t || sqrt_1m_a > 0.0f, "param_pred: the noise estimate of an x0 output needs sqrt_1m_a > 0, got %g", (double)sqrt_1m_a);
    ParamArgs g = {x, o, nullptr, nullptr, nullptr, a, sqrt_1m_a, p0, e_t, 1, (long long)numel, 0, kind, clip};
    return param_launch<false>("param_pred", g, stream);
}

extern "C" int eod_ddpm_param_pred(const float* x_t, const float* o, const int64_t* t, const float* sqrt_acp, const float* sqrt_1m_acp, int kind,
                                   int clip, float* p0, int N, int64_t chw, int T, void* stream) {
    EOD_REQUIRE(kind == PARAM_X0 || kind == PARAM_V, "ddpm_param_pred: kind is 1 (x0) or 2 (v), got %d (the noise form is eod_ddpm_pred_x0)", kind);
    EOD_REQUIRE(t && sqrt_acp && sqrt_1m_acp && T > 0, "ddpm_param_pred: bad args");
    ParamArgs g = {x_t, o, (const long long*)t, sqrt_acp, sqrt_1m_acp, 0.0f, 0.0f, p0, nullptr, N, (long long)chw, T, kind, clip};
    return param_launch<false>("ddpm_param_pred", g, stream);
}

extern "C" int eod_q_sample_v(const float* x0, const float* noise, const int64_t* t, const float* sqrt_acp, const float* sqrt_1m_acp, float* x_t,
                              float* v, int N, int64_t chw, int T, void* stream) {
    EOD_REQUIRE(t && sqrt_acp && sqrt_1m_acp && v && T > 0, "q_sample_v: bad args");
    ParamArgs g = {x0, noise, (const long long*)t, sqrt_acp, sqrt_1m_acp, 0.0f, 0.0f, x_t, v, N, (long long)chw, T, PARAM_V, 0};
    return param_launch<true>("q_sample_v", g, stream);
}

// ---------------------------------------------------------------------------------------------
// Learned variance: the model output is [N][2][chw], mean half and variance half, both read in place with a sample
// stride of 2 * chw.  eod_ddpm_var_pred is eod_ddpm_pred_x0 / eod_ddpm_param_pred on the mean half, eod_ddpm_step_p0_var is
// eod_ddpm_step_p0 with sigma = sigma_min[t] * expf(((v + 1) * 0.5) * half_gap[t]) per element.  The bodies are var_body.h (a host program
// compiles them, too).  Streaming kernels in ddpm_p0_kernel's shape.
// ---------------------------------------------------------------------------------------------
template <bool STEP, bool VEC>
__global__ void __launch_bounds__(256) var_kernel(VarArgs g) {
    const long long first = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
    if (STEP) var_step_thread<VEC>(g, blockIdx.y, first, stride);
    else var_pred_thread<VEC>(g, blockIdx.y, first, stride);
}

template <bool STEP>
static int var_launch(const char* what, const VarArgs& g, void* stream) {
    EOD_REQUIRE(g.x && g.o && g.t && g.out && g.N > 0 && g.chw > 0 && g.T > 0, "%s: bad args", what);
    const long long n = (long long)g.N * g.chw;
    const float* const tensors[3] = {g.x, g.p0c, g.z};
    const float* const tables[7] = {g.betas, g.alphas, g.acp, g.sa_tab, g.s1_tab, g.sigma_min, g.half_gap};
    bool vec = g.chw % 4 == 0 && eod_aligned16(g.out) && eod_aligned16(g.o);
    EOD_REQUIRE(!eod_overlap2(g.out, n, g.o, 2 * n), "%s: the output overlaps the model output", what);
    for (const float* p : tensors) {
        if (!p) continue;
        EOD_REQUIRE(!eod_overlap2(g.out, n, p, n), "%s: the output overlaps an input", what);
        vec = vec && eod_aligned16(p);
    }
    for (const float* p : tables) EOD_REQUIRE(!p || !eod_overlap2(g.out, n, p, g.T), "%s: the output overlaps a table", what);
    EOD_REQUIRE(!eod_overlap2(g.out, n, reinterpret_cast<const float*>(g.t), 2LL * g.N), "%s: the output overlaps t", what);
    const dim3 grid(blocks_for((g.chw + 3) / 4, 2048), g.N), block(256);
    if (vec) hipLaunchKernelGGL((var_kernel<STEP, true>), grid, block, 0, (hipStream_t)stream, g);
    else hipLaunchKernelGGL((var_kernel<STEP, false>), grid, block, 0, (hipStream_t)stream, g);
    EOD_CHECK_LAUNCH(what);
    return EOD_OK;
}

extern "C" int eod_ddpm_var_pred(const float* x_t, const float* o, const int64_t* t, const float* acp, const float* sqrt_acp,
                                 const float* sqrt_1m_acp, int kind, int clip, float* p0, int N, int64_t chw, int T, void* stream) {
    EOD_REQUIRE(kind >= PARAM_EPS && kind <= PARAM_V, "ddpm_var_pred: kind is 0 (eps), 1 (x0) or 2 (v), got %d", kind);
    EOD_REQUIRE(kind == PARAM_EPS ? acp != nullptr : (sqrt_acp && sqrt_1m_acp), "ddpm_var_pred: bad args (a table of this kind is null)");
    VarArgs g = {x_t, o, nullptr, nullptr, (const long long*)t, nullptr, nullptr, kind == PARAM_EPS ? acp : nullptr,
                 kind == PARAM_EPS ? nullptr : sqrt_acp, kind == PARAM_EPS ? nullptr : sqrt_1m_acp, nullptr, nullptr, p0, N, (long long)chw, T, kind,
                 clip};
    return var_launch<false>("ddpm_var_pred", g, stream);
}

extern "C" int eod_ddpm_step_p0_var(const float* x_t, const float* p0, const float* o, const float* noise, const int64_t* t, const float* betas,
                                    const float* alphas, const float* acp, const float* sigma_min, const float* half_gap, float* out, int N,
                                    int64_t chw, int T, void* stream) {
    EOD_REQUIRE(p0 && noise && betas && alphas && acp && sigma_min && half_gap, "ddpm_step_p0_var: bad args");
    VarArgs g = {x_t, o, p0, noise, (const long long*)t, betas, alphas, acp, nullptr, nullptr, sigma_min, half_gap, out, N, (long long)chw, T, 0, 0};
    return var_launch<true>("ddpm_step_p0_var", g, stream);
}

extern "C" int eod_cfg_combine(const float* e_uncond, const float* e_cond, float scale, float* out, int64_t numel, void* stream) {
    EOD_REQUIRE(e_uncond && e_cond && out && numel > 0, "cfg_combine: bad args");
    hipLaunchKernelGGL(cfg_combine_kernel, dim3(blocks_for(numel, 4096)), dim3(256), 0, (hipStream_t)stream, e_uncond, e_cond, scale, out, (long long)numel);
    EOD_CHECK_LAUNCH("cfg_combine");
    return EOD_OK;
}

extern "C" int eod_ldm_p_sample(const float* x, const float* eps, const float* noise, const int64_t* t, const float* sqrt_recip_acp,
                                const float* sqrt_recipm1_acp, const float* post_coef1, const float* post_coef2,
                                const float* post_logvar, float* out, int N, int64_t chw, int T, int clip, void* stream) {
    EOD_REQUIRE(x && eps && noise && t && sqrt_recip_acp && sqrt_recipm1_acp && post_coef1 && post_coef2 && post_logvar && out && N > 0 && chw > 0 && T > 0,
                "ldm_p_sample: bad args");
    dim3 grid(blocks_for(chw, 512), N);
    if (clip)
        hipLaunchKernelGGL(ldm_p_sample_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, eps, noise, (const long long*)t, sqrt_recip_acp, sqrt_recipm1_acp, post_coef1, post_coef2, post_logvar, out, (long long)chw, T);
    else
        hipLaunchKernelGGL(ldm_p_sample_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, eps, noise, (const long long*)t, sqrt_recip_acp, sqrt_recipm1_acp, post_coef1, post_coef2, post_logvar, out, (long long)chw, T);
    EOD_CHECK_LAUNCH("ldm_p_sample");
    return EOD_OK;
}


// ---------------------------------------------------------------------------------------------
// Harness-side elementwise ops of inference.py, same bit-exact convention as above:
//   repaint_cond   inference.py:100-109   cond = cat(image, 1 - mask)   (cond_type == "sum": mask 1 = keep after the inversion)
//   postprocess    inference.py:128       samples.clip(0, 1)  |  (samples + 1) / 2
//   masked_preview inference.py:134       image * (mask + 0.7).clip(0, 1)
// ---------------------------------------------------------------------------------------------
// torch.clip(v, 0, 1) = min(max(v, 0), 1) with torch's comparisons: a NaN stays NaN and -0 stays -0 (fmaxf(-0, 0) returns +0 here)
__device__ __forceinline__ float clip_01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

__global__ void repaint_cond_kernel(const float* __restrict__ image, const float* __restrict__ mask, float* __restrict__ cond, int C,
                                    long long hw, int invert) {
    const int n = blockIdx.y;
    const long long per_in = (long long)C * hw, per_out = (long long)(C + 1) * hw;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < per_out; i += (long long)gridDim.x * blockDim.x) {
        float v;
        if (i < per_in) {
            v = image[(long long)n * per_in + i];
        } else {
            const float m = mask[(long long)n * hw + (i - per_in)];
            v = invert ? 1.0f - m : m;
        }
        cond[(long long)n * per_out + i] = v;
    }
}

__global__ void postprocess_kernel(const float* __restrict__ x, float* __restrict__ y, long long numel, int mode) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < numel; i += (long long)gridDim.x * blockDim.x) {
        const float v = x[i];
        float o;
        if (mode == 0) {
            o = clip_01(v);
        } else {
            const float a = v + 1.0f;
            o = a / 2.0f;
        }
        y[i] = o;
    }
}

__global__ void masked_preview_kernel(const float* __restrict__ image, const float* __restrict__ mask, float* __restrict__ out, int C,
                                      long long hw, float lift) {
    const int n = blockIdx.y;
    const long long per = (long long)C * hw;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < per; i += (long long)gridDim.x * blockDim.x) {
        const float a = mask[(long long)n * hw + (i % hw)] + lift;
        const float g = clip_01(a);
        out[(long long)n * per + i] = image[(long long)n * per + i] * g;
    }
}

extern "C" int eod_repaint_cond(const float* image, const float* mask, float* cond, int N, int C, int64_t hw, int invert, void* stream) {
    EOD_REQUIRE(image && mask && cond && N > 0 && C > 0 && hw > 0, "repaint_cond: bad args");
    hipLaunchKernelGGL(repaint_cond_kernel, dim3(blocks_for((long long)(C + 1) * hw, 512), N), dim3(256), 0, (hipStream_t)stream, image, mask, cond, C, (long long)hw, invert);
    EOD_CHECK_LAUNCH("repaint_cond");
    return EOD_OK;
}

extern "C" int eod_postprocess(const float* x, float* y, int64_t numel, int mode, void* stream) {
    EOD_REQUIRE(x && y && numel > 0 && (mode == 0 || mode == 1), "postprocess: bad args");
    hipLaunchKernelGGL(postprocess_kernel, dim3(blocks_for(numel, 4096)), dim3(256), 0, (hipStream_t)stream, x, y, (long long)numel, mode);
    EOD_CHECK_LAUNCH("postprocess");
    return EOD_OK;
}

extern "C" int eod_masked_preview(const float* image, const float* mask, float* out, int N, int C, int64_t hw, float lift, void* stream) {
    EOD_REQUIRE(image && mask && out && N > 0 && C > 0 && hw > 0, "masked_preview: bad args");
    hipLaunchKernelGGL(masked_preview_kernel, dim3(blocks_for((long long)C * hw, 512), N), dim3(256), 0, (hipStream_t)stream, image, mask, out, C, (long long)hw, lift);
    EOD_CHECK_LAUNCH("masked_preview");
    return EOD_OK;
}
