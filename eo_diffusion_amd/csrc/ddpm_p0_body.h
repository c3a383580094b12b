// The bodies of the two kernels that are the clipped DDPM step cut where its data prediction is complete (csrc/sampler.hip:
// eod_ddpm_pred_x0, eod_ddpm_step_p0), the quads of one sample that one thread owns at a time.  The kernels call
// them with (blockIdx.y, the thread's number in the grid's x direction, the number of such threads); a host program can do the same
// with a loop over the samples and the thread numbers (tests/ancestral_host_check.cc does, under the address and undefined-behaviour
// sanitizers).  Nothing here needs the HIP headers.  Built with -ffp-contract=off: every operation is rounded once, in the order of
// ddpm_step_kernel<true>, whose bits pred -> step therefore has.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef DDPM_P0_FN
#define DDPM_P0_FN static inline
#endif

typedef float ddpm_f4 __attribute__((ext_vector_type(4)));

// The static clamp of a data prediction, torch.clamp(v, -1, 1): fminf / fmaxf drop a NaN operand (a NaN would become -1 and the step
// a plausible image), so the NaN is put back.  The ONE statement of the clamp for every sampler kernel; bits of a non-NaN v: fminf(fmaxf()).
DDPM_P0_FN float clamp_pm1(float v) {
    const float c = fminf(fmaxf(v, -1.0f), 1.0f);
    return v != v ? v : c;
}

struct DdpmP0Args {
    const float* x;        // [N][chw] x_t
    const float* e;        // pred: [N][chw] the noise estimate
    const float* p0c;      // step: [N][chw] the (projected) data prediction
    const float* z;        // step: [N][chw] the draw
    const long long* t;    // [N]
    const float* betas;    // step: [T]
    const float* alphas;   // step: [T]
    const float* acp;      // [T]
    float* out;            // [N][chw]
    int N;
    long long chw;
    int T, clip;
};

// a timestep outside [0, T) is computed with index 0 and the sample's output is NaN (checked_t of sampler.hip)
DDPM_P0_FN long long ddpm_p0_t(const DdpmP0Args& g, int n, bool& bad) {
    const long long tn = g.t[n];
    bad = tn < 0 || tn >= (long long)g.T;
    return bad ? 0 : tn;
}

DDPM_P0_FN float ddpm_p0_poison(bool bad, float v) { return bad ? __builtin_nanf("") : v; }

template <bool VEC>
DDPM_P0_FN void ddpm_p0_load(const float* src, float* v, int nv) {
    if (VEC) {
        const ddpm_f4 q = *reinterpret_cast<const ddpm_f4*>(src);
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
    } else {
        for (int j = 0; j < nv; ++j) v[j] = src[j];
    }
}

template <bool VEC>
DDPM_P0_FN void ddpm_p0_store(float* dst, const float* v, int nv) {
    if (VEC) {
        const ddpm_f4 q = {v[0], v[1], v[2], v[3]};
        *reinterpret_cast<ddpm_f4*>(dst) = q;
    } else {
        for (int j = 0; j < nv; ++j) dst[j] = v[j];
    }
}

// ------------------------------------------------------------------------------------------------ p0 = (c_x0 * x) - (c_pred * e) [clamped]
template <bool VEC>
DDPM_P0_FN void ddpm_pred_x0_thread(const DdpmP0Args& g, int n, long long first, long long stride) {
    bool bad;
    const long long tn = ddpm_p0_t(g, n, bad);
    const float acp_t = g.acp[tn];
    const float c_x0 = sqrtf(1.0f / acp_t);
    const float c_pred = sqrtf(1.0f / acp_t - 1.0f);
    const long long base = (long long)n * g.chw, quads = (g.chw + 3) / 4;
    for (long long qd = first; qd < quads; qd += stride) {
        const long long i0 = qd * 4;
        const int nv = VEC || g.chw - i0 >= 4 ? 4 : (int)(g.chw - i0);
        float xv[4] = {0.f, 0.f, 0.f, 0.f}, ev[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
        ddpm_p0_load<VEC>(g.x + base + i0, xv, nv);
        ddpm_p0_load<VEC>(g.e + base + i0, ev, nv);
        for (int j = 0; j < 4; ++j) {
            const float u = c_x0 * xv[j];
            const float v = c_pred * ev[j];
            float p0 = u - v;
            if (g.clip) p0 = clamp_pm1(p0);
            o[j] = ddpm_p0_poison(bad, p0);
        }
        ddpm_p0_store<VEC>(g.out + base + i0, o, nv);
    }
}

// ------------------------------------------------------------------------------------------------ out = mean(p0c, x) + (std * z)
template <bool VEC>
DDPM_P0_FN void ddpm_step_p0_thread(const DdpmP0Args& g, int n, long long first, long long stride) {
    bool bad;
    const long long tn = ddpm_p0_t(g, n, bad);
    long long tmin = g.t[0];
    for (int i = 1; i < g.N; ++i) tmin = g.t[i] < tmin ? g.t[i] : tmin;
    const bool all_pos = tmin > 0;  // the reference branches on the BATCH minimum (model.py:140)
    const float alpha_t = g.alphas[tn], acp_t = g.acp[tn], beta_t = g.betas[tn];
    float m_x0, m_xt = 0.0f, std = 0.0f;
    if (all_pos) {
        const float acp_prev = g.acp[tn > 0 ? tn - 1 : 0];  // (tn == 0 here: a sample out of range, whose output is NaN)
        m_x0 = beta_t * sqrtf(acp_prev) / (1.0f - acp_t);
        m_xt = (1.0f - acp_prev) * sqrtf(alpha_t) / (1.0f - acp_t);
        std = sqrtf(beta_t * (1.0f - acp_prev) / (1.0f - acp_t));
    } else {
        m_x0 = beta_t / (1.0f - acp_t);
    }
    const long long base = (long long)n * g.chw, quads = (g.chw + 3) / 4;
    for (long long qd = first; qd < quads; qd += stride) {
        const long long i0 = qd * 4;
        const int nv = VEC || g.chw - i0 >= 4 ? 4 : (int)(g.chw - i0);
        float xv[4] = {0.f, 0.f, 0.f, 0.f}, pv[4] = {0.f, 0.f, 0.f, 0.f}, zv[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
        ddpm_p0_load<VEC>(g.p0c + base + i0, pv, nv);
        ddpm_p0_load<VEC>(g.x + base + i0, xv, nv);
        ddpm_p0_load<VEC>(g.z + base + i0, zv, nv);
        for (int j = 0; j < 4; ++j) {
            float mean;
            if (all_pos) {
                const float p = m_x0 * pv[j];
                const float q = m_xt * xv[j];
                mean = p + q;
            } else {
                mean = m_x0 * pv[j];
            }
            const float sz = std * zv[j];
            o[j] = ddpm_p0_poison(bad, mean + sz);
        }
        ddpm_p0_store<VEC>(g.out + base + i0, o, nv);
    }
}
