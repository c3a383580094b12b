/* The C ABI of the learned-variance kernels (csrc/sampler.hip and csrc/train.hip, bodies in csrc/var_body.h).  Included by eodiff.h, whose
 * EOD_ABI_VERSION, error codes and conventions hold here; eo_diffusion_amd/_lib.py mirrors these declarations in VAR_SYMBOLS. */
#ifndef EODIFF_VAR_H
#define EODIFF_VAR_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Learned variance (Nichol & Dhariwal 2021; guided-diffusion's learn_sigma=True; DESIGN.md sections 8.3 and 9.17).  The model output is
 * o [N][2 C][H][W] = [N][2][chw] fp32: the mean half o[n][0], read under the model's parameterization (kind 0 = the noise, 1 = x0, 2 = v),
 * and the variance half v = o[n][1], an interpolation coefficient between the two ends of the reverse variance:
 *     lv = ln beta~_t + ((v + 1) / 2) (ln beta_t - ln beta~_t),   beta~_t = beta_t (1 - acp_{t-1}) / (1 - acp_t),  beta~_0 := beta~_1.
 * Both halves are read IN PLACE, with a sample stride of 2 chw; no dense copy is made.  The per-timestep levels are derived by the caller in
 * float64 from the schedule (EODiffusion.variance_tables) and live on the device.  Every element index is formed in 64 bits.
 *
 * The ancestral step, cut where the prediction is complete as eod_ddpm_pred_x0 / eod_ddpm_step_p0 are (the links of an observation or a
 * threshold go in between).  x_t, p0, noise, out: [N][chw]; t: int64 [N]; tables [T]:
 *   eod_ddpm_var_pred: the data prediction of the mean half.  kind 0: eod_ddpm_pred_x0's operations from acp (sqrt_acp / sqrt_1m_acp may be
 *     NULL); kind 1, 2: eod_ddpm_param_pred's from sqrt_acp / sqrt_1m_acp (acp may be NULL).  Bit-equal to those kernels on a dense copy of the
 *     mean half.  The variance half is never read.
 *   eod_ddpm_step_p0_var: eod_ddpm_step_p0 with the standard deviation of every element, in fp32, every operation rounded once:
 *         frac = (v + 1) * 0.5;   arg = frac * half_gap[t];   sigma = sigma_min[t] * expf(arg);   out = mean + (sigma * noise)
 *     sigma_min = (float) sqrt(beta~_t), half_gap = (float)((ln beta_t - ln beta~_t) / 2).  The batch-wide rule of eod_ddpm_step stays: with
 *     a member at t = 0 the standard deviation is 0 for the whole batch and v is not read (the bits of eod_ddpm_step_p0).  The mean half is
 *     never read.
 * A timestep outside [0, T) fills that sample's output with NaN.  EOD_EINVAL with nothing launched: a null pointer (the tables a kind does not
 * use excepted), N / chw / T <= 0, a kind outside 0..2, the output overlapping an input, a table or t.  16-byte accesses where chw % 4 == 0
 * and every tensor pointer is 16-byte aligned, element by element otherwise: same arithmetic.  Nothing is allocated, copied or synchronised:
 * the calls can be captured in a graph. */
int eod_ddpm_var_pred(const float* x_t, const float* o, const int64_t* t, const float* acp, const float* sqrt_acp, const float* sqrt_1m_acp,
                      int kind, int clip, float* p0, int N, int64_t chw, int T, void* stream);
int eod_ddpm_step_p0_var(const float* x_t, const float* p0, const float* o, const float* noise, const int64_t* t, const float* betas,
                         const float* alphas, const float* acp, const float* sigma_min, const float* half_gap, float* out, int N, int64_t chw,
                         int T, void* stream);

/* The hybrid objective L = L_simple + lambda L_vlb in one fused pass over o [N][2 C][H][W], target, x_0, x_t [N][C][H][W], an optional mask
 * and an optional weight (both as in eod_diffusion_loss, whose kinds l2 / l1 / huber the simple term has).
 *   simple[n] = L_n and the mean half of grad: eod_diffusion_loss's on a dense copy of the mean half, bit for bit.
 *   vlb[n] (float64) = V_n = sum_e m_e term_e / S_n (0 where S_n = 0), the variational-bound term in bits per element, float64 throughout,
 *     with the mean DETACHED (its gradient goes to v alone).  With p0 the unclamped prediction of the mean half at (x_t, t) formed in
 *     float64 from the fp32 tables (kind 0: (x_t - s1 o) / sa; 1: o; 2: sa x_t - s1 o) and c1[t] = beta_t sqrt(acp_{t-1}) / (1 - acp_t):
 *       t > 0:  term = 0.5 (-1 + (lv - lmin) + exp(lmin - lv) + (c1 (x_0 - p0))^2 exp(-lv)) / ln 2           (the KL of the two posteriors)
 *       t = 0:  term = -log(max(P, 1e-12)) / ln 2, the likelihood of x_0 under the Gaussian N(c1 p0, exp(lv)) discretised to bins of half-width
 *               h: plus = (x_0 - c1 p0 + h) exp(-lv / 2), minus = (.. - h) ..;  P = Phi(plus) where x_0 < -0.999, 1 - Phi(minus) where
 *               x_0 > 0.999, Phi(plus) - Phi(minus) otherwise; Phi is the EXACT normal distribution function through erfc (guided-diffusion
 *               uses a tanh approximation)
 *     The branch is per SAMPLE.  lmin[t] = ln beta~_t and gap[t] = ln beta_t - ln beta~_t are float64 tables [T] like c1.
 *   loss[0] = (1/N) sum_n (w_n L_n + lambda V_n): the weight applies to the simple term only.
 *   grad (optional) [N][2 C][H][W]: the variance half is (float)((lambda / (N S_n)) m_e d term / d v) formed in double, d lv / d v = gap / 2;
 *     a P at the clamp has derivative 0.
 * An element whose m_e is exactly 0 is skipped in both terms and both halves of grad (+0.0 there).  A timestep outside [0, T) makes that
 * sample's simple, vlb and grad NaN (and so loss).  Sums are float64 in the discipline of csrc/met_sum.h: no floating-point atomics, and a
 * sample's bits depend on that sample alone.  One workgroup column per sample: the branch on t is uniform within a workgroup.  With a mask:
 * one pass over the mask, then the fused pass; no host synchronisation; capturable.  EOD_EINVAL with nothing launched: a null pointer (mask,
 * weight, grad excepted), a size <= 0, N > 65535, a bad kind / param_kind / mask shape, delta <= 0 under huber, lambda or h not finite or
 * h <= 0, an output overlapping an input or another output, a workspace that is misaligned or smaller than
 * eod_hybrid_loss_workspace_size(N, C, H, W) bytes (-1: bad arguments). */
int64_t eod_hybrid_loss_workspace_size(int N, int C, int H, int W);
int eod_hybrid_loss(const float* o, const float* target, const float* x0, const float* x_t, const int64_t* t, const float* mask, int mask_n,
                    int mask_c, const float* weight, const float* sqrt_acp, const float* sqrt_1m_acp, const double* c1, const double* lmin,
                    const double* gap, int N, int C, int H, int W, int T, int param_kind, int kind, float delta, double lambda, double h,
                    float* loss, float* simple, double* vlb, float* grad, void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
