/*
 * eodiff.h -- C ABI of libeodiff.so: the MI355X (gfx950) replacement for the stock-torch op call
 * sites on the EODiffusion hot path.
 *
 * Contract: stateless, stream-ordered entry points.  Every function returns 0 on success and a
 * negative EOD_E* code on failure (message via eod_last_error()).  The caller owns every buffer
 * (raw device pointers); nothing is allocated, freed or synchronised inside, so every call is
 * hipGraph-capturable.  `stream` is a hipStream_t passed as void*.  No torch types cross here.
 *
 * Activation layout inside the library is channels-last ("NHWC": [N][H][W][C], C contiguous) in
 * the storage dtype of the precision mode (EOD_F32: exact-fp32 MFMA; EOD_F16: fp16 storage,
 * fp16 MFMA, fp32 accumulate).  The reference API layout (NCHW fp32) is converted at the edges.
 *
 * Each entry point cites the reference call site (file:line in furio1999/EO_Diffusion) it replaces.
 */
#ifndef EODIFF_H
#define EODIFF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EOD_OK 0
#define EOD_EINVAL (-1)  /* bad shape / alignment / argument */
#define EOD_ELAUNCH (-2) /* HIP launch error */
#define EOD_ENOSYS (-3)  /* variant not built */

enum { EOD_F32 = 0, EOD_F16 = 1 };

const char* eod_last_error(void);
/* ABI revision of this header: bumped whenever an entry point's arguments, a descriptor layout or the size / meaning of a caller-provided
 * state buffer changes (round 3 -> 4: eod_gn_finalize, eod_gn_apply, eod_gn_bwd_apply, eod_attention_fwd_nat, the 4 + Cout slot weight-scale
 * buffer of eod_pack_conv_weight_split, the 4-int state of eod_adamw_step_guarded).  eod_version() returns the value the library was built
 * with; a binding compares it with the header it mirrors at load time (eo_diffusion_amd/_lib.py does) instead of finding out by an
 * out-of-bounds device write. */
#define EOD_ABI_VERSION 120
int eod_version(void);
/* Kernel-selection options ("skip_fuse", "head", "halo_bn256", "halo_splitk", "first", "s2_halo": 1 / 0; "gn_fuse_max_cout": n, -1 = default;
 * "head_tpw": pixel tiles per workgroup of conv_head_kernel, 0 = chosen per launch = default): every option has one measured-best default, the other arm computes the same function
 * on another kernel (same-box A/B runs, per-switch parity tests).  Read from the environment (EOD_SKIP_FUSE, EOD_HEAD, EOD_HALO_BN256,
 * EOD_GN_FUSE_MAX_COUT, EOD_HALO_SPLITK, EOD_FIRST, EOD_HEAD_TPW, EOD_S2_HALO) at first use; returns the previous value,
 * or EOD_EINVAL for an unknown name.  Plans built before a change keep the kernels they were built with. */
int eod_set_option(const char* name, int value);
int eod_get_option(const char* name);
/* sizeof() of the descriptor structs as compiled (1 conv, 2 gemm, 3 temb, 4 small, 5 op): lets a
 * foreign-language binding verify its mirror of the layouts at load time. */
int eod_struct_size(int kind);

/* ------------------------------------------------------------------------------------------
 * k1/k2/k3/k4/k9/k10: implicit-GEMM convolution on MFMA.
 * Replaces nn.Conv2d call sites: ResBlock.in_layers[2]/out_layers[3] unet_openai.py:315,341;
 * skip_connection 1x1 :352; Downsample.op (stride 2) :262-264; Upsample.conv after nearest-2x
 * F.interpolate :227,236 (the 2x is virtual: upsample=1 indexes h>>1,w>>1); th.cat :773 is
 * virtual too (two A sources x | x2); first/last conv :609,742.
 * y[n,ho,wo,co] = alpha * sum_{tap,c} A(n, ho*stride-pad+dy, wo*stride-pad+dx, c) * w[tap][co][c]
 *                 + bias[co] + cbias[n*cbias_stride + co] + res[n,ho,wo,co]
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    const void* x;       /* A source 0, NHWC [N][H][W][C0], storage dtype                      */
    const void* x2;      /* A source 1 (virtual concat) [N][H][W][C1], or NULL when C1 == 0     */
    const void* w;       /* packed weights [ksize*ksize][Cout][C0+C1], storage dtype            */
    const float* bias;   /* [Cout] fp32 or NULL                                                 */
    const float* cbias;  /* per-sample bias (timestep embedding, unet_openai.py:374-383) or NULL */
    const void* res;     /* residual, NHWC [N][Ho][Wo][Cout], storage dtype, or NULL (:385)      */
    void* y;             /* output: NHWC storage dtype (out_nchw_f32=0) or NCHW fp32 (=1)        */
    int64_t cbias_stride;
    int32_t dtype;       /* EOD_F32 | EOD_F16 */
    int32_t N, H, W;     /* input spatial dims as stored (before the virtual 2x upsample)        */
    int32_t C0, C1, Cout;
    int32_t ksize;       /* 1 or 3 */
    int32_t stride;      /* 1 or 2 */
    int32_t pad;         /* 0 or 1 */
    int32_t upsample;    /* 1: A is the nearest-2x upsampling of x (H,W are the stored dims);
                            2: A is x with zeros inserted between the pixels (z[2i][2j] = x[i][j]): the input of the
                            backward-data conv of a stride-2 conv (training path);
                            3: as 1, computed as four 2x2-tap parity classes with pre-summed weights (see eod_conv_up4_ok);
                            4: the backward-data of 3 (see eod_conv_up4_bwd_ok): x = dY on the (H x W) = (2 Ho x 2 Wo) grid */
    int32_t pad_tl;      /* 1: extra zero row/col on top/left after upsampling (3x3 -> 7x7 hack,
                            unet_openai.py:237-239)                                              */
    int32_t Ho, Wo;      /* output spatial dims */
    int32_t out_nchw_f32;
    float alpha;
    float* stats;        /* optional OUT: per-channel GroupNorm partial sums of y, [N][stats_slots][Cout][2] (sum, sumsq),
                            produced by the epilogue (saves the statistics read pass of the next GroupNorm); NULL = off */
    int32_t stats_slots; /* must equal eod_conv_stats_slots(d) when stats != NULL */
    int32_t gn_silu;     /* with gn_scale_shift: 1 = SiLU after the affine normalisation */
    const float* gn_scale_shift; /* optional: fuse GroupNorm32 (+FiLM) (+SiLU) of the conv INPUT (in_layers[0:2] / out_layers[0:2],
                            unet_openai.py:312-316,336-343): {scale, shift} per (image, input channel of the virtual concat),
                            [N][C0+C1][2] fp32 as written by eod_gn_finalize.  x / x2 are then the UN-normalised tensors; the
                            normalised activation is never written to HBM.  Only where eod_conv_gn_fusable(d) == 1. */
    void* workspace;     /* caller-owned scratch of eod_conv_workspace_size(d) bytes (split-K partial tiles of small maps) */
    int64_t workspace_bytes;
    int32_t w_tapmajor;  /* 1: thin-input 3x3 conv (the UNet's first conv, unet_openai.py:609: 3 / 7 / 13 image channels):
                            w is [Cout][ldk] with k = tap*C0 + c (eod_pack_conv_weight_tapmajor, ldk =
                            eod_conv_tapmajor_ldk) and the K loop runs over the flattened [tap][C0] axis -- ceil(9*C0/BK)
                            K-steps instead of 9 mostly-zero ones.  Needs C1 == 0, no upsample, C0 in {1,2,4} 16-byte chunks */
    int32_t w_split;     /* 1: "fp32x3" product -- fp32 storage, every product as three fp16 MFMAs on split operands (hi + lo):
                            w is the output of eod_pack_conv_weight_split, w_scale its scale pair.  Only where
                            eod_conv_split_ok(d) == 1 (fp32, C0 and C1 multiples of 8 -- or w_tapmajor with eod_pack_conv_weight_tapmajor_split);
                            rel. error ~2^-22 per product */
    const float* w_scale; /* device pointer to the scale buffer written by eod_pack_conv_weight_split (w_split only): float {s, 1/(16 s), -, -}
                           * followed by one int32 row exponent d_j per output row (4 + Cout slots; the parity-class form: 4 + 4 Cout):
                           * row j is packed under s * 2^d_j, the epilogue multiplies column j by 2^-d_j / (16 s) */
    const float* a_bound; /* w_split: bound table [N][32] fp32 (device) of the tensor the conv SPLITS -- x | x2 as the conv sees them, i.e. behind
                            the fused GroupNorm + SiLU when gn_scale_shift is set: entry maximum per image >= max|element|.  The kernel
                            derives a power-of-two operand scale per image from it (no host synchronisation), so the product is
                            fp32-grade for inputs of any magnitude.  Written by eod_gn_finalize (ab_norm / ab_raw) or eod_act_bound.
                            NULL = the caller guarantees |element| < 4094 (fixed scale 16) */
    /* ResBlock skip connection fused into out_layers' conv (unet_openai.py:352, 385: `return self.skip_connection(x) + h`): y gets
     * sum_c skip_w[co][c] * X(n, ho, wo, c) on top of the 3x3 conv, X = the block input (skip_x | skip_x2 as a virtual concat) at the
     * output resolution.  The skip tensor is never written: same accumulators, the K loop simply continues over X's channels.
     * skip_w = the 1x1 weight packed like `w` (eod_pack_conv_weight, ksize 1: [Cout][skip_C0 + skip_C1]; w_split: BOTH weights packed
     * by eod_pack_conv_weight_split_pair -- one common scale); the skip conv's bias can go through cbias with cbias_stride = 0.  Only where
     * eod_conv_skip_ok(d) == 1 (3x3 / stride 1 / halo-tile geometry, Cout > 64, C1 == 0, no `res`); NULL = off. */
    const void* skip_x;
    const void* skip_x2;
    const void* skip_w;
    int32_t skip_C0, skip_C1;
    const float* skip_bound; /* w_split: bound table [N][32] of skip_x | skip_x2 (see a_bound; the launch runs on the smaller of the two
                            scales because both phases feed one accumulator); NULL = |element| < 4094 guaranteed */
    int32_t x_presplit;  /* w_split, generic-kernel geometries (1x1, stride 2): x | x2 are PRE-SPLIT -- 4 bytes per element, every 8
                            channels as [8 x fp16 hi | 8 x fp16 lo] of s_n * x with s_n = the power-of-two scale that a_bound gives for
                            image n -- written by a producer that knew the bound beforehand (eod_gn_apply split_out, the fp32-storage
                            attention).  The conv DMAs the rows straight into its LDS image: no split pass per K-step. */
    const float* y_presplit_bound; /* w_split, generic-kernel geometries whose tiles lie inside one image (Ho*Wo % 128 == 0), Cout % 8 == 0:
                            write y PRE-SPLIT, scaled per image from this table [N][32] (an a-priori bound of y: eod_bound_affine; exponent
                            range of the attention kernels, s >= 2^-48) -- the qkv projection in front of eod_attention_fwd_nat(in_presplit).
                            NULL = plain fp32 output */
} eod_conv_desc;
int eod_conv2d_igemm(const eod_conv_desc* d, void* stream);
/* number of partial-sum slots per image the epilogue of this conv would write, or 0 if it cannot (tiles that straddle
 * images, NCHW output): the caller sizes `stats` with it. */
int eod_conv_stats_slots(const eod_conv_desc* d);
int eod_conv_gn_fusable(const eod_conv_desc* d);
int eod_conv_split_ok(const eod_conv_desc* d);
int eod_conv_skip_ok(const eod_conv_desc* d);
/* upsample = 3 (Upsample.conv, unet_openai.py:236-241, in 4/9 of the MACs): output pixel (2i+p, 2j+q) of the 3x3 conv over the nearest-2x
 * image reads only stored rows {i-1+p, i+p} and columns {j-1+q, j+q}, so each parity class (p, q) is a 2x2-tap conv of the STORED map with
 * summed taps (rows: p = 0 -> [w0 | w1+w2], p = 1 -> [w0+w1 | w2]; columns alike).  w is then ONE packed tensor (eod_pack_conv_weight /
 * _split) of a [4*Cout][Cin][3][3] weight whose row block 2p+q holds class (p, q)'s kernel in the tap slots (dy' in {p, p+1}, dx' in
 * {q, q+1}) and zeros elsewhere; Cout stays the real channel count.  1 where this form is available (fp16, or fp32 with w_split). */
int eod_conv_up4_ok(const eod_conv_desc* d);
/* the [4*Cout][Cin][3][3] fp32 class-kernel tensor of that form from the OIHW weight (device side: the training step re-forms it from
 * the live parameter every step, then packs it like any weight) */
int eod_conv_up4_weights(const float* w_oihw, float* wc, int Cout, int Cin, void* stream);
/* upsample = 4 (fp16): dX of that conv straight from dY -- per class (p, q) a 2x2-tap conv of the stride-2 view dY[2i+p][2j+q] with the
 * transposed class kernels, the four accumulated in one dense (Ho x Wo) tile (no (2Ho x 2Wo) intermediate, no 2x2 sum pool).  w =
 * eod_pack_conv_weight_dgrad (cout_pad = 4*C0) of the class-kernel tensor of eod_conv_up4_weights; Cout = channels of dX. */
int eod_conv_up4_bwd_ok(const eod_conv_desc* d);
int64_t eod_conv_workspace_size(const eod_conv_desc* d);
/* the kernel family eod_conv2d_igemm runs this descriptor on under the current options (a static string): "conv3x3_halo_kernel",
 * "conv3x3_halo_kernel<BN=32>", "conv_up4_halo_kernel", "conv_s2_halo_kernel", "conv_first_x3_kernel", "conv_head_kernel" or "igemm_kernel" */
const char* eod_conv_kernel_name(const eod_conv_desc* d);
/* output columns per workgroup where that family is "conv3x3_halo_kernel" (32, 64, 128 or 256; 256 = the 8-wave instance, which a
 * 256 + 128 conv runs on all but its last 128 columns), 0 for every other family */
int eod_conv_halo_columns(const eod_conv_desc* d);

/* ------------------------------------------------------------------------------------------
 * k3/k7/k8: batched GEMM on MFMA,  C[b][m][n] = alpha * sum_k A[b][m][k] * B[b][n][k] (+bias)(+res)
 * A and B are both K-contiguous ("NT").  Used for the attention block (unet_openai.py:427-433):
 * qkv / proj_out Conv1d(1x1) :414,422 and the two einsums of QKVAttention(Legacy) :476-480.
 * batch index z = b0 * nb1 + b1, each operand has one stride per level (elements).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    const void* a;
    const void* b;
    const float* bias; /* fp32, or NULL */
    const void* res;   /* same layout/dtype as c, or NULL */
    void* c;
    int64_t lda, ldb, ldc;
    int64_t sa0, sa1, sb0, sb1, sc0, sc1; /* batch strides (elements) */
    int32_t dtype;     /* dtype of a, b (and res / c unless c_f32) */
    int32_t M, N, K;   /* K must be a multiple of 16 bytes worth of elements */
    int32_t nb0, nb1;
    int32_t bias_mode; /* 0 none, 1 per column n, 2 per row m, 3 = softmax-backward epilogue: bias is [batch][M], and
                          c = res * (alpha*acc - bias[z][m])  (dS = P * (dP - rowsum(dP*P)), unet_openai.py:479);
                          4 = softmax-rebuild epilogue: c = exp(alpha*acc - bias[z][m])  (P from the scores and their log-sum-exp) */
    int32_t c_f32;     /* 1: store c as fp32 regardless of dtype */
    float alpha;
    int32_t x3;        /* 1 (dtype EOD_F32, K % 8 == 0): every product as three fp16 MFMAs on operands split into hi + lo halves in LDS
                          (the fp32x3 precision mode, see eod_conv_desc.w_split) */
    const float* a_bound; /* x3: bound tables [nb0][32] of a / b (see eod_conv_desc.a_bound; indexed by the OUTER batch index b0 = image);
                          NULL = that operand is known to stay below 4094 in magnitude (softmax weights) */
    const float* b_bound;
} eod_gemm_desc;
int eod_gemm_nt(const eod_gemm_desc* d, void* stream);

/* weights: OIHW fp32 (Conv2d.weight, unet_openai.py:21-25) -> [tap][Cout][cin_pad] storage dtype */
int eod_pack_conv_weight(const float* w_oihw, void* dst, int dtype, int Cout, int Cin, int ksize,
                         int cin_pad, void* stream);
/* split-fp16 weights of the fp32x3 product (eod_conv_desc.w_split): [tap][Cout][cin_pad] at 4 bytes per element, every 8 input
 * channels as [8 x fp16 hi | 8 x fp16 lo] of s_j*w, s_j = s * 2^d_j: s = 2^k per tensor and d_j >= 0 per output row, both chosen on the
 * device so that every row's largest value lies in (2^12, 2^13] (each output channel keeps its own 22 bits whatever the other rows hold);
 * scale (device, 4 + Cout slots of 4 bytes) receives float {s, 1/(16 s), -, -} and int32 d_j.  cin_pad % 8 == 0.  No host synchronisation. */
int eod_pack_conv_weight_split(const float* w_oihw, void* dst, float* scale, int Cout, int Cin, int ksize, int cin_pad, void* stream);
/* two weights that feed ONE accumulator (eod_conv_desc.skip_w: out_layers' 3x3 conv + the 1x1 skip_connection, unet_openai.py:341,352):
 * both packed as above with one common scale s taken over the two tensors.  w2 is [Cout][Cin2] (1x1), dst2 [Cout][Cin2] at 4 bytes. */
int eod_pack_conv_weight_split_pair(const float* w_oihw, void* dst, const float* w2_oi, void* dst2, float* scale, int Cout, int Cin,
                                    int ksize, int cin_pad, int Cin2, void* stream);
/* thin-input variant: OIHW fp32 -> [Cout][ldk], k = tap*cin_pad + c, zero padded (see eod_conv_desc.w_tapmajor) */
int eod_pack_conv_weight_tapmajor(const float* w_oihw, void* dst, int dtype, int Cout, int Cin, int cin_pad, void* stream);
/* the same in the split-fp16 pair format (fp32 storage, eod_conv_desc.w_tapmajor together with w_split); scale as above */
int eod_pack_conv_weight_tapmajor_split(const float* w_oihw, void* dst, float* scale, int Cout, int Cin, int cin_pad, void* stream);
int eod_conv_tapmajor_ldk(int C0, int dtype);
/* generic strided 2-D cast-copy: dst[r][c] = (dtype) src[row_map[r]*ld_src + c]; row_map may be NULL
 * (identity); a negative row_map entry yields a zero row (K padding of attention heads) */
int eod_pack_rows(const float* src, int64_t ld_src, const int32_t* row_map, void* dst, int64_t ld_dst,
                  int dtype, int rows, int cols, void* stream);

/* API-edge layout conversion (x.type(self.dtype) / th.cat([x,cond],1), unet_openai.py:756,767):
 * dst NHWC [N][H][W][c_pad] = concat(src0 NCHW fp32 [N][C0], src1 NCHW fp32 [N][C1]), zero padded. */
int eod_nchw_to_nhwc(const float* src0, int C0, const float* src1, int C1, void* dst, int dtype,
                     int N, int H, int W, int c_pad, void* stream);
int eod_nhwc_to_nchw(const void* src, int dtype, float* dst, int N, int H, int W, int C, void* stream);

/* ------------------------------------------------------------------------------------------
 * k5: GroupNorm32(32, C) [+ SiLU]  (unet_openai.py:11-13, 71-78, 312-316, 336-343, 739-743)
 * three stream-ordered phases, deterministic (no atomics):
 *   partial : per (n, pixel-chunk p, channel) sum / sum-of-squares       -> part[N][P][Ctot][2]
 *             (skipped when the producing conv already emitted them: eod_conv_desc.stats)
 *   finalize: per (n, group) mean/rstd over BOTH concat sources (part0 [N][P0][C0][2] | part1 [N][P1][C1][2],
 *             part1 may be NULL), folded with gamma/beta (and the
 *             FiLM scale/shift of use_scale_shift_norm :377-381) into scale/shift[N][Ctot]
 *   apply   : y = act(x * scale + shift), written at channel offset `coff` of a Ctot-wide tensor
 * ------------------------------------------------------------------------------------------ */
int eod_gn_partial(const void* x, int dtype, int N, int HW, int C, float* part, int P, int Ctot,
                   int coff, void* stream);
int eod_gn_finalize(const float* part0, int P0, int C0, const float* part1, int P1, int C1, int N, int64_t HW,
                    int groups, float eps, const float* gamma, const float* beta, const float* film,
                    int64_t film_stride, float* scale_shift, float* ab_raw, float* ab_norm, void* stream);
/* ab_raw / ab_norm (optional OUT, [N][32] fp32, groups <= 32): bound tables for the split-fp16 consumers of the tensor(s) the statistics
 * were taken of (eod_conv_desc.a_bound / skip_bound): entry g of image n = an upper bound of max|x| (ab_raw) and of max|x*scale + shift|
 * (ab_norm; also bounds its SiLU) over group g, from the largest partial sum of squares -- no extra pass over the tensor.
 * eod_act_bound writes the same table for a tensor without a GroupNorm in front of its consumer: from the partial sums a conv epilogue
 * emitted (part0 [N][P0][C0][2] | part1), or -- part0 == NULL -- as the exact max|x| of x ([N][per_image] elements, any finite fp32;
 * accumulate = 1: entry-wise maximum with what the table already holds -- the further sources of a virtual concat). */
int eod_act_bound(const void* x, int dtype, int N, int64_t per_image, const float* part0, int P0, int C0, const float* part1, int P1,
                  int C1, float* ab, int accumulate, void* stream);
/* A-priori table of a linear layer's OUTPUT (a producer that writes pre-split needs its scale before it has seen its values):
 * |y_r| <= (max_r sum_c |w[r][c]|) * max|x| + max|b|.  eod_weight_l1max: coef = {max row L1 norm of w [rows][cols], max|bias|} (device,
 * once per plan); eod_bound_affine: ab_out[n][j] = ab_in[n][j] * coef[0] + coef[1]. */
int eod_weight_l1max(const float* w, int rows, int cols, const float* bias, float* coef, void* stream);
int eod_bound_affine(const float* ab_in, const float* coef, float* ab_out, int N, void* stream);
int eod_gn_apply(const void* x, int dtype, int N, int HW, int C, const float* scale_shift, int Ctot,
                 int coff, int silu, void* y, const float* split_bound, void* stream);
/* split_bound (EOD_F32, C / Ctot / coff multiples of 8): write y PRE-SPLIT for a split-fp16 consumer (eod_conv_desc.x_presplit):
 * [8 x fp16 hi | 8 x fp16 lo] per 8 channels of s_n * y, s_n from this bound table [N][32] (eod_gn_finalize's ab_norm). NULL = plain. */

/* ------------------------------------------------------------------------------------------
 * k8: fused ("flash"-style) QKVAttention / QKVAttentionLegacy forward (unet_openai.py:465-481, 497-515):
 *   out[n, t, h*d + j] = sum_s softmax_s((q_t . k_s) / sqrt(d)) v[s, j]     (scale = d^-1/4 on q and on k, :475-478)
 * online softmax in fp32, the T x T matrix is never materialised.  fp16 storage, head dim <= 64.
 *   qk  [N*T][ld_qk] : q heads at column h*dpad, k heads at k_off + h*dpad (each head zero-padded to dpad channels)
 *   vT  [N][C][ldt]  : V transposed (keys contiguous, zero beyond T)
 *   out [N*T][C]
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    const void* qk;
    const void* vT;
    void* out;
    float* lse;          /* optional OUT [N][heads][T]: log-sum-exp of every score row (natural log) -- what the training path
                            needs to rebuild P = exp(S - lse) in the backward without keeping the T x T matrix */
    int64_t ld_qk, ldt;
    int32_t dtype, N, T, C, heads, d, dpad, k_off;
} eod_attn_desc;
int eod_attention_fwd(const eod_attn_desc* d, void* stream);

/* k8 (softmax of QKVAttention, unet_openai.py:479/513): p[r][0..ldp) = softmax(s[r][0..n)), zero pad */
int eod_softmax_rows(const float* s, int64_t lds, void* p, int64_t ldp, int dtype, int64_t rows, int n,
                     void* stream);

/* ------------------------------------------------------------------------------------------
 * k6: timestep embedding MLP (unet_openai.py:81-99, 597-602, 604-605, 329-335, 763-766).
 *   emb   = W2 * silu(W1 * [cos(t f) | sin(t f)] + b1) + b2 (+ label_emb[y])
 *   out   = Wcat * silu(emb) + bcat             (all ResBlock emb_layers batched into one GEMV)
 * all fp32.  freqs[half] is the host-computed fp32 table of :92-94.  t is int64 [N]; with t_f32 != 0 it points at fp32 [N] instead
 * (`timesteps[:, None].float()`, :95: the reference's embedding also takes fractional timesteps).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    const int64_t* t;
    const float* freqs;
    const float* w1; const float* b1; /* [E][D], [E] */
    const float* w2; const float* b2; /* [E][E], [E] */
    const float* label_emb;           /* [num_classes][E] or NULL */
    const int64_t* y;                 /* [N] or NULL */
    const float* wcat; const float* bcat; /* [J][E], [J] */
    float* h1;   /* scratch [N][E] */
    float* emb;  /* out [N][E] (pre-SiLU, as the reference's emb) */
    float* out;  /* out [N][J] */
    int32_t N, D, E, J;
    int32_t t_f32, _pad;
} eod_temb_desc;
int eod_time_embed(const eod_temb_desc* d, void* stream);
/* the sinusoid alone (timestep_embedding, unet_openai.py:81-99; the reference's standalone helper): out [N][dim] fp32 =
 * [cos(t f) | sin(t f)] (+ a zero column when dim is odd); t fp32 [N] (may be fractional), freqs[dim/2] as above */
int eod_timestep_embedding(const float* t, const float* freqs, float* out, int N, int dim, void* stream);

/* ------------------------------------------------------------------------------------------
 * k11-k15: fused sampler updates.  fp32, built with -ffp-contract=off so that every rounding of
 * the reference's torch op sequence is reproduced bit-for-bit.  x/pred/noise/out are [N][CHW] fp32.
 * tables are the EODiffusion buffers (model.py:23-32) of length T, t is int64 [N].  A timestep outside [0, T) never reads
 * behind (or in front of) the tables: that sample is computed with index 0 and its output is filled with NaN (the reference's gather
 * raises there); the batch-wide branch of eod_ddpm_step follows the minimum of the timesteps as given.  The clamp of the clipped steps is
 * torch.clamp(x0, -1, 1): fminf(fmaxf(x0, -1), 1) with a NaN put back, so a NaN estimate or state gives a NaN output, never an image.
 * ------------------------------------------------------------------------------------------ */
/* model.py:94-98 (== ddpm.py:279-282) */
int eod_q_sample(const float* x0, const float* noise, const int64_t* t, const float* sqrt_acp,
                 const float* sqrt_1m_acp, float* out, int N, int64_t chw, int T, void* stream);
/* model.py:58-60  x_t <- mask*q_sample(gt,t,noise) + (1-mask)*x_t ; mask is [N][1][H][W] */
int eod_repaint_mix(const float* x_t, const float* gt, const float* mask, const float* noise,
                    const int64_t* t, const float* sqrt_acp, const float* sqrt_1m_acp, float* out,
                    int N, int C, int64_t hw, int T, void* stream);
/* model.py:126-150 (clip=1) / :101-122 (clip=0), including the batch-wide `t.min()>0` branch */
int eod_ddpm_step(const float* x_t, const float* pred, const float* noise, const int64_t* t,
                  const float* betas, const float* alphas, const float* acp, const float* sqrt_1m_acp,
                  float* out, int N, int64_t chw, int T, int clip, void* stream);
/* ddim.py:192-206; the four scalars are the fp32-rounded table entries of :192-195 */
int eod_ddim_step(const float* x, const float* e_t, const float* noise, float a_t, float a_prev,
                  float sigma_t, float sqrt_1m_at, float temperature, float* x_prev, float* pred_x0,
                  int64_t numel, void* stream);
/* DPM-Solver++ (2M), one step of the data-prediction multistep solver from the level with cumulative alpha product a_s (no reference
 * line).  Per element, every operation rounded once in fp32, in this order:
 *   se = sqrt_1m_as * e_t
 *   p0 = (x - se) / sqrtf(a_s)                     -- eod_ddim_step's operations: pred_x0 has its bits for the same (x, e_t, a, sqrt_1m_a)
 *   clip != 0:  p0 = clamp(p0, -1, 1)              -- eod_ddpm_step's clamp: fminf(fmaxf(p0, -1), 1), a NaN stays NaN (torch.clamp)
 *   D = d_prev ? (w_cur * p0) + (w_prev * d_prev) : p0
 *   x_next = (c_x * x) + (c_d * D)
 *   pred_x0 = p0                                   -- the next step's d_prev
 * d_prev NULL: first order (w_cur / w_prev are not read).  The scalars are shared by all samples and come from the host
 * (diffusion/util.py dpm_coefficients: float64, rounded once).  x, e_t, d_prev, x_next, pred_x0 are [numel] fp32.
 * EOD_EINVAL with nothing launched: a null x / e_t / x_next / pred_x0, numel <= 0, a_s outside (0, 1] (NaN included), x_next or pred_x0
 * overlapping d_prev or each other.  16-byte accesses where numel % 4 == 0 and all (five, or four) pointers are 16-byte aligned, element
 * by element otherwise: same arithmetic. */
int eod_dpmpp_step(const float* x, const float* e_t, const float* d_prev, float a_s, float sqrt_1m_as, float c_x, float c_d,
                   float w_cur, float w_prev, int clip, float* x_next, float* pred_x0, int64_t numel, void* stream);
/* Observation consistency (no reference line): eod_ddim_step / eod_dpmpp_step with the data prediction moved towards
 * an observation of per-channel block means (the range / null-space projection of DDNM for A = masked per-channel block mean, A+ =
 * replication) before the update uses it.  The tensors are [B][C][H][W] fp32; factors is a HOST array of C <= 32 ints in 1..8 (the block
 * edge per channel, 1 = observed at full resolution), read during the call and handed to the kernels by value: nothing is allocated,
 * copied or synchronised.  blk(i) = the f_c x f_c block of pixel i, anchored at the plane's origin.  Per pixel, every operation rounded
 * once in fp32, in this order:
 *   p0    as eod_ddim_step / eod_dpmpp_step form it (the same bits), for dpmpp with clip != 0 clamped as there
 *   s     = p0 of the block's first pixel, then + p0 of each further pixel of the block ROW BY ROW, LEFT TO RIGHT (sequential adds)
 *   mean  = s / (float)(f_c * f_c)                 -- f_c = 1: p0 / 1.0f
 *   lm    = lambda * m                             -- m = mask at the pixel, 1.0f with mask NULL
 *   p0c   = p0 - (lm * (mean - values))
 *   ddim:  x_prev = ((sqrtf(a_prev) * p0c) + dir_xt) + nz, dir_xt and nz as in eod_ddim_step (from e_t and noise);  pred_x0 = p0c
 *   dpmpp: D = d_prev ? (w_cur * p0c) + (w_prev * d_prev) : p0c;  x_next = (c_x * x) + (c_d * D);  pred_x0 = p0c (the next step's d_prev)
 * The order of the block sum is part of the contract: it does not depend on B, on pointer alignment, on the launch geometry or on whether
 * the tensor is a batch or a scene.  values is the observation on the full-resolution grid ([B or 1][C][H][W], values_b1 != 0: one for all
 * samples); mask NULL or [B or 1][C or 1][H][W] (mask_b1 / mask_c1 != 0: broadcast), 1 = observed, 0 = free.  With values and mask constant
 * on every block and mask in {0, 1}, lambda = 1 this is the projection: afterwards the block means of pred_x0 are values (to rounding).
 * EOD_EINVAL with nothing launched: a null x / e_t / values / output / factors, C > 32, a factor outside 1..8 or one that does not divide
 * H and W, a outside (0, 1], lambda outside [0, 1] (NaN included), an output overlapping values, mask, d_prev or the other output.
 * One launch per factor that occurs.  16-byte accesses (f = 4, 8, and f = 1 where H * W % 4 == 0) or 8-byte ones (f = 2, 6) where every
 * pointer is 16-byte aligned, element by element otherwise and for odd f: same arithmetic.  Nothing is read or written outside a plane. */
int eod_ddim_step_obs(const float* x, const float* e_t, const float* noise, float a_t, float a_prev, float sigma_t, float sqrt_1m_at,
                      float temperature, const float* values, const float* mask, float lambda, const int32_t* factors, int B, int C,
                      int H, int W, int values_b1, int mask_b1, int mask_c1, float* x_prev, float* pred_x0, void* stream);
int eod_dpmpp_step_obs(const float* x, const float* e_t, const float* d_prev, float a_s, float sqrt_1m_as, float c_x, float c_d,
                       float w_cur, float w_prev, int clip, const float* values, const float* mask, float lambda, const int32_t* factors,
                       int B, int C, int H, int W, int values_b1, int mask_b1, int mask_c1, float* x_next, float* pred_x0, void* stream);
/* the operator alone: out = A+ A x, every pixel replaced by its block's mean (s and mean as above, of x itself); out must not overlap x */
int eod_block_mean(const float* x, const int32_t* factors, float* out, int B, int C, int H, int W, void* stream);
/* section 9.5's projection of a GIVEN prediction p [B][C][H][W] (a link of a chain of observations): s, mean, lm as above with p in place
 * of p0, out = p - (lm * (mean - values)).  Refusals as above; out must not overlap p, values or mask. */
int eod_obs_project(const float* p, const float* values, const float* mask, float lambda, const int32_t* factors, int B, int C, int H, int W,
                    int values_b1, int mask_b1, int mask_c1, float* out, void* stream);
/* Cross-band observations (no reference line): what is observed is K linear mixes of the C channels' f x f block
 * means, A = R (x) D_f: D_f the mean over f x f blocks anchored at the plane's origin, R [K][C] of full row rank.  A+ = G (x) replication
 * with G = pinv(R) [C][K].  R and G are HOST arrays (row-major fp32, the values the arithmetic uses: G is computed by the caller in float64
 * and rounded once), read during the call and handed to the kernel by value: nothing is allocated, copied or synchronised, the calls can be
 * captured in a graph.  Per pixel i, every operation rounded once in fp32, in this order:
 *   p0_c   as eod_ddim_step / eod_dpmpp_step form it (the same bits), for dpmpp with clip != 0 clamped as there
 *   mean_c = the block mean of section 9.5 of channel c over blk(i): the same first pixel, the same ROW BY ROW, LEFT TO RIGHT order of the
 *            sequential adds, / (float)(f * f)      -- f = 1: p0_c / 1.0f
 *   d_k    = R[k][0] * mean_0;  then for c = 1 .. C-1 in order:  d_k = d_k + (R[k][c] * mean_c)           (k = 0 .. K-1)
 *   r_k    = d_k - values_k(i)
 *   t_c    = G[c][0] * r_0;     then for k = 1 .. K-1 in order:  t_c = t_c + (G[c][k] * r_k)
 *   lm     = lambda * m(i)                          -- m = mask at the pixel, 1.0f with mask NULL
 *   p0c_c  = p0_c - (lm * t_c)
 *   the update from p0c as in eod_ddim_step_obs / eod_dpmpp_step_obs;  pred_x0 = p0c
 * Only the K rows of R and the K columns of G take part: there is no term for k >= K.  This is a property of the block alone: it does not
 * depend on B, on pointer alignment, on the launch geometry or on whether the tensor is a batch or a scene.  values [B or 1][K][H][W]
 * (values_b1 != 0: one for all samples) is what the other sensor saw, replicated onto the full-resolution grid; mask NULL or
 * [B or 1][1][H][W] (mask_b1 != 0: one for all samples), one mask for all K rows.  The formula is computed for ANY values and mask; with
 * both constant on every block, mask in {0, 1} and lambda = 1 it is the range / null-space projection of DDNM: afterwards R times the block
 * means of pred_x0 is values (to rounding) on the observed blocks.
 * EOD_EINVAL with nothing launched: a null x / e_t / values / R / G / output, K outside 1 .. min(C, 8), C > 32, f outside 1..8 or not
 * dividing H and W, a outside (0, 1], lambda outside [0, 1] (NaN included), an output overlapping ANY input or the other output.
 * ONE launch.  Access widths as for eod_ddim_step_obs; beyond EOD_SPEC_GRID_BLOCKS blocks of 256 threads the threads stride over the plane. */
#define EOD_SPEC_GRID_BLOCKS 4096
int eod_ddim_step_spec(const float* x, const float* e_t, const float* noise, float a_t, float a_prev, float sigma_t, float sqrt_1m_at,
                       float temperature, const float* values, const float* mask, float lambda, const float* R, const float* G, int K, int f,
                       int B, int C, int H, int W, int values_b1, int mask_b1, float* x_prev, float* pred_x0, void* stream);
int eod_dpmpp_step_spec(const float* x, const float* e_t, const float* d_prev, float a_s, float sqrt_1m_as, float c_x, float c_d, float w_cur,
                        float w_prev, int clip, const float* values, const float* mask, float lambda, const float* R, const float* G, int K,
                        int f, int B, int C, int H, int W, int values_b1, int mask_b1, float* x_next, float* pred_x0, void* stream);
/* the same projection of a GIVEN prediction p [B][C][H][W] (mean_c of p itself): out = p0c.  out must not overlap p, values or mask. */
int eod_spec_project(const float* p, const float* values, const float* mask, float lambda, const float* R, const float* G, int K, int f, int B,
                     int C, int H, int W, int values_b1, int mask_b1, float* out, void* stream);
/* the operator alone: out [B][K][H][W] = d_k of x [B][C][H][W] on the full-resolution grid (mean_c of x itself); out must not overlap x */
int eod_spec_apply(const float* x, const float* R, int K, int f, float* out, int B, int C, int H, int W, void* stream);
/* The ends of a chain of observations: a prediction is formed, projected by one link after the other (eod_spec_project, eod_obs_project),
 * and the update uses the result.  eod_pred_x0: p0 = (x - (sqrt_1m_a * e_t)) / sqrtf(a), clip != 0: clamped to [-1, 1] -- the p0 of
 * eod_ddim_step (clip = 0) / eod_dpmpp_step.  eod_ddim_step_p0: x_prev = ((sqrtf(a_prev) * p0c) + dir_xt) + nz as in eod_ddim_step (which
 * reads e_t and noise, not x).  eod_dpmpp_step_p0: D = d_prev ? (w_cur * p0c) + (w_prev * d_prev) : p0c; x_next = (c_x * x) + (c_d * D).
 * pred_x0 -> ONE projection -> step_p0 has the bits of the fused kernel (_obs / _spec) on the same inputs.  [numel] fp32 tensors.
 * EOD_EINVAL with nothing launched: a null tensor (noise / d_prev may be NULL), numel <= 0, a outside (0, 1], the output overlapping an input. */
int eod_pred_x0(const float* x, const float* e_t, float a, float sqrt_1m_a, int clip, float* p0, int64_t numel, void* stream);
int eod_ddim_step_p0(const float* e_t, const float* p0c, const float* noise, float a_prev, float sigma_t, float temperature, float* x_prev,
                     int64_t numel, void* stream);
int eod_dpmpp_step_p0(const float* x, const float* p0c, const float* d_prev, float c_x, float c_d, float w_cur, float w_prev, float* x_next,
                      int64_t numel, void* stream);
/* The clipped DDPM step of eod_ddpm_step cut where its data prediction is complete (no reference line for the cut):
 * the ancestral samplers form the prediction, project it by the links of an observation (eod_obs_project, eod_spec_project, eod_psf_*) and
 * finish the posterior step from the result.  Tensors [N][chw] fp32, t int64 [N] and the tables [T] on the device as for eod_ddpm_step; a
 * timestep outside [0, T) fills that sample's output with NaN.  Per element, every operation rounded once in fp32, in this order:
 *   eod_ddpm_pred_x0:
 *     c_x0 = sqrtf(1.0f / acp_t);  c_pred = sqrtf(1.0f / acp_t - 1.0f)
 *     u = c_x0 * x;  v = c_pred * e;  p0 = u - v
 *     clip != 0:  p0 = clamp(p0, -1, 1)                                      -- eod_ddpm_step's clamp: fminf(fmaxf(p0, -1), 1), a NaN stays NaN
 *   eod_ddpm_step_p0:
 *     all_pos = (min over the batch of t) > 0                                -- the reference's batch-wide branch, as eod_ddpm_step
 *     all_pos:  m_x0 = beta_t * sqrtf(acp_prev) / (1 - acp_t);  m_xt = (1 - acp_prev) * sqrtf(alpha_t) / (1 - acp_t)
 *               std  = sqrtf(beta_t * (1 - acp_prev) / (1 - acp_t));         mean = (m_x0 * p0c) + (m_xt * x)
 *     else:     m_x0 = beta_t / (1 - acp_t);  std = 0;                       mean = m_x0 * p0c
 *     out = mean + (std * z)
 * eod_ddpm_step_p0(eod_ddpm_pred_x0(x, e, clip = 1)) has the bits of eod_ddpm_step(clip = 1).  With clip = 0 the pair is the same posterior
 * form without the clamp: algebraically the reference's epsilon form (model.py:101-122), NOT bit-equal to eod_ddpm_step(clip = 0).
 * EOD_EINVAL with nothing launched: a null pointer, N, chw or T <= 0, the output overlapping an input (a tensor, t or a table).  16-byte
 * accesses where chw % 4 == 0 and every tensor pointer is 16-byte aligned, element by element otherwise: same arithmetic.  Nothing is
 * allocated, copied or synchronised: the calls can be captured in a graph.  The bodies are csrc/ddpm_p0_body.h. */
int eod_ddpm_pred_x0(const float* x_t, const float* pred, const int64_t* t, const float* acp, float* p0, int N, int64_t chw, int T, int clip,
                     void* stream);
int eod_ddpm_step_p0(const float* x_t, const float* p0c, const float* noise, const int64_t* t, const float* betas, const float* alphas,
                     const float* acp, float* out, int N, int64_t chw, int T, void* stream);
/* Prediction targets other than the noise (a model output read as x0 or as v; DESIGN.md sections 8.2 and 9.16): the three entry points
 * are declared, with their operations, in eodiff_param.h, which this header includes.  They are part of this ABI revision. */
#include "eodiff_param.h"
/* Learned variance (a model output of 2 C channels, mean half and variance half; DESIGN.md sections 8.3 and 9.17): the entry points of the
 * ancestral step and of the hybrid loss are declared, with their operations, in eodiff_var.h.  They only add to this ABI revision. */
#include "eodiff_var.h"
/* Dynamic thresholding (Saharia et al. 2022; no reference line): the data prediction is clamped to the sample's own
 * q-quantile of |p| and rescaled, where the static clamp of the entries above saturates.  p and out [B][n] fp32, s_out [B] fp32 on the
 * device; sample b is the n elements at p + b * n (64-bit indexing: B * n may exceed 2^31).  Per sample, every operation rounded once in
 * fp32:
 *     key(x) = bits(x) & 0x7fffffff              as an unsigned integer (|x|; NaNs rank above +inf)
 *     a_(0) <= a_(1) <= ... <= a_(n-1)           the sample's keys in ascending order: an EXACT order statistic (radix selection)
 *     lo = float(a_(k));  hi = float(a_(min(k + 1, n - 1)))
 *     v  = (frac == 0) ? lo : lo + (frac * (hi - lo))
 *     s  = fminf(fmaxf(v, 1.0f), cap)            (a NaN v gives s = 1: the static clamp)
 *     out[i] = fminf(fmaxf(p[i], -s), s) / s     (IEEE division; a NaN element becomes -1 HERE -- the static clamp of the step kernels keeps it)
 *     s_out[b] = s
 * The caller computes k and frac from the quantile q: pos = q * (n - 1) in float64, k = floor(pos), frac = fp32(pos - k).
 * Consequences: where v <= 1, s = 1 and out has the bits of the static clamp of a p without NaN (division by 1 is exact), so
 * eod_pred_x0(clip = 0) -> eod_dyn_threshold -> eod_*_step_p0 then has the bits of the clipped fused step; and the operator is idempotent:
 * |out| <= 1, so a second application has s = 1 and returns the same bits.
 * The result is a function of the sample's data, n, k, frac and cap alone: not of B, the pointers' alignment, the launch geometry or what
 * the workspace held (all counters are integers; the call clears them itself, on the stream).  ws: caller-owned DEVICE workspace of at
 * least eod_dyn_threshold_workspace_size(B, n) bytes (-1 for B <= 0 or n outside 1 .. 2^31 - 1), any alignment, private layout, reusable
 * from call to call.  One clear, four reading passes over p and the apply pass; 16-byte accesses where n % 4 == 0 and p / out are 16-byte
 * aligned, element by element otherwise: same bits.  Nothing is allocated, copied to or from the host, or synchronised: the call can be
 * captured in a graph.
 * EOD_EINVAL with nothing launched and the outputs untouched: a null pointer, B <= 0, n <= 0 or n > 2^31 - 1, k outside [0, n - 1], frac
 * outside [0, 1) (NaN included), cap < 1 or NaN (+inf is allowed), a workspace that is too small, out / s_out / ws overlapping p or each
 * other. */
int64_t eod_dyn_threshold_workspace_size(int B, int64_t n);
int eod_dyn_threshold(const float* p, int64_t k, float frac, float cap, float* out, float* s_out, int B, int64_t n, void* ws,
                      int64_t ws_bytes, void* stream);
/* Image-quality metrics (inference.py:136-138 evaluates torchmetrics' PSNR / SSIM on the GPU).  Two operators over
 * pred [B][C][H][W] and ref [ref_B][C][H][W], ref_B = B or 1 (one truth against a stack), fp32 on the device, any 4-byte alignment, any W,
 * 64-bit indexing; where: null or [where_B][1][H][W] fp32, where_B = B or 1 -- a pixel is COUNTED iff its value != 0.0f (a NaN counts).
 * C <= 32.  Both images pass an affine on load, every operation below rounded once in float64 (-ffp-contract=off):
 *     p = (a * (double)pred[i]) + b;      t = (a * (double)ref[i]) + b
 *
 * eod_band_stats: band [B][C][8] and sample [B][3], float64, 8-byte aligned.  Over the counted pixels of (sample, band):
 *     band = { n, sum p, sum t, sum (p * p), sum (t * t), sum (p * t), sum ((p - t) * (p - t)), max |p - t| }
 *   and per counted pixel, with the SAME rounded products summed over the bands c = 0 .. C - 1 in ascending order:
 *     pp = sum_c p_c * p_c;   tt = sum_c t_c * t_c;   dot = sum_c p_c * t_c
 *     pp == 0 or tt == 0:  the pixel has no angle (sample[2] += 1)
 *     else  w = (pp * tt) - (dot * dot);  theta = atan2(sqrt(w > 0 ? w : 0), dot);  sample[0] += theta;  sample[1] += 1
 *   (bit-identical spectra: pp * tt and dot * dot are the same rounded product, theta is exactly 0; atan2 is well conditioned at 0 where
 *   acos(dot / (|p| |t|)) is not).  The maximum keeps a NaN: m = (d > m || d != d) ? d : m.  A NaN element therefore makes the sums and the
 *   maximum of its own (sample, band) NaN, and its sample's angle sum; nothing else.
 *   Order of the additions: a pixel belongs to chunk i / 2048 and there to thread (i % 2048) % 256; a thread adds its pixels in ascending
 *   order from 0.0; of the 256 thread sums x[0 .. 255] of a chunk, y[l] = ((x[l] + x[l + 32]) + ..) + x[l + 224] for l = 0 .. 31, and the 32 y
 *   meet by the butterfly y[l] = y[l] + y[l ^ 16], .. y[l] + y[l ^ 1]; the chunks of a sample are added from left to right from 0.0 in groups
 *   of 64, the group sums again in groups of 64, until one is left (up to 64 chunks: plainly left to right).  A function of (C, H, W) alone:
 *   not of B, the grid, the alignment or what the workspace held.
 *
 * eod_ssim: the window is taps[0 .. 2r] (HOST array of float64, read during the call), r = 0 .. 12, applied horizontally, then vertically,
 * WITHOUT padding: window position (y, x), y = 0 .. H - 2r - 1, x = 0 .. W - 2r - 1, covers rows y .. y + 2r and columns x .. x + 2r and has
 * its centre at (y + r, x + r).  (torchmetrics reflect-pads and crops the pad away again: the cropped map is this valid region.)  For each of
 * q = p, t, p * p, t * t, p * t (the products rounded in float64), taps in ascending order, one rounded multiply and one rounded add per tap:
 *     h_q[y'][x] = ((taps[0] * q[y'][x]) + taps[1] * q[y'][x + 1]) + ... + taps[2r] * q[y'][x + 2r]
 *     E_q[y][x]  = ((taps[0] * h_q[y][x]) + taps[1] * h_q[y + 1][x]) + ... + taps[2r] * h_q[y + 2r][x]
 *     mpp = Ep * Ep;  mtt = Et * Et;  mpt = Ep * Et;   spp = Epp - mpp;  stt = Ett - mtt;  spt = Ept - mpt
 *     ssim = (((2 * mpt) + c1) * ((2 * spt) + c2)) / (((mpp + mtt) + c1) * ((spp + stt) + c2))
 *   map: null, or [B][C][H][W] fp32: map[centre] = (float)ssim; the elements outside the valid region are not written.
 *   sums [B][C][2] float64, 8-byte aligned: { sum of ssim, n } over the positions whose CENTRE is counted by `where`.
 *   Order of the additions: position (y, x) belongs to tile (y / 32, x / 32) and there to thread ((y % 32) * 32 + x % 32) % 256; threads,
 *   then tiles (row-major) are added as above.  A function of (H, W, r) alone.
 *
 * ws: caller-owned DEVICE workspace of at least *_workspace_size(...) bytes (-1 for arguments the operator refuses), any alignment, private
 * layout, reusable: every slot is written before it is read.  No floating-point atomics; nothing is allocated, copied or synchronised: the
 * calls can be captured in a graph.  EOD_EINVAL with nothing launched and the outputs untouched: a null pointer (where and map may be null),
 * B, H or W <= 0, C outside 1 .. 32, ref_B or where_B neither B nor 1, a or b not finite, a float64 output that is not 8-byte aligned, a
 * workspace that is too small, outputs overlapping each other or the workspace; eod_ssim also: r outside 0 .. 12, H or W < 2r + 1, a tap,
 * c1 or c2 not finite, map overlapping an input.  The tile body of eod_ssim is csrc/ssim_body.h. */
int64_t eod_band_stats_workspace_size(int B, int C, int H, int W);
int eod_band_stats(const float* pred, const float* ref, const float* where, int B, int ref_B, int where_B, int C, int H, int W, double a,
                   double b, double* band, double* sample, void* ws, int64_t ws_bytes, void* stream);
int64_t eod_ssim_workspace_size(int B, int C, int H, int W, int r);
int eod_ssim(const float* pred, const float* ref, const float* where, int B, int ref_B, int where_B, int C, int H, int W, const double* taps,
             int r, double a, double b, double c1, double c2, float* map, double* sums, void* ws, int64_t ws_bytes, void* stream);
/* Ensemble statistics (no reference line): order statistics over the B members of a stack, 1 <= B <= 64.  One lane
 * owns one pixel at a time: the pixel's B members become order-preserving 32-bit keys (the sign bit of a non-negative float flipped, every
 * bit of a negative one; every NaN the top key), so the order is total, -inf < .. < -0.0 < +0.0 < .. < +inf < NaN, and are sorted in
 * registers by a fixed compare-exchange network padded to 1, 2, 4 .. 64 keys; the stack is read once.  x_(0) <= .. <= x_(B-1) below are the
 * sorted members; a NaN that is an order statistic comes back as the quiet NaN 0x7fc00000, every other member with its own bits.
 * A rank (k, frac), 0 <= k < B, 0 <= frac < 1, frac > 0 only with k + 1 < B, names the quantile
 *   frac == 0: x_(k) (no arithmetic);  else d = hi - lo, m = frac * d, v = lo + m with lo = x_(k), hi = x_(k+1), each rounded in fp32
 * (the form of eod_dyn_threshold).
 * eod_scene_quantiles: x [B][n] -> out [Q][n], out[j][i] = the quantile (k[j], frac[j]) of pixel i; 1 <= Q <= 8, k and frac host arrays
 * read during the call.  out must not overlap x.  One launch, no workspace, no host synchronisation.  16-byte accesses where n % 4 == 0,
 * both pointers are 16-byte aligned and B <= 16; element by element otherwise: the same bits.
 * eod_ensemble_stats: x [B][C][H][W] against one truth [C][H][W], 1 <= C <= 32; where: NULL or [H][W], a pixel counts iff its value is not
 * 0; L = 0 .. 4 central intervals, level_k [L][2] and level_frac [L][2] (host arrays) the ranks of the lower and the upper quantile.  Per
 * counted pixel of band c, in float64 on the converted members, y the truth:
 *   a = sum |x_(i) - y| and g = sum (2 i - B + 1) x_(i) (= sum over i < j of x_(j) - x_(i)) and s = sum x_(i), ascending i, left to right;
 *   m = s / B;  s2 = (sum (x_(i) - m)^2, ascending i) / (B - 1), 0 at B = 1;  crps = a / B - g / (B B);
 *   rank = members whose key is below the truth's key (0 .. B);  tie: a member's key equals the truth's;
 *   covered_l: q_lo <= y <= q_hi in fp32, the two quantiles formed as eod_scene_quantiles forms them.
 *   sums [C][5] (float64)               sum over the counted pixels of a / B, g / (B B), (m - y)^2, s2, m - y
 *   counts [C][2 + (B + 1) + L] (int64)  counted pixels, ties, the rank histogram, covered pixels per level
 *   crps_map [C][H][W] (fp32) or NULL   (float)crps at a counted pixel, NaN elsewhere
 * The float64 sums follow eod_band_stats: no floating-point atomics, every thread adds its pixels in ascending order, a workgroup its
 * threads in a fixed order, the workgroups' slots are added left to right; which pixels a thread and a workgroup own depends on H * W
 * alone, so a band of a C-band call has the bits of its single-band call.  The counts use integer atomics.  The call clears what it
 * accumulates into: the contents of the workspace and of the outputs before the call do not matter.  No host synchronisation
 * (graph-capturable).  A NaN in a band's members or truth propagates into that band's sums and into no other band; the counts stay defined
 * through the keys.  eod_ensemble_stats_workspace_size: bytes of ws (any alignment), -1 for arguments the call refuses. */
int eod_scene_quantiles(const float* x, float* out, int B, int64_t n, const int32_t* k, const float* frac, int Q, void* stream);
int64_t eod_ensemble_stats_workspace_size(int B, int C, int H, int W);
int eod_ensemble_stats(const float* x, const float* truth, const float* where, int B, int C, int H, int W, const int32_t* level_k,
                       const float* level_frac, int L, double* sums, int64_t* counts, float* crps_map, void* ws, int64_t ws_bytes,
                       void* stream);
/* PSF-aware observations (no reference line): the K channels `channels` (strictly increasing) of p [B][C][H][W] are
 * observed through A = D_f N^-1 B0 -- B0 the zero-padded separable convolution with the 1-D taps h[0 .. 2r] (r = 0 .. 12; fp32, finite,
 * non-negative, bitwise symmetric, h[r] > 0), horizontally, then vertically; N = diag(B0 1); D_f the f x f block mean of section 9.5 -- on
 * the COARSE grid [H / f][W / f].  taps and channels are HOST arrays read during the call and handed to the kernels by value: nothing is
 * allocated, copied or synchronised, the calls can be captured in a graph.  Per pixel, every operation rounded once in fp32 (u outside the
 * plane is +0.0f, and its product is formed and added like any other):
 *   conv_h(u)[y][x] = (((h[0] * u[y][x-r]) + h[1] * u[y][x-r+1]) + ...) + h[2r] * u[y][x+r]       taps in ascending order
 *   conv_v likewise along y;   blur(u) = conv_v(conv_h(u))                                        horizontal first, always
 *   nh[x] = conv_h of a row of 1.0f;  nv[y] likewise;  n[y][x] = nv[y] * nh[x]
 *   b       = blur(p_c) / n
 *   mean    = section 9.5's block sum of b (first pixel, then row by row, left to right) / (float)(f * f)
 *   q       = lm * (mean - values),   lm = lambda * m   (mask NULL: m = 1.0f)                     coarse grid
 *   w[y][x] = (q[y / f][x / f] * step) / n[y][x]
 *   out_c   = p_c - blur(w)                              channels not listed: out_c = p_c
 * The order is a property of the pixel alone: it does not depend on B, on pointer alignment, on the tile or the launch geometry or on
 * whether the tensor is a batch or a scene.  With h = {1.0f} and step = 1.0f, values / mask being what section 9.5 replicates, out has
 * the bits of eod_obs_project.  With lambda = 0 or mask = 0 a finite p gives out = p.  A^T q = B0((replicate(q) / f^2) / n) because h is
 * symmetric; with step = tau / f^2, tau <= 1 / ||A||^2, residual + update is one non-expansive Landweber step p - lambda tau A^T(m (A p - y)).
 * eod_psf_residual: q [B][K][H/f][W/f] from p, values [B or 1][K][H/f][W/f] and mask NULL or [B or 1][K or 1][H/f][W/f] (the _b1 / _c1
 * flags != 0: broadcast).  eod_psf_apply: out [B][K][H/f][W/f] = mean, the operator alone.  eod_psf_update: out [B][C][H][W] from p and q.
 * EOD_EINVAL with nothing launched: a null pointer (mask may be NULL), C > 32, K outside 1 .. C, channels not strictly increasing or out of
 * range, r outside 0 .. 12, f outside 1 .. 8 or not dividing H and W, taps breaking the rules above, lambda outside [0, 1] (NaN included),
 * step not finite or <= 0, an output overlapping any input (eod_psf_update reads a tile's halo of p after the neighbours have written).
 * One launch each; 16-byte accesses of the full-resolution tensors where W % 4 == 0 and their pointers are 16-byte aligned, of the coarse
 * ones where W / f % 4 == 0 and theirs are, element by element otherwise: same arithmetic.  Beyond EOD_PSF_GRID_BLOCKS workgroups the
 * workgroups stride over the (plane, tile) pairs.  Nothing is read or written outside a plane. */
#define EOD_PSF_GRID_BLOCKS 4096
int eod_psf_residual(const float* p, const float* values, const float* mask, float lambda, const float* taps, int r, int f,
                     const int32_t* channels, int K, int B, int C, int H, int W, int values_b1, int mask_b1, int mask_c1, float* q, void* stream);
int eod_psf_apply(const float* x, const float* taps, int r, int f, const int32_t* channels, int K, float* out, int B, int C, int H, int W,
                  void* stream);
int eod_psf_update(const float* p, const float* q, float step, const float* taps, int r, int f, const int32_t* channels, int K, int B, int C,
                   int H, int W, float* out, void* stream);
/* Cross-band PSF observations (no reference line): K bands, each a known linear mix R [K][C] of the C channels of
 * p [B][C][H][W], seen through ONE operator A_s = D_f N^-1 B0 (the taps, f and contract of the block above) under ONE coarse mask:
 * A = R (x) A_s.  R [K][C] and G [C][K] are HOST arrays of finite fp32 read during the call and handed to the kernels by value like the
 * taps: nothing is allocated, copied or synchronised, the calls can be captured in a graph.  Per pixel, every operation rounded once in
 * fp32, the order a property of the pixel alone (not of B, the alignment, the tile, the launch geometry, batch or scene):
 *   u_k[y][x] = R[k][0] * p_0[y][x];  then for c = 1 .. C-1 in order:  u_k = u_k + (R[k][c] * p_c[y][x])     in-plane; outside the plane +0.0f
 *   b = blur(u_k) / n;  mean = block sum of b / (float)(f * f);  q_k = lm * (mean - values_k),  lm = lambda * m      (the lines above, unchanged)
 *   s_c[Y][X] = G[c][0] * q_0[Y][X];  then for k = 1 .. K-1 in order:  s_c = s_c + (G[c][k] * q_k[Y][X])     coarse grid
 *   w[y][x]   = (s_c[y / f][x / f] * step) / n[y][x];   out_c = p_c - blur(w)                                 (the lines above, unchanged)
 * Every product is formed, zeros of R or G included; eod_psf_update_mix writes every channel (a zero row of G: out_c = p_c - blur(0) = p_c
 * for finite q).  With the rows of R rows of the identity and G = R^T the pair has the bits of eod_psf_residual / eod_psf_update with that
 * channel list.  eod_psf_residual_mix: q [B][K][H/f][W/f] from p, values [B or 1][K][H/f][W/f], mask NULL or [B or 1][1][H/f][W/f] (one mask
 * for all K bands).  eod_psf_apply_mix: out [B][K][H/f][W/f] = mean, the operator alone.  eod_psf_update_mix: out [B][C][H][W] from p and
 * q [B][K][H/f][W/f].  With G = pinv(R), q the result of eod_psf_cg on the K residual planes (shared mask) and step = fp32(1 / f^2) the
 * triple is the exact projection onto {M A p = M values}: M A A^T M = (R R^T) (x) (M_s G_s M_s) factorises plane by plane.
 * EOD_EINVAL with nothing launched: the refusals of eod_psf_residual / eod_psf_update, K outside 1 .. min(C, 8), C > 32, R / G null or
 * with a non-finite entry.  One launch each; the access forms and the striding are those of the block above. */
int eod_psf_residual_mix(const float* p, const float* values, const float* mask, float lambda, const float* taps, int r, int f,
                         const float* R, int K, int B, int C, int H, int W, int values_b1, int mask_b1, float* q, void* stream);
int eod_psf_apply_mix(const float* x, const float* taps, int r, int f, const float* R, int K, float* out, int B, int C, int H, int W,
                      void* stream);
int eod_psf_update_mix(const float* p, const float* q, float step, const float* taps, int r, int f, const float* G, int K, int B, int C,
                       int H, int W, float* out, void* stream);
/* Anisotropic and shifted PSFs (no reference line): A = D_f N^-1 B0 as above with B0 = B_y B_x built from TWO tap
 * vectors, hx[0 .. 2 rx] along x and hy[0 .. 2 ry] along y; rx and ry independent, each 0 .. 12; each vector fp32, finite, non-negative,
 * NOT necessarily symmetric, centre tap positive (hx[rx] > 0, hy[ry] > 0: n > 0 on every line, however short).  h[t] weights the scene
 * pixel at offset t - r: mass at t > r means "this sample sees the scene to its right / below".  Per pixel, every operation rounded once in
 * fp32 (u outside the plane is +0.0f, and its product is formed and added like any other):
 *   conv_x(u; h, r)[y][x] = (((h[0] * u[y][x-r]) + h[1] * u[y][x-r+1]) + ...) + h[2r] * u[y][x+r]      taps in ascending order
 *   conv_y likewise along y;   blur(u) = conv_y(conv_x(u; hx, rx); hy, ry)                             horizontal first, always
 *   nh[x] = conv_x of a row of 1.0f with hx;  nv[y] = conv_y of a column of 1.0f with hy;  n[y][x] = nv[y] * nh[x]
 *   b = blur(p_c) / n;   mean = section 9.5's block sum of b / (float)(f * f);   q = lm * (mean - values),  lm = lambda * m
 *   w[y][x] = (s[y / f][x / f] * step) / n[y][x]                                                        n from the FORWARD taps
 *   out_c   = p_c - conv_y(conv_x(w; hx~, rx); hy~, ry),   hx~[t] = hx[2 rx - t],  hy~[t] = hy[2 ry - t]
 * (horizontal first, the reversed taps in ascending order of the reversed array): B0^T is the correlation with the reversed taps.  With
 * hx == hy bitwise symmetric these are the lines of the two blocks above, and the results have the bits of eod_psf_residual / eod_psf_apply /
 * eod_psf_update (and of the _mix triple).  The order is a property of the pixel alone (not of B, the alignment, the tile, the launch
 * geometry, batch or scene).  A non-finite p pixel reaches exactly the outputs within (ry, rx) of it: the shorter vector is never padded.
 * taps_y / taps_x are the FORWARD taps (HOST arrays, by value to the kernels); eod_psf_update_xy reverses them itself.  Each entry point
 * serves the plain and the mixed form: EXACTLY ONE of `channels` (K strictly increasing channel numbers, as in the first block) and the
 * matrix (R [K][C] / G [C][K], as in the second; u_k, s_c and the one coarse mask as there) is non-NULL.
 * EOD_EINVAL with nothing launched and the outputs untouched: every refusal of the entry points above except tap symmetry; both or neither
 * of channels and the matrix; with R: mask_c1 == 0, K > 8.  One launch each, nothing allocated, copied or synchronised; the tile, the
 * access forms and the striding are those of the first block; a tile stages ft + 2 ry rows of ft + 2 rx columns. */
int eod_psf_residual_xy(const float* p, const float* values, const float* mask, float lambda, const float* taps_y, int ry, const float* taps_x,
                        int rx, int f, const int32_t* channels, const float* R, int K, int B, int C, int H, int W, int values_b1, int mask_b1,
                        int mask_c1, float* q, void* stream);
int eod_psf_apply_xy(const float* x, const float* taps_y, int ry, const float* taps_x, int rx, int f, const int32_t* channels, const float* R,
                     int K, float* out, int B, int C, int H, int W, void* stream);
int eod_psf_update_xy(const float* p, const float* q, float step, const float* taps_y, int ry, const float* taps_x, int rx, int f,
                      const int32_t* channels, const float* G, int K, int B, int C, int H, int W, float* out, void* stream);
/* The exact PSF data consistency (no reference line): conjugate gradients on the COARSE grid [Hc][Wc] = [H / f][W / f],
 * one independent system per plane (sample b, observed channel k):
 *   S z = c,   S = M G M + mu I,   M = diag(m), m in {0, 1} (mask NULL: 1),   G = A A^T = G_H (x) G_W
 * gy [Hc][2b + 1] and gx [Wc][2b + 1] are DEVICE fp32 tables of the banded symmetric 1-D Gram matrices G_L = A1(L) A1(L)^T, entry [i][j] =
 * G_L[i][i - b + j], zero where the column lies outside the line; b = 0 .. 24.  One application, every operation rounded once in fp32 (u
 * outside the plane is +0.0f, and its product is formed and added like any other):
 *   u       = m * d                                                               (mask NULL: u = d)
 *   t[y][x] = (((gx[x][0] * u[y][x-b]) + gx[x][1] * u[y][x-b+1]) + ...) + gx[x][2b] * u[y][x+b]
 *   v[y][x] = (((gy[y][0] * t[y-b][x]) + gy[y][1] * t[y-b+1][x]) + ...) + gy[y][2b] * t[y+b][x]
 *   q       = (m * v) + (mu * d)                                                  (mask NULL: v + (mu * d))
 * q is a function of the pixel alone.  sigma[plane] = <d, q>: the fp32 x fp32 products are exact in float64 and are added in float64, each
 * tile of 32 x 32 in a fixed order into a slot indexed by (plane, tile), the slots of a plane in a fixed tree over the tile index -- a plane's
 * total depends on that plane's data and on Hc, Wc alone, not on B, K, the alignment, the grid or the other planes of the launch.
 * eod_psf_cg runs `iters` = 1 .. 64 iterations from z = 0, r = d = c, rho = <r, r>:
 *   q = S d;  sigma = <d, q>;  alpha = fp32(rho / sigma);  z = z + (alpha * d);  r = r - (alpha * q);  rho' = <r, r>;
 *   beta = fp32(rho' / rho);  d = r + (beta * d);  rho = rho'
 * with alpha = beta = 0 for a plane whose rho is 0, whose sigma is <= 0 or where either is not finite (and beta = 0 where rho' is not
 * finite), and writes q_out = lambda * (m * z), ready for eod_psf_update with step = fp32(1 / f^2).  A plane with c = 0 keeps z = 0.
 * ws: caller-owned DEVICE workspace of at least eod_psf_cg_workspace_size(B, K, Hc, Wc) bytes, any alignment, private layout.
 * eod_psf_gram: q [B][K][Hc][Wc] and sigma (double [B * K], 8-byte aligned) from d.  eod_psf_cg: 4 iters + 2 launches in one call.
 * EOD_EINVAL with nothing launched: a null pointer (mask may be NULL), B, K, Hc or Wc <= 0, b outside 0 .. 24, iters outside 1 .. 64, mu
 * negative or not finite, lambda outside [0, 1] (NaN included), a workspace that is too small, an output or the workspace overlapping an
 * input or each other.  Nothing is allocated, copied or synchronised: the calls can be captured in a graph.  16-byte accesses where
 * Wc % 4 == 0 and the pointers are 16-byte aligned, element by element otherwise: same bits.  Beyond EOD_PSF_GRID_BLOCKS workgroups the
 * workgroups stride over the (plane, tile) pairs. */
int64_t eod_psf_cg_workspace_size(int B, int K, int Hc, int Wc);
int eod_psf_gram(const float* d, const float* mask, float mu, const float* gy, const float* gx, int b, int B, int K, int Hc, int Wc,
                 int mask_b1, int mask_c1, float* q, double* sigma, void* ws, int64_t ws_bytes, void* stream);
int eod_psf_cg(const float* c, const float* mask, float mu, float lambda, const float* gy, const float* gx, int b, int iters, int B, int K,
               int Hc, int Wc, int mask_b1, int mask_c1, float* q_out, void* ws, int64_t ws_bytes, void* stream);
/* classifier-free guidance of p_sample_ddim (ddim.py:177-181): out = e_uncond + scale * (e_cond - e_uncond) */
int eod_cfg_combine(const float* e_uncond, const float* e_cond, float scale, float* out, int64_t numel, void* stream);
/* table-driven DDPM step of the LDM-derived sampler: DDPM.p_sample ddpm.py:248-255 with predict_start_from_noise :221-225,
 * q_posterior :227-234 (tables of register_schedule :122-162, fp32 [T]); noise masked per sample at t == 0.  t outside [0, T): NaN. */
int eod_ldm_p_sample(const float* x, const float* eps, const float* noise, const int64_t* t, const float* sqrt_recip_acp,
                     const float* sqrt_recipm1_acp, const float* post_coef1, const float* post_coef2,
                     const float* post_logvar, float* out, int N, int64_t chw, int T, int clip, void* stream);
/* k15: counter-based N(0,1): Philox4x32-10 keyed by seed, counter = (element/4, sample0+n, step, stream_id)
 * -> results are invariant to how samples are sharded over ranks. */
int eod_randn_philox(float* out, int N, int64_t chw, uint64_t seed, int64_t sample0, int32_t step,
                     int32_t stream_id, void* stream);
/* RePaint resampling, the forward move between two levels a < b of a chain (q(x_b | x_a) collapsed over the b - a single steps):
 *   out = ca * x + cb * z,  r = acp_to / acp_from,  ca = sqrtf(r),  cb = sqrtf(1.0f - r),  every operation rounded separately in fp32.
 * acp_from / acp_to are the cumulative alpha products of the level left and the level reached (entries of alphas_cumprod for DDPM,
 * of ddim_alphas for DDIM), shared by all N samples; 0 < acp_to <= acp_from, else EOD_EINVAL and nothing is launched.
 * noise != NULL: z is read from noise [N][CHW].  noise == NULL: z is generated in registers, bit for bit what eod_randn_philox
 * writes for (seed, sample0 + n, step, stream_id), and never passes through memory.  out must not alias x.
 * 16-byte accesses where chw % 4 == 0 and the pointers are 16-byte aligned, element by element otherwise: same arithmetic. */
int eod_renoise(const float* x, const float* noise, float acp_from, float acp_to, float* out, int N, int64_t chw,
                uint64_t seed, int64_t sample0, int32_t step, int32_t stream_id, void* stream);

/* Whole-scene sampling (csrc/scene.hip; plan = eo_diffusion_amd/tiling.py TilePlan).  Tiles are s x s, numbered row-major
 * i = iy * ntx + ix; tile (iy, ix) has its top-left corner at (origins_y[iy], origins_x[ix]).  origins_* are DEVICE int32 arrays,
 * non-decreasing, every origin + s inside the scene; wy [nty][s] / wx [ntx][s] are DEVICE fp32 per-axis weight tables whose
 * covering entries sum to one at every coordinate.  fp32, NCHW like every sampler tensor.
 *   eod_scene_gather  tiles[i][c][ly][lx] = scene[c][origins_y[iy] + ly][origins_x[ix] + lx]          (bit-exact copy)
 *   eod_scene_blend   scene[c][y][x] = sum over the tiles covering (y, x), in ascending (iy, ix), of
 *                     (wy[iy][y - oy] * wx[ix][x - ox]) * tiles[i][c][y - oy][x - ox]: each product rounded once to fp32, the sum
 *                     taken left to right in fp32, no atomics -- a pure function of the inputs, whatever the launch geometry.
 * A tile whose origin lies outside the scene is NaN-filled by the gather, a pixel no tile covers is NaN in the blend (neither reads
 * outside its buffers).  16-byte accesses where W, s, the origins and the pointers allow, scalar otherwise (odd W, odd origins). */
int eod_scene_gather(const float* scene, float* tiles, int C, int H, int W, int s, const int32_t* origins_y,
                     const int32_t* origins_x, int nty, int ntx, void* stream);
int eod_scene_blend(const float* tiles, float* scene, const float* wy, const float* wx, const int32_t* origins_y,
                    const int32_t* origins_x, int C, int H, int W, int s, int nty, int ntx, void* stream);

/* A tile SUBSET of the same plan (tiling.py TileSubset): the tiles whose window holds a hole pixel of a RePaint mask, the only ones
 * whose estimate the next mix does not throw away.  A value of the mask is a hole when it is != 1.0f (soft values and NaN included).
 * `index` [n_list] DEVICE int32: the listed tiles, ascending; tiles [n_list][C][s][s] holds them in that order (slot k = tile
 * index[k]); `slot_of` [nty * ntx] DEVICE int32: the slot of each tile, -1 = not listed.  1 <= n_list <= nty * ntx.  A pixel is
 * ESTIMATED when it is covered and every tile covering it is listed.
 *   eod_scene_tile_active   active[i] = 1 iff any of the Cm x s x s values of mask [Cm][H][W] in tile i's window is != 1.0f, else 0;
 *                           every entry is written (one block-level reduction per tile, stored by one lane).
 *   eod_scene_gather_list   tiles[k] = the window of tile index[k] (bit-exact copy).
 *   eod_scene_blend_list    at an estimated pixel eod_scene_blend's sum on tiles[slot_of[i]]: same products, same left-to-right order
 *                           in ascending i, same roundings; 0.0f at every other pixel.  Every scene element is written.
 *   eod_scene_keep_known    out = x at estimated pixels, known elsewhere (x, known, out [C][H][W]).
 * The tables are never trusted with an address: an index outside [0, nty * ntx) gives a NaN tile, a slot outside [0, n_list) counts as
 * not listed (the device arrays cannot be checked on the host without a synchronisation; the counts are, before the launch). */
int eod_scene_tile_active(const float* mask, int32_t* active, int Cm, int H, int W, int s, const int32_t* origins_y,
                          const int32_t* origins_x, int nty, int ntx, void* stream);
int eod_scene_gather_list(const float* scene, float* tiles, int C, int H, int W, int s, const int32_t* origins_y,
                          const int32_t* origins_x, int nty, int ntx, const int32_t* index, int n_list, void* stream);
int eod_scene_blend_list(const float* tiles, float* scene, const float* wy, const float* wx, const int32_t* origins_y,
                         const int32_t* origins_x, const int32_t* slot_of, int n_list, int C, int H, int W, int s, int nty, int ntx,
                         void* stream);
int eod_scene_keep_known(const float* x, const float* known, const int32_t* slot_of, int n_list, const int32_t* origins_y,
                         const int32_t* origins_x, int C, int H, int W, int s, int nty, int ntx, float* out, void* stream);

/* A STACK of B scenes of one plan (tiling.py TileStack): the same four kernels with a leading scene dimension; the entry points above
 * are their B = 1 case.  scene / x / known / out are [B][C][H][W], mask is [B][Cm][H][W].  Tile i of scene b has the global number
 * g = b * nty * ntx + i; the full forms hold tiles [B * nty * ntx][C][s][s] in that order.  `index` [n_list] lists global numbers,
 * ascending; `slot_of` [B * nty * ntx] is the slot of each global tile or -1; 1 <= n_list <= B * nty * ntx.  A pixel of scene b is
 * ESTIMATED when every tile OF SCENE b covering it is listed.  The blend's arithmetic per scene is eod_scene_blend's, to the bit: a
 * scene's result does not depend on what else is in the stack.  The tables are trusted with no address, as above.
 *   eod_scene_stack_gather       index == NULL: every tile of every scene (n_list ignored); else tiles[k] = the window of tile index[k]
 *   eod_scene_stack_blend        slot_of == NULL: the full blend of every scene (n_list ignored); else the list blend, 0.0f where not estimated
 *   eod_scene_stack_tile_active  active [B * nty * ntx], one verdict per global tile from its own scene's mask
 *   eod_scene_stack_keep_known   out[b] = x[b] at scene b's estimated pixels, known[b] elsewhere */
int eod_scene_stack_gather(const float* scene, float* tiles, int B, int C, int H, int W, int s, const int32_t* origins_y,
                           const int32_t* origins_x, int nty, int ntx, const int32_t* index, int n_list, void* stream);
int eod_scene_stack_blend(const float* tiles, float* scene, const float* wy, const float* wx, const int32_t* origins_y,
                          const int32_t* origins_x, const int32_t* slot_of, int n_list, int B, int C, int H, int W, int s, int nty,
                          int ntx, void* stream);
int eod_scene_stack_tile_active(const float* mask, int32_t* active, int B, int Cm, int H, int W, int s, const int32_t* origins_y,
                                const int32_t* origins_x, int nty, int ntx, void* stream);
int eod_scene_stack_keep_known(const float* x, const float* known, const int32_t* slot_of, int n_list, const int32_t* origins_y,
                               const int32_t* origins_x, int B, int C, int H, int W, int s, int nty, int ntx, float* out, void* stream);
/* Per-element mean and sample standard deviation over the B members of a stack x [B][n] (K draws of one scene: n = C * H * W), one
 * pass, every operation separately rounded in fp32:
 *   s = x_0; s = s + x_b for ascending b;  mean = s / (float)B;  q = sum over ascending b of d * d with d = x_b - mean;
 *   std = sqrtf(q / (float)(B - 1));  B = 1: std = 0.  Division and square root are the correctly rounded ones (IEEE fp32:
 * the root is taken in fp64 and rounded, the device's own fp32 square root is 1 ulp).
 * 16-byte accesses where n % 4 == 0 and the three pointers are 16-byte aligned, element by element otherwise: same arithmetic.
 * (Member b starts at x + b * n: with n % 4 != 0 the members are misaligned against each other, so no split into a vector body
 * and a scalar tail gives every member 16-byte loads; the whole array then takes the scalar form.) */
int eod_scene_stats(const float* x, float* mean, float* std_out, int B, int64_t n, void* stream);

/* harness-side elementwise ops of inference.py, fp32, bit-exact vs the torch expressions:
 *   eod_repaint_cond   :100-109  cond [N][C+1][hw] = cat(image [N][C][hw], invert ? 1 - mask : mask), mask [N][1][hw]
 *   eod_postprocess    :128      mode 0: y = clip(x, 0, 1) (data in [0,1]);  mode 1: y = (x + 1) / 2 (data in [-1,1])
 *   eod_masked_preview :134      out = image * clip(mask + lift, 0, 1)   (lift = 0.7 in the reference)
 * clip is torch.clip: a NaN stays NaN (a NaN in the mask reaches every channel of its pixel) and -0 stays -0. */
int eod_repaint_cond(const float* image, const float* mask, float* cond, int N, int C, int64_t hw, int invert, void* stream);
int eod_postprocess(const float* x, float* y, int64_t numel, int mode, void* stream);
int eod_masked_preview(const float* image, const float* mask, float* out, int N, int C, int64_t hw, float lift, void* stream);

/* ------------------------------------------------------------------------------------------
 * Native executor: run a pre-built program (array of tagged descriptors) on one stream without
 * returning to the host language between launches (replaces the ~100-180 Python-dispatched
 * ATen launches per UNet forward).
 * ------------------------------------------------------------------------------------------ */
enum {
    EOD_OP_CONV = 1, EOD_OP_GEMM = 2, EOD_OP_GN_PARTIAL = 3, EOD_OP_GN_FINALIZE = 4,
    EOD_OP_GN_APPLY = 5, EOD_OP_SOFTMAX = 6, EOD_OP_TEMB = 7, EOD_OP_TO_NHWC = 8, EOD_OP_TO_NCHW = 9,
    EOD_OP_POOL = 10, EOD_OP_ATTN = 11,
    EOD_OP_TRANSPOSE = 12, /* eod_transpose_gather (training forward: transposed q|k|v for the attention GEMMs) */
    EOD_OP_ATTN_NAT = 13,  /* eod_attention_fwd_nat */
    EOD_OP_DROPOUT = 14,   /* eod_dropout (training forward) */
    EOD_OP_ACT_BOUND = 15, /* eod_act_bound */
    EOD_OP_BOUND_AFFINE = 16 /* eod_bound_affine */
};
typedef struct {
    const void* p[8];
    int64_t l[4];
    int32_t i[10];
    float f[2];
} eod_small_desc; /* argument pack of the small ops, field use documented in csrc/program.hip */
typedef struct {
    int32_t kind;
    int32_t _pad;
    union {
        eod_conv_desc conv;
        eod_gemm_desc gemm;
        eod_temb_desc temb;
        eod_attn_desc attn;
        eod_small_desc small;
    } u;
} eod_op;
int eod_program_run(const eod_op* ops, int n_ops, void* stream);
/* Measurement variant: brackets every op with HIP events recorded on `stream` (the stream the kernels run
 * on).  timer = eod_timer_create(n_ops, max_runs); after a stream sync, eod_timer_read() returns the number
 * of recorded runs and fills ms[n_ops] with each op's duration summed over those runs. */
void* eod_timer_create(int n_ops, int max_runs);
void eod_timer_destroy(void* timer);
int eod_timer_read(void* timer, float* ms);
/* bracket only the ops whose mask byte is non-zero (each event pair idles the stream for a few microseconds) */
int eod_timer_set_mask(void* timer, const unsigned char* mask, int n_ops);
int eod_program_run_timed(const eod_op* ops, int n_ops, void* stream, void* timer);
/* resblock_updown helpers (unet_openai.py:320-325): mode 0 = 2x2 average pool, 1 = nearest 2x,
 * 2 = 2x2 sum pool (backward of nearest 2x), 3 = nearest 2x times 0.25 (backward of the average pool), 4 = crop the last row
 * (pad_tl & 1) / column (pad_tl & 2) -- training path */
int eod_resample2x(const void* x, int dtype, int N, int H, int W, int C, int mode, int pad_tl, void* y,
                   void* stream);

/* ------------------------------------------------------------------------------------------
 * Training path (train.py:109-124: forward, nn.MSELoss, loss.backward(), AdamW.step(), EMA update).
 * The backward of every UNet block runs on the forward's MFMA kernels (see csrc/train.hip):
 *   backward-data    = eod_conv2d_igemm(dY, eod_pack_conv_weight_dgrad(W))        (stride 2: upsample = 2)
 *   backward-weights = eod_gemm_nt over the pixel axis on eod_transpose_gather'ed operands + eod_wgrad_reduce
 * ------------------------------------------------------------------------------------------ */
/* OIHW fp32 -> [taps-1-tap][ci - ci0][cout_pad]: packed weights of the conv dY -> dX[:, ci0:ci0+nci] */
int eod_pack_conv_weight_dgrad(const float* w_oihw, void* dst, int dtype, int Cout, int Cin, int ksize, int ci0, int nci,
                               int cout_pad, void* stream);
/* every weight re-pack of a training step in one launch: jobs (device array) of kind 0 = eod_pack_conv_weight (cpad = cin_pad) or
 * kind 1 = eod_pack_conv_weight_dgrad (cpad = cout_pad); the caller cuts each job's destination into blocks of EOD_PACK_CHUNK
 * elements: blk_job[b] = job index, blk_first[b] = first destination element of block b (device arrays, nblocks entries) */
#define EOD_PACK_CHUNK 4096
typedef struct {
    const float* w;  /* OIHW fp32 parameter */
    void* dst;       /* packed destination, storage dtype */
    int32_t kind, Cout, Cin, taps, ci0, nci, cpad, _pad;
} eod_pack_job;
int eod_pack_jobs(const eod_pack_job* jobs, const int32_t* blk_job, const int64_t* blk_first, int nblocks, int dtype, void* stream);
/* NHWC [N][H][W][C] -> [C][ld_dst], column k = (n*(Ho+2*row_pad) + ho + row_pad)*Wo + wo holds
 * src[n][ho*stride - pad + dy][wo*stride - pad + dx][c] (ups: of the nearest-2x image), zero outside / in pad rows */
int eod_transpose_gather(const void* src, int dtype, int N, int H, int W, int C, void* dst, int64_t ld_dst, int Ho, int Wo,
                         int stride, int pad, int dy, int dx, int ups, int row_pad, void* stream);
/* seg[s][c] = scale * sum of x[c][s*seg_len .. (s+1)*seg_len)   (bias / timestep-embedding gradients) */
int eod_rowsum_segments(const void* x, int dtype, int C, int64_t ld, int nseg, int64_t seg_len, float scale, float* seg,
                        int64_t seg_ld, void* stream);
int eod_colsum(const float* seg, int S, int C, float* out, void* stream); /* out[c] = sum_s seg[s][c] */
/* the same gradients from eod_gn_partial's per-(image, slab, channel) sums of the NHWC gradient (no transposed copy):
 * dbias[c] = scale * sum_{n,p} part[n][p][c][0] (c < cvalid), demb[n][c] = sum_p part[n][p][c][0]; either may be NULL */
int eod_channel_sums_finish(const float* part, int N, int P, int C, int cvalid, float scale, float* dbias, float* demb,
                            int64_t demb_ld, float* scratch /* N*cvalid floats when dbias != NULL */, void* stream);
/* dW_oihw[co][ci0+ci][tap] = scale * sum_s partial[s][tap][co][ci]  (partial: fp32 [S][taps][Cout][ldp]) */
int eod_wgrad_reduce(const float* partial, int S, int ksize, int Cout, int nci, int ldp, int ci0, int Cin, float scale,
                     float* dw_oihw, void* stream);
/* dedicated backward-weights kernel for 3x3 / stride-1 / pad-1 convs (fp16, Wo % 64 == 0, channels % 8 == 0): reads dY
 * [N][Ho][Wo][Cy] and X [N][H][W][Cx] (ups: conv input = nearest-2x of X) in place -- no transposed copies -- and writes the
 * fp32 partial tiles partial[S][9][Cout][ldp] that eod_wgrad_reduce sums (csrc/train.hip: conv3x3_wgrad_kernel) */
int eod_conv3x3_wgrad(const void* dy, const void* x, int dtype, int N, int H, int W, int Cx, int Ho, int Wo, int Cy, int Cout,
                      int ups, float* partial, int ldp, int S, void* stream);
/* ups = 2: the same for a conv whose input is the nearest-2x upsampling of X, in the parity-class form (see eod_conv_up4_ok): 16 tap
 * planes partial[S][((2p+q)*2 + a)*2 + b][Cout][ldp] from the stride-2 views of dY (4/9 of the MACs of ups = 1);
 * eod_wgrad_reduce(ksize = 4) sums the splits into [Cout][Cin][16], eod_wgrad_up4_map folds those into dW_oihw [Cout][Cin][3][3] */
int eod_wgrad_up4_map(const float* t16, int Cout, int Cin, float* dw_oihw, void* stream);
/* ups = 3: the same kernel for a STRIDE-2 3x3 conv (Downsample.op, unet_openai.py:262) of an even map: X is [N][H = 2 Ho][W = 2 Wo][Cx],
 * gathered at pixel stride 2 (two column phases per row tap); ordinary 9-plane partial tiles -> eod_wgrad_reduce(ksize 3) */
/* the same for a 1x1 / stride-1 conv (skip connections, attention projections; F.conv2d / conv1d backward-weights behind
 * unet_openai.py:345,409,413): dW[co][ci] = sum_pix dY[pix][co] X[pix][ci] over npix = N*H*W pixel-major rows, split over S
 * pixel ranges into partial[S][1][Cout][ldp] (fp16, channels % 8 == 0; csrc/train.hip: gemm_tn_kernel) */
int eod_conv1x1_wgrad(const void* dy, const void* x, int dtype, int64_t npix, int Cx, int Cy, int Cout, float* partial, int ldp,
                      int S, void* stream);
/* GroupNorm32 (+SiLU) backward (unet_openai.py:11-13,312-316): see csrc/train.hip for the algebra */
int eod_gn_mean_rstd(const float* part0, int P0, int C0, const float* part1, int P1, int C1, int N, int64_t HW, int groups,
                     float eps, float* mean_rstd, void* stream);
int eod_gn_bwd_partial(const void* x, const void* dy, const float* scale_shift, int dtype, int N, int HW, int C, float* part,
                       int P, int Ctot, int coff, int silu, void* stream);
/* film / dfilm (optional): FiLM of use_scale_shift_norm (:377-381), film[n] = [scale | shift] with row stride film_stride;
 * dfilm[n] = [d scale | d shift] */
int eod_gn_bwd_finalize(const float* part, int P, int Ctot, int N, int64_t HW, int groups, const float* mean_rstd,
                        const float* gamma, const float* beta, const float* film, int64_t film_stride, float* dfilm,
                        int64_t dfilm_stride, float* coef, float* gb, void* stream);
int eod_gn_bwd_params(const float* gb, int N, int Ctot, float scale, float* dgamma, float* dbeta, void* stream);
int eod_gn_bwd_apply(const void* x, const void* dy, const float* scale_shift, const float* coef, const void* add, int dtype,
                     int N, int HW, int C, int Ctot, int coff, int silu, void* dx, float* csum, void* stream);
/* csum (optional OUT): per-(image, slab, channel) sums of the stored dx, [N][eod_gn_bwd_apply_slabs(...)][C][2] (sum at [0]): dx is the
 * output gradient of the conv that produced x, and that conv's bias / timestep-projection gradients are these sums
 * (eod_channel_sums_finish) -- no separate eod_gn_partial pass over dY. */
int eod_gn_bwd_apply_slabs(int dtype, int N, int HW, int C);
int eod_add(const void* a, const void* b, void* y, int dtype, int64_t n, void* stream);
/* nn.Dropout of ResBlock.out_layers (unet_openai.py:339): y = x * keep / (1 - p); keep = Philox4x32-10(seed; element/4, layer, step)
 * -- forward and backward call it with the same key (x = activation / x = gradient), the mask is never stored */
int eod_dropout(const void* x, void* y, int dtype, int64_t n, float p, uint64_t seed, uint32_t layer, uint32_t step, void* stream);
/* out[(i0*n1 + i1)*n2 + i2] = sum_{j<d} a[off + j] * b[off + j], off = i0*s0 + i1*s1 + i2*s2 (elements): the attention
 * backward's D[n][head][t] = sum_j dO * O over one head's channels (rowsum(dP * P) without forming dP) */
int eod_rowdot(const void* a, const void* b, int dtype, int64_t n0, int64_t n1, int64_t n2, int64_t s0, int64_t s1, int64_t s2, int d,
               float* out, void* stream);
/* x[i] *= s (fp32, in place).  Training keeps dS = P (dP - D) of the materialised attention backward on a 2^12 scale so that it stays
 * a NORMAL fp16 number at T in the thousands (P ~ 1/T): D is scaled with this before the dS GEMM, whose alpha carries the same factor */
int eod_scale_f32(float* x, int64_t n, float s, void* stream);
/* softmax backward on rows (QKVAttention, unet_openai.py:479): dS[r][j] = P[r][j] * (dP[r][j] - sum_k dP[r][k] P[r][k]),
 * P / dS storage dtype with row stride ldp, dP fp32 with row stride lds; columns n..ldp-1 of dS are written as zeros */
/* fused attention forward on the NATURAL qkv layout [N][T][3C] (channel = q_off / k_off / v_off + head*head_stride + j; legacy
 * order: 0, d, 2d, 3d; new order: 0, C, 2C, d), head dim a multiple of 8 and <= 512, any T; out [N][T][C]; lse optional
 * [N][heads][T].  The T x T weights of unet_openai.py:476-480 / 508-514 never exist in HBM.  Head dims above 64 (the one 512-channel
 * head of the train.py:50 architecture's middle block, unet_openai.py:675-681) run on csrc/attn_wide.hip: the head dim split over the
 * waves of a workgroup, EOD_F16 and EOD_F32 (split-fp16 products) only, no pre-split tensors.
 *   EOD_F16: K / V tiles staged row-major by LDS-DMA, V^T through transposed LDS reads (csrc/attn_bwd.hip)
 *   EOD_F32: fp32 in / out, fp32 online softmax, both contractions as three fp16 MFMAs per product on operands split into
 *            hi + lo halves (fp32-grade, ~2^-22 per product; csrc/attn_x3.hip) */
enum { EOD_ATTN_OUT_PRESPLIT = 1, EOD_ATTN_IN_PRESPLIT = 2, EOD_ATTN_EXACT_F32 = 4 };
int eod_attention_fwd_nat(const void* qkv, void* out, float* lse, int dtype, int N, int T, int C, int heads, int d, int q_off, int k_off,
                          int v_off, int head_stride, const float* qkv_bound, int flags, void* stream);
/* EOD_F32 only.  qkv_bound: bound table [N][32] of the qkv tensor (eod_conv_desc.a_bound); NULL = |q|, |k|, |v| < 4094 guaranteed.
 * flags: EOD_ATTN_OUT_PRESPLIT: `out` is written pre-split for a split-fp16 conv (eod_conv_desc.x_presplit with a_bound = qkv_bound:
 *        rows of out are convex combinations of v rows, so the table of qkv bounds them);
 *        EOD_ATTN_IN_PRESPLIT: qkv arrives pre-split (eod_conv_desc.y_presplit_bound = qkv_bound): q fragments are loaded as they are,
 *        K / V tiles staged by LDS-DMA, no split arithmetic in the kernel;
 *        EOD_ATTN_EXACT_F32: IEEE fp32 products (v_mfma_f32_32x32x2_f32, csrc/attn_f32.hip) instead of the split-fp16 ones -- the
 *        fused kernel of the exact `fp32` precision mode (no bound table, no pre-split tensors). */
/* flash-style attention backward (fp16, head dim a multiple of 8 and <= 64, any T): dqkv [N][T][3C] from qkv [N][T][3C] (channel = q_off /
 * k_off / v_off + head*head_stride + j), dO [N][T][C], the forward's log-sum-exp lse [N][heads][T] (eod_attn_desc.lse) and
 * D[n][h][t] = sum_j dO*O (eod_rowdot).  P is rebuilt tile by tile in registers: nothing T x T touches HBM (csrc/attn_bwd.hip) */
int eod_attention_bwd(const void* qkv, const void* dO, const float* lse, const float* D, void* dqkv, int dtype, int N, int T, int C,
                      int heads, int d, int q_off, int k_off, int v_off, int head_stride, void* stream);
/* C[m][n] = alpha * sum_k A[k][m] * B[k][n], both operands K-major ([K][lda], [K][ldb]), fp16, batched with two stride levels
 * (batch z = b0*nb1 + b1): dV = P^T dO and dK = dS^T Q of the attention backward without transposing the T x T matrices */
int eod_gemm_tn(const void* a, int64_t lda, const void* b, int64_t ldb, void* c, int64_t ldc, int dtype, int M, int N, int K, float alpha,
                int nb0, int nb1, int64_t sa0, int64_t sa1, int64_t sb0, int64_t sb1, int64_t sc0, int64_t sc1, void* stream);
int eod_softmax_bwd_rows(const void* P, int64_t ldp, const float* dP, int64_t lds, void* dS, int dtype, int64_t rows, int n,
                         void* stream);
/* dense layers of the timestep-embedding MLP (unet_openai.py:597-602,329-335), fp32: dW, db (scaled) and / or din;
 * act_in: the layer's input is 0 = in, 1 = SiLU(in), 2 = sinusoid(t); pre != NULL multiplies din by SiLU'(pre) */
int eod_linear_bwd_small(const float* dout, int64_t ld_dout, const float* in, const int64_t* t, const float* freqs, const float* w,
                         const float* pre, int N, int K, int J, int act_in, float scale, float* dW, float* db, float* din,
                         float* scratch /* optional, 32*N*K floats: splits the J loop of din */, void* stream);
int eod_temb_pre1(const int64_t* t, const float* freqs, const float* w1, const float* b1, int N, int D, int E, float* pre1,
                  void* stream);
/* nn.Embedding backward (label_emb :604-605): dW[c][e] = scale * sum over the rows n with y[n] == c of dout[n][e] */
int eod_embedding_bwd(const float* dout, const int64_t* y, int N, int E, int classes, float scale, float* dW, void* stream);
/* nn.MSELoss(reduction='mean') (train.py:86,117): loss[0] = mean((pred-target)^2), dpred = 2*(pred-target)/n (optional);
 * scratch: scratch_len (>= 1, up to 1024 used) floats of per-block partial sums (fixed-order two-level sum) */
int eod_mse_loss(const float* pred, const float* target, int64_t n, float* loss, float* dpred, float* scratch, int scratch_len,
                 void* stream);
/* torch.optim.AdamW single-tensor step (train.py:75,119; algorithm of the pinned PyTorch 1.13, eo_diffusion.yml:114) on flat
 * fp32 buffers; `step` is the 1-based update count */
int eod_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2, double eps,
                   double weight_decay, int step, void* stream);
/* the same step behind an overflow guard (fp16 training with a static loss scale): if any gradient is inf / NaN the step is SKIPPED
 * (p, m, v untouched).  state (device, 4 ints, zero-initialised by the caller once) = {this step was skipped, steps skipped so far,
 * two floats of the kernel's own}; scratch: scratch_len (>= 1, up to 8192 used) ints.  `step` = the 1-based number of CALLS; the bias
 * corrections use step - (steps skipped so far), i.e. the number of moment updates, computed on the device: a skipped step never
 * reaches the optimizer, as with torch.cuda.amp.GradScaler.  No host synchronisation. */
int eod_adamw_step_guarded(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2, double eps,
                           double weight_decay, int step, int* state, int* scratch, int scratch_len, void* stream);
/* The training objective of the reference's vendored trainers (denoising_diffusion_pytorch.py:662-706: loss_type, per-sample reduction,
 * per-timestep weight, batch mean) with a pixel mask.  pred, target: [N][C][H][W] fp32; mask (optional): [mask_n][mask_c][H][W] fp32 with
 * mask_n = N or 1, mask_c = C or 1, values finite and >= 0 (a one-channel mask counts once per channel); weight (optional): [N] fp32.
 * kind 0 = l2 (l = d^2), 1 = l1 (|d|, l' = sign(d), sign(+-0) = 0), 2 = huber (torch's huber_loss, delta > 0), d = pred - target:
 *   S_n = sum_e m_e,  L_n = sum_e m_e l(d_e) / S_n (0 where S_n = 0),  loss[0] = (1/N) sum_n w_n L_n,  per_sample[n] = L_n,
 *   dpred (optional) = (s_n * m_e) * l'(d_e) in fp32, s_n = (float)(w_n / (N * S_n)) formed in double (0 where S_n = 0).
 * An element whose m_e is exactly 0 is skipped: it adds 0 and its dpred is +0.0 even where pred / target are NaN or inf.  Sums are float64
 * in the discipline of csrc/met_sum.h (no floating-point atomics; a sample's L_n and dpred bits depend on that sample alone).  With a mask:
 * one pass over the mask, then one fused loss + gradient pass; without: the fused pass alone.  No host synchronisation; capturable.
 * ws: eod_diffusion_loss_workspace_size(N, C, H, W) bytes (-1: bad arguments), 8-byte aligned. */
int64_t eod_diffusion_loss_workspace_size(int N, int C, int H, int W);
int eod_diffusion_loss(const float* pred, const float* target, const float* mask, int mask_n, int mask_c, const float* weight, int N, int C,
                       int H, int W, int kind, float delta, float* loss, float* per_sample, float* dpred, void* ws, int64_t ws_bytes,
                       void* stream);
/* sumsq[0] = the float64 sum of g[i]^2 (inf or NaN iff a g[i] is): the guarded step's scan, forming the squared norm.  Up to
 * min(slots, 8192) workgroups, one float64 slot each, added in the order of csrc/met_sum.h; ws: eod_grad_sumsq_workspace_size(slots) bytes,
 * 8-byte aligned like sumsq. */
int64_t eod_grad_sumsq_workspace_size(int slots);
int eod_grad_sumsq(const float* g, int64_t n, double* sumsq, void* ws, int64_t ws_bytes, int slots, void* stream);
/* eod_adamw_step_guarded with gradient clipping to a GLOBAL norm (denoising_diffusion_pytorch.py:877, torch's clip_grad_norm_ rule):
 * sumsq[0 .. n_groups) are the eod_grad_sumsq results of ALL parameter groups (every group's call passes the same array); they are added in
 * group order, total_norm = sqrt(sum), coef = (float) min(1, max_norm / (total_norm + 1e-6)), and the update is the guarded step's with
 * g[i] * coef in place of g[i].  g is NOT written (torch's clip scales p.grad in place).  A sum that is not finite skips the step as the
 * guarded step does (`step` = the number of calls, bias corrections from the applied steps).  state (device, 10 ints, 8-byte aligned,
 * zeroed once): {skipped now, skipped so far, clipped now, clipped so far, bits(sqrt(1 - beta2^a)), bits(-lr / (1 - beta1^a)),
 * bits(coef) (1.0 on a skipped step), 0, total_norm as a double}.  max_norm > 0, inf allowed.  No host synchronisation. */
int eod_adamw_step_clipped(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2, double eps,
                           double weight_decay, int step, double max_norm, const double* sumsq, int n_groups, int* state, void* stream);
/* EMA of script_utils/utils.py:56-67: avg = decay*avg + (1-decay)*p */
int eod_ema_update(float* avg, const float* p, int64_t n, double decay, void* stream);

#ifdef __cplusplus
}
#endif
#endif
