/* nisqa_train.h -- C ABI of the training-step kernels in libnisqa_hip.so (BASELINE config 5).
 *
 * One optimiser step of the CNN-SA-AP model -- what the reference does at nisqa/NISQA_model.py:131-152 / 330-352
 * (model.train(); model(x, n_wins); biasLoss.get_loss; backward; Adam.step) -- is driven from the host
 * (nisqa_amd/train.py) as a sequence of these operators.  Train-mode BatchNorm needs statistics over every valid
 * segment of the batch between a convolution and its activation, so the per-segment fusion of the inference
 * kernels does not apply; convolutions run as implicit GEMMs on fp32 MFMA, activations live in HBM.
 *
 * Conventions: float32 row-major everywhere; activations are pixel-major, channels contiguous: act[S][H*W][C];
 * token matrices are [tokens][features].  All pointers are device memory owned by the caller, all work is enqueued
 * on `stream`; return 0 or NISQA_ERR_* (nisqa_hip.h).
 */
#ifndef NISQA_TRAIN_H
#define NISQA_TRAIN_H

#include <stdint.h>
#include "nisqa_hip.h"        /* nisqa_mel_cfg, NISQA_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

/* Grouped GEMM on v_mfma_f32_32x32x2_f32: for every group g, C_g (+)= alpha * op(A_g) op(B_g).
 * desc[g][10] (int64): a_off, b_off, c_off (element offsets into A, B, C), M, N, K, lda, ldb, ldc, tile_start
 * (exclusive prefix sum of ceil(M/64)*ceil(N/64) over the groups; total_tiles = the sum).
 * trans_a: A_g is stored [K][M] (lda = row stride of the stored matrix); trans_b: B_g is stored [N][K] (a Linear /
 * conv weight).  ksplit > 1 splits K over blockIdx.y and accumulates with atomicAdd into a C the caller zeroed
 * (weight gradients: K = number of rows of the batch).  Replaces every F.linear / F.conv2d / torch.bmm and their
 * autograd counterparts of the training step. */
int nisqa_gemm_f32(const float* a, const float* b, float* c, const int64_t* desc, int32_t n_groups,
                   int32_t total_tiles, int32_t trans_a, int32_t trans_b, int32_t ksplit, float alpha, void* stream);
/* the single-group case without a descriptor in device memory: C[m][n] (+)= alpha * op(A) op(B), with an optional
 * epilogue (ksplit == 1 only): + bias[n] (may be NULL), then ReLU if relu != 0 */
int nisqa_gemm_f32_one(const float* a, const float* b, float* c, int64_t m, int64_t n, int64_t k, int64_t lda,
                       int64_t ldb, int64_t ldc, int32_t trans_a, int32_t trans_b, int32_t ksplit, float alpha,
                       const float* bias, int32_t relu, void* stream);
/* the tile nisqa_gemm_f32_one runs an m x n product on (host only, launches nothing; the launcher calls it, so a test
 * reads the kernel a shape selects instead of restating the rule): returns the configuration index and writes the
 * tile's rows / columns to *bm / *bn (either may be NULL): 0 = 64 x 64, 1 = 128 x 32, 2 = 128 x 128, 3 = 256 x 64,
 * 4 = 64 x 256.  The big tiles 2 and 3 only from 192 workgroups up. */
int nisqa_gemm_f32_one_tile(int64_t m, int64_t n, int32_t* bm, int32_t* bn);

/* conv1 patches straight from the dB spectrogram (Framewise + segment_specs, NISQA_lib.py:2239-2282, 487-502):
 * col[s*720 + m*15 + j][dy*3+dx] = max(mel_tm[frame_off[b] + k*seg_hop + j+dx-1][m+dy-1], clip_floor[b]) or 0
 * outside the 48x15 segment; s = seg_off[b] + k runs over the VALID segments of the batch only. */
int nisqa_im2col_mel(const float* mel_tm, const int32_t* frame_off, const int32_t* seg_off, const float* clip_floor,
                     int32_t n_clips, int32_t n_segments, int32_t seg_hop, float* col, void* stream);
/* conv1 (1 -> 16 channels) without a patch matrix: z[s*720 + m*15 + j][co] = bias[co] + sum_tap w[co][tap] * patch, and
 * its weight gradient dw[co][tap] += sum dz * patch (dw zeroed by the caller); w is [16][9] with tap = dy*3 + dx */
int nisqa_conv1_fwd(const float* mel_tm, const int32_t* frame_off, const int32_t* seg_off, const float* clip_floor,
                    int32_t n_clips, int32_t n_segments, int32_t seg_hop, const float* w, const float* bias, float* z,
                    void* stream);
int nisqa_conv1_wgrad(const float* mel_tm, const int32_t* frame_off, const int32_t* seg_off, const float* clip_floor,
                      int32_t n_clips, int32_t n_segments, int32_t seg_hop, const float* dz, float* dw, void* stream);
/* Layer 1 of the training step without its 720-pixel activations (conv1 -> train-mode BatchNorm -> ReLU -> 24 x 7 adaptive
 * max-pool -> per-channel dropout scale; NISQA_lib.py:688-697 in train mode).  z1 is affine in the nine patch values, so
 * the batch statistics, the reductions of the BatchNorm backward and the dense part of the weight gradient follow from the
 * first and second patch moments; pooled values and their gradients are recomputed from the spectrogram.
 *   nisqa_conv1_moments: mom54 [dev, zeroed by the caller] += P1[t] = sum patch[t] (9), then the upper triangle of
 *                        P2[t][u] = sum patch[t] patch[u] (45), over all pixels of all valid segments;
 *   ..._fwd: sums32 [dev] (sum z, sum z^2 per channel, as nisqa_col_dot(z, z) would give), running statistics and
 *            mean_rstd [dev, 32] updated like nisqa_bn_act_pool_fwd, y [S][168][16] pooled activations (x drop[s][c] if
 *            drop != NULL), arg = pixel (band * 15 + frame) of each maximum;
 *   ..._bwd: dy [S][168][16] -> dgamma, dbeta [16], dw [16][9] (overwritten; the conv bias gradient is exactly zero);
 *            acc176 [dev, zeroed by the caller] is scratch for the float64 reductions. */
int nisqa_conv1_moments(const float* mel_tm, const int32_t* frame_off, const int32_t* seg_off, const float* clip_floor,
                        int32_t n_clips, int32_t n_segments, int32_t seg_hop, double* mom54, void* stream);
int nisqa_conv1_bn_act_pool_fwd(const float* mel_tm, const int32_t* frame_off, const int32_t* seg_off, const float* clip_floor,
                                int32_t n_clips, int32_t n_segments, int32_t seg_hop, const float* w, const float* bias,
                                const double* mom54, const float* gamma, const float* beta, float* running_mean,
                                float* running_var, double* sums32, float* mean_rstd, const float* drop, float* y,
                                int32_t* arg, void* stream);
int nisqa_conv1_bn_act_pool_bwd(const float* mel_tm, const int32_t* frame_off, const int32_t* seg_off, const float* clip_floor,
                                int32_t n_clips, int32_t n_segments, int32_t seg_hop, const float* w, const float* bias,
                                const double* mom54, const float* gamma, const float* beta, const float* mean_rstd,
                                const float* drop, const float* dy, const int32_t* arg, double* acc176, float* dgamma,
                                float* dbeta, float* dw, void* stream);
/* The same for StandardCNN's layer 1 (conv1 -> train-mode BatchNorm -> ReLU -> pool_first = MaxPool2d(2, stride 2, padding (0, 1)),
 * 48 x 15 -> 24 x 8 -> per-channel dropout scale; NISQA_lib.py:712-836): arguments and moments as above, y / dy / arg are
 * [S][192][16]; pooled pixel (oy, ox) reads bands 2 oy, 2 oy + 1 and frames 2 ox - 1, 2 ox (the padding column never wins),
 * ties go to the first maximum in (band, frame) order as in PyTorch. */
int nisqa_conv1_bn_act_pool_std_fwd(const float* mel_tm, const int32_t* frame_off, const int32_t* seg_off, const float* clip_floor,
                                    int32_t n_clips, int32_t n_segments, int32_t seg_hop, const float* w, const float* bias,
                                    const double* mom54, const float* gamma, const float* beta, float* running_mean,
                                    float* running_var, double* sums32, float* mean_rstd, const float* drop, float* y,
                                    int32_t* arg, void* stream);
int nisqa_conv1_bn_act_pool_std_bwd(const float* mel_tm, const int32_t* frame_off, const int32_t* seg_off, const float* clip_floor,
                                    int32_t n_clips, int32_t n_segments, int32_t seg_hop, const float* w, const float* bias,
                                    const double* mom54, const float* gamma, const float* beta, const float* mean_rstd,
                                    const float* drop, const float* dy, const int32_t* arg, double* acc176, float* dgamma,
                                    float* dbeta, float* dw, void* stream);
/* 3x3 patches, padding (1, pad_w): x[S][H*W][C] -> col[S*H*Wo][9*C], Wo = W + 2*pad_w - 2, k = (dy*3+dx)*C + c
 * (C % 4 == 0, 16-byte aligned buffers) */
int nisqa_im2col3x3(const float* x, int32_t n_segments, int32_t h, int32_t w, int32_t c, int32_t pad_w, float* col,
                    void* stream);
/* The same three convolution products without a patch matrix (implicit GEMM: the loaders gather the patches).
 *   mode 0  z[S*H*Wo][co]  = conv(x[S][H*W][ci], w[co][9*ci]) (+ bias, may be NULL)      in: x,  w   out: z
 *   mode 1  dx[S*H*W][ci]  = conv^T(dz[S][H*Wo][co], w)                                  in: dz, w   out: dx
 *   mode 2  dw[co][9*ci]  += dz^T * patches(x)   (dw zeroed by the caller, ksplit chunks) in: x,  dz  out: dw
 * ci, co powers of two >= 4; padding (1, pad_w) as in nisqa_im2col3x3. */
int nisqa_conv3x3_gemm(int32_t mode, const float* x_or_dz, const float* w_or_dz, float* out, int32_t n_segments, int32_t h,
                       int32_t w, int32_t ci, int32_t co, int32_t pad_w, const float* bias, int32_t ksplit, void* stream);
/* The same on split-bf16 MFMA (operands as bf16 hi + lo, three products per term, fp32 accumulation: 16 operand bits, the
 * arithmetic of the inference path's default precision; 5.3x the fp32-MFMA rate).  Same arguments. */
int nisqa_conv3x3_gemm_bf16(int32_t mode, const float* x_or_dz, const float* w_or_dz, float* out, int32_t n_segments, int32_t h,
                            int32_t w, int32_t ci, int32_t co, int32_t pad_w, const float* bias, int32_t ksplit, void* stream);
/* Mode 0 with the BatchNorm batch statistics riding along: stats2c [dev, float64, zeroed by the caller] += sum z, sum z^2
 * per output channel over all rows (what nisqa_col_dot(z, z) would add in a second pass over z); split_bf16 selects the
 * arithmetic of nisqa_conv3x3_gemm_bf16. */
int nisqa_conv3x3_fwd_stats(int32_t split_bf16, const float* x, const float* w_, float* z, int32_t n_segments, int32_t h,
                            int32_t w, int32_t ci, int32_t co, int32_t pad_w, const float* bias, double* stats2c, void* stream);
/* Forward and input-gradient convolutions of the AdaptCNN layers 2..6, SEGMENT-RESIDENT (csrc/train_conv.hip): a workgroup
 * stages the activations of a few whole segments in LDS once (split into bf16 hi + lo once) and runs the K loop of the
 * inference kernel over them; arithmetic = nisqa_conv3x3_gemm_bf16 (three products per term, fp32 accumulation).
 * Replaces, for the five layer shapes of config/train_nisqa_cnn_sa_ap.yaml, what PyTorch does inside
 * nisqa/NISQA_lib.py:690-705 (conv forward) and in autograd's convolution backward (NISQA_model.py:142-143).
 *   nisqa_segconv_supported  1 if (h, w, ci, co, pad_w) is one of those shapes; otherwise callers use nisqa_conv3x3_gemm_bf16.
 *                            The shapes, each with the pooled size (ho, wo) that the folded weight gradients below take:
 *                              (24,7,16,32,1) -> (12,5)   (12,5,32,64,1) -> (12,5)   (12,5,64,64,1) -> (6,3)
 *                              (6,3,64,64,1) -> (6,3)     (6,3,64,64,0) -> (6,1)
 *                            Every nisqa_segconv_* entry below takes exactly these and returns NISQA_ERR_ARG for anything else.
 *   nisqa_segconv_frag_bytes size of the packed weight fragments of one layer and mode (-1: bad arguments)
 *   nisqa_segconv_pack       w[co][9*ci] -> fragments (bf16 hi / lo, MFMA B-operand order); mode 0 forward, mode 1 input
 *                            gradient (taps mirrored, matrix transposed).  Once per optimiser step.
 *   nisqa_segconv_bf16       mode 0: z[S*h*wo][co] = conv(x[S][h*w][ci]) + bias (may be NULL); stats2c (may be NULL; float64,
 *                            zeroed by the caller) += sum z, sum z^2 per channel;
 *                            mode 1: dx[S*h*w][ci] = conv^T(dz[S][h*wo][co]); bias and stats2c must be NULL.
 *                            frags = nisqa_segconv_pack of the same mode.
 * The other operand formats (_f32, _bf16x6, _f16 below) each have their own nisqa_segconv_frag_bytes* / nisqa_segconv_pack*_many /
 * convolution entry with the arguments of nisqa_segconv_frag_bytes / nisqa_segconv_pack_many / nisqa_segconv_bf16; fragments of
 * one format are read by that format's convolution only. */
int nisqa_segconv_supported(int32_t h, int32_t w, int32_t ci, int32_t co, int32_t pad_w);
int64_t nisqa_segconv_frag_bytes(int32_t mode, int32_t ci, int32_t co);
int nisqa_segconv_pack(int32_t mode, const float* w, int32_t ci, int32_t co, uint16_t* frags, void* stream);
/* nisqa_segconv_pack for n_jobs <= 10 (layer, mode) pairs in one launch; all arrays are HOST arrays of n_jobs entries
 * (w[j], frags[j] device pointers) */
int nisqa_segconv_pack_many(int32_t n_jobs, const int32_t* modes, const float* const* w, const int32_t* ci, const int32_t* co,
                            uint16_t* const* frags, void* stream);
int nisqa_segconv_bf16(int32_t mode, const float* src, const uint16_t* frags, float* out, int32_t n_segments, int32_t h,
                       int32_t w, int32_t ci, int32_t co, int32_t pad_w, const float* bias, double* stats2c, void* stream);
/* The same two products in EXACT fp32 (v_mfma_f32_32x32x2_f32; fp32 planes in LDS, fp32 fragments): the forward convolutions of
 * the precision modes 'f32' and 'mixed' and the input gradients of 'f32'.  The implicit GEMMs (nisqa_conv3x3_gemm) reach the
 * fp32-MFMA peak on none of these shapes but the 64 -> 64 one at 12 x 5 (narrow outputs, gathers per K-tile); here every
 * activation is fetched once.  Fragments are floats. */
int64_t nisqa_segconv_frag_bytes_f32(int32_t mode, int32_t ci, int32_t co);
int nisqa_segconv_pack_f32_many(int32_t n_jobs, const int32_t* modes, const float* const* w, const int32_t* ci, const int32_t* co,
                                float* const* frags, void* stream);
int nisqa_segconv_f32(int32_t mode, const float* src, const float* frags, float* out, int32_t n_segments, int32_t h, int32_t w,
                      int32_t ci, int32_t co, int32_t pad_w, const float* bias, double* stats2c, void* stream);
/* The same two products at fp32 OPERAND precision on the bf16 matrix pipe (precision mode 'bf16x6'): activations and weights
 * as three exact bf16 terms (hi + mid + lo), six MFMA products per term pair, fp32 accumulation -- the accuracy of
 * nisqa_segconv_f32 at 2.7 x its matrix-pipe rate.  Three-term fragments: 1.5 x the bytes. */
int64_t nisqa_segconv_frag_bytes_x6(int32_t mode, int32_t ci, int32_t co);
/* The same two products on TWO f16 terms per operand, all four term products (precision mode 'f16x4'): the staged tensor of a
 * workgroup's group of segments as f16 hi + lo of x * 2^e, e from the group's own largest magnitude (measured while the values are
 * in registers); the weights as f16 hi + lo of W * 2^kw, kw from the layer's largest |W| of this optimiser step (computed on the
 * device by the packer, stored behind the fragments: the buffer is 16 bytes longer).  11 + 11 significand bits and the low term's
 * sign: the fp32 value itself for ~75 % of the operands, one fp32 ulp off otherwise; held to the bounds of nisqa_segconv_f32 by the
 * same test. */
int64_t nisqa_segconv_frag_bytes_f16(int32_t mode, int32_t ci, int32_t co);
int nisqa_segconv_pack_f16_many(int32_t n_jobs, const int32_t* modes, const float* const* w, const int32_t* ci, const int32_t* co,
                                uint16_t* const* frags, void* stream);
int nisqa_segconv_f16(int32_t mode, const float* src, const uint16_t* frags, float* out, int32_t n_segments, int32_t h, int32_t w,
                      int32_t ci, int32_t co, int32_t pad_w, const float* bias, double* stats2c, void* stream);
int nisqa_segconv_pack_x6_many(int32_t n_jobs, const int32_t* modes, const float* const* w, const int32_t* ci, const int32_t* co,
                               uint16_t* const* frags, void* stream);
int nisqa_segconv_bf16x6(int32_t mode, const float* src, const uint16_t* frags, float* out, int32_t n_segments, int32_t h, int32_t w,
                         int32_t ci, int32_t co, int32_t pad_w, const float* bias, double* stats2c, void* stream);
/* Weight gradient of the same layers, segment-resident: dw[co][9*ci] += dz^T * patches(x) (dw zeroed by the caller, like
 * nisqa_conv3x3_gemm mode 2); x[S][h*w][ci], dz[S][h*wo][co].  A workgroup keeps its part of dw in registers over all the
 * segments it walks over and adds it to dw once (fp32 atomics). */
int nisqa_segconv_wgrad_bf16(const float* x, const float* dz, float* dw, int32_t n_segments, int32_t h, int32_t w, int32_t ci,
                             int32_t co, int32_t pad_w, void* stream);
/* adjoint of nisqa_im2col3x3 (gather form, no atomics): dx[S][H*W][C] = sum of the patch entries that read it */
int nisqa_col2im3x3(const float* dcol, int32_t n_segments, int32_t h, int32_t w, int32_t c, int32_t pad_w, float* dx,
                    void* stream);

/* out[0..C) += sum_rows a[r][c], out[C..2C) += sum_rows a[r][c]*b[r][c] in float64 (caller zeroes out).
 * BatchNorm statistics (b = a), BatchNorm / LayerNorm / bias gradients. */
int nisqa_col_dot(const float* a, const float* b, int64_t rows, int32_t c, double* out, void* stream);

/* BatchNorm2d (batch statistics) + ReLU + adaptive_max_pool2d + Dropout2d (NISQA_lib.py:690-705, train mode).
 * sums = nisqa_col_dot(z, z) over rows = S*H*W.  Writes mean_rstd[2C], updates running_mean / running_var
 * (momentum 0.1, unbiased variance), y[S][Ho*Wo][C] and the arg-max pixel of every output (int32, for backward; NOT written
 * when Ho == H and Wo == W -- the identity "pooling" of layers 3, 5, 6, whose backward never reads it).
 * drop (may be NULL): [S][C] multipliers (0 or 1/(1-p)). */
int nisqa_bn_act_pool_fwd(const float* z, const double* sums, const float* gamma, const float* beta,
                          float* running_mean, float* running_var, float* mean_rstd, int32_t n_segments, int32_t h,
                          int32_t w, int32_t c, int32_t ho, int32_t wo, const float* drop, float* y, int32_t* arg,
                          void* stream);
/* backward of the above in two passes around a nisqa_col_dot(dyb, z):
 * pass 1: dyb[S][H*W][C] = d loss / d (BatchNorm output) from dy[S][Ho*Wo][C] (pool scatter, dropout, ReLU gate);
 * pass 2: in place dyb -> dz = gamma*rstd*(dyb - mean(dyb) - xhat*mean(dyb*xhat)); dgamma, dbeta from sums2.
 * c must be a multiple of 4 (1024 % c == 0 for nisqa_bn_bwd2).  When 1024 % c == 0 the reductions ride along: pass 1 adds sum(dyb), sum(dyb*z) to sums2_opt[2c] (zeroed by the caller;
 * NULL: run nisqa_col_dot yourself), pass 2 adds the column sums of dz (the conv bias gradient) to sum_dz_opt[2c]. */
int nisqa_bn_act_pool_bwd1(const float* dy, const int32_t* arg, const float* drop, const float* z,
                           const float* mean_rstd, const float* gamma, const float* beta, int32_t n_segments,
                           int32_t h, int32_t w, int32_t c, int32_t ho, int32_t wo, float* dyb, double* sums2_opt,
                           void* stream);
/* The two passes above in a form that reads z and writes dz ONCE: the reductions only see pixels that won a pooling
 * window, so they are taken over the pooled values first (sums2 [2c] float64, zeroed by the caller; 1024 % c == 0). */
int nisqa_bn_act_pool_bwd(const float* dy, const int32_t* arg, const float* drop, const float* z, const float* mean_rstd,
                          const float* gamma, const float* beta, int32_t n_segments, int32_t h, int32_t w, int32_t c, int32_t ho,
                          int32_t wo, double* sums2, float* dz, float* dgamma, float* dbeta, void* stream);
/* The first launch of nisqa_bn_act_pool_bwd on its own (sums2 += sum dyb, sum dyb * z over the pooled values), and the weight
 * gradient of the segment-resident convolutions with the REST of that backward folded into its staging: it is handed z and the
 * pooled gradient dy (+ arg, drop) instead of dz, computes dz = gamma rstd (dyb - mean(dyb) - xhat mean(dyb xhat)) per element
 * while it stages a group of segments, writes dz (for the input-gradient kernel that runs next), dgamma and dbeta, and adds dw
 * like nisqa_segconv_wgrad_bf16.  The dense z -> dz pass of layers 2..6 (memory-bound, 0.29 ms of a 3.4 ms step) disappears.
 * Shapes: the nisqa_segconv_supported layers, each with its own pooled size (ho, wo) listed there; anything else returns
 * NISQA_ERR_ARG (run nisqa_bn_act_pool_bwd + nisqa_segconv_wgrad_bf16 instead). */
int nisqa_bn_pool_bwd_sums(const float* dy, const int32_t* arg, const float* drop, const float* z, const float* mean_rstd,
                           const float* gamma, const float* beta, int32_t n_segments, int32_t h, int32_t w, int32_t c, int32_t ho,
                           int32_t wo, double* sums2, void* stream);
int nisqa_segconv_wgrad_bn_bf16(const float* x, const float* z, const float* dy, const int32_t* arg, const float* drop,
                                const float* mean_rstd, const float* gamma, const float* beta, const double* sums2, float* dz_out,
                                float* dgamma, float* dbeta, float* dw, int32_t n_segments, int32_t h, int32_t w, int32_t ci,
                                int32_t co, int32_t pad_w, int32_t ho, int32_t wo, void* stream);
/* The weight gradient of the same five layers, segment-resident, in EXACT fp32 (v_mfma_f32_32x32x2_f32: precision mode 'f32',
 * the reference's arithmetic), with or without the BatchNorm backward folded in: z == NULL -> dz_out holds dz on entry (as
 * nisqa_segconv_wgrad_bf16's dz; dy .. sums2, dgamma, dbeta unused); z != NULL -> the contract of nisqa_segconv_wgrad_bn_bf16. */
int nisqa_segconv_wgrad_f32(const float* x, const float* z, const float* dy, const int32_t* arg, const float* drop,
                            const float* mean_rstd, const float* gamma, const float* beta, const double* sums2, float* dz_out,
                            float* dgamma, float* dbeta, float* dw, int32_t n_segments, int32_t h, int32_t w, int32_t ci, int32_t co,
                            int32_t pad_w, int32_t ho, int32_t wo, void* stream);
/* ... and at fp32 OPERAND precision on the bf16 matrix pipe (x and dz as three exact bf16 terms, six products: precision mode
 * 'bf16x6'); the contract of nisqa_segconv_wgrad_f32. */
int nisqa_segconv_wgrad_bf16x6(const float* x, const float* z, const float* dy, const int32_t* arg, const float* drop,
                               const float* mean_rstd, const float* gamma, const float* beta, const double* sums2, float* dz_out,
                               float* dgamma, float* dbeta, float* dw, int32_t n_segments, int32_t h, int32_t w, int32_t ci,
                               int32_t co, int32_t pad_w, int32_t ho, int32_t wo, void* stream);
int nisqa_bn_bwd2(float* dyb_to_dz, const float* z, const double* sums2, const float* mean_rstd, const float* gamma,
                  int64_t rows, int32_t c, float* dgamma, float* dbeta, double* sum_dz_opt, void* stream);

/* LayerNorm over rows of 64 (NISQA_lib.py:991, 1033, 1037): y = gamma*xhat + beta; saves xhat and rstd */
int nisqa_layernorm_fwd(const float* x, const float* gamma, const float* beta, int64_t rows, float* y, float* xhat,
                        float* rstd, void* stream);
/* dx = rstd*(g - mean(g) - xhat*mean(g*xhat)), g = dy*gamma (parameter gradients: nisqa_col_dot(dy, xhat)) */
int nisqa_layernorm_bwd(const float* dy, const float* xhat, const float* rstd, const float* gamma, int64_t rows,
                        float* dx, void* stream);

/* Row softmax over ragged rows: row r has len[r] entries at x + off[r]; p = softmax(scale * x) (in place allowed).
 * Attention probabilities (one row per query token) and attention pooling (one row per clip and head). */
int nisqa_softmax_rows_fwd(const float* x, const int64_t* off, const int32_t* len, int64_t rows, float scale,
                           float* p, void* stream);
/* ds = scale * p * (dp - sum_j dp_j p_j)  (in place on dp allowed) */
int nisqa_softmax_rows_bwd(const float* p, const float* dp, const int64_t* off, const int32_t* len, int64_t rows,
                           float scale, float* ds, void* stream);

/* Elementwise helpers on [rows][cols] matrices (cols = row length, bias / vectors of length cols):
 *   op 0: y = x + bias                      op 1: y = relu(x + bias)
 *   op 2: y = x * (aux > 0)   (ReLU gate)   op 3: y = x * aux        (dropout mask)
 *   op 4: y = x + aux          (residual)   op 5: y = x * bias[col]  (per-column scale) */
int nisqa_elementwise(int32_t op, const float* x, const float* aux, const float* bias, int64_t rows, int32_t cols,
                      float* y, void* stream);

/* biasLoss.get_loss (NISQA_lib.py:1880-1892, 1946-1950): loss = sum_h mean_{b: y not NaN} (map_bh(y_hat[b][h]) - y[b][h])^2,
 * map_bh(v) = q0 + q1 v + q2 v^2 + q3 v^3 (NULL: identity), d y_hat[b][h] = 2 e / count_h * (q1 + 2 q2 v + 3 q3 v^2).  Writes
 * loss[1 + heads] (total, then one term per head) and dy_hat[B][heads].
 *   nisqa_mse_loss        q = bias[b][4]: one mapping per clip, shared by the heads (the one-headed models);
 *   nisqa_mse_loss_heads  q = bias[b][h][4]: one mapping per clip AND head (NISQA_DIM keeps five biasLoss objects,
 *                         NISQA_model.py:256-371).  With n_heads == 1 the two are the same. */
int nisqa_mse_loss(const float* y_hat, const float* y, const float* bias, int32_t n_clips, int32_t n_heads,
                   float* loss, float* dy_hat, void* stream);
int nisqa_mse_loss_heads(const float* y_hat, const float* y, const float* bias, int32_t n_clips, int32_t n_heads,
                         float* loss, float* dy_hat, void* stream);

/* Dropout multipliers (nn.Dropout / Dropout2d in train mode): out[i] = u_i >= p ? 1/(1-p) : 0 with u_i the i-th value of the
 * Philox-4x32-10 stream (seed, offset counts groups of four values); the reference draws its masks from torch's global
 * generator inside the modules, so only the distribution, not the bits, can agree. */
int nisqa_dropout_mask(uint64_t seed, uint64_t offset, float p, int64_t n, float* out, void* stream);

/* dst[table[e][1] + t] = (float)src[table[e][0] + t], t < table[e][2], for e < n_entries (table: int32 [n_entries][3]):
 * the float64 column sums of a step that ARE gradients (biases, LayerNorm parameters) move to the flat gradient buffer */
int nisqa_cast_scatter(const double* src, const int32_t* table, int32_t n_entries, float* dst, void* stream);

/* BiLSTM of the StandardCNN + BiLSTM models in training (csrc/train_lstm.hip; nn.LSTM(20, 128, bidirectional) over each clip's
 * valid segments, NISQA_lib.py:897-943, then the reduction of PoolLastStepBi / PoolAvg / PoolMax, NL:1099-1115, 1185-1224).
 * One workgroup per (clip, direction), one launch each; clip b owns tokens seg_off[b] .. seg_off[b+1]-1 (seg_off [n_clips+1]).
 * Weights in PyTorch's gate order (i, f, g, o), both directions back to back: w_ih [2][512][20], w_hh [2][512][128],
 * b_ih, b_hh [2][512].  pool_mode: NISQA_LSTM_POOL_* (nisqa_hip.h).
 *   nisqa_lstm_train_fwd  x20 [tokens][20] -> save [tokens][2][640] (activated gates i, f, g, o and the cell state c of each
 *                         step), hprev [tokens][2][128] (the hidden state each step read; 0 at a direction's first step),
 *                         pooled [n_clips][256] (direction-major: the last step / the float64 mean / the maximum), argmax
 *                         [n_clips][256] (pool_mode MAX only, else may be NULL: the step -- in the direction's own order -- of
 *                         each maximum);
 *   nisqa_lstm_train_bptt dpooled [n_clips][256] = d loss / d pooled -> dgates [tokens][2][512] = d loss / d (gate
 *                         pre-activations); dbias (may be NULL; float64 [2][512], zeroed by the caller) += the sum of dgates
 *                         over the tokens (the gradient of b_ih and of b_hh alike).  Parameter and input gradients then
 *                         follow from nisqa_gemm_f32_one: dW_ih = dgates^T x20, dW_hh = dgates^T hprev, dx20 = dgates w_ih. */
int nisqa_lstm_train_fwd(const float* x20, const int32_t* seg_off, int32_t n_clips, const float* w_ih, const float* w_hh,
                         const float* b_ih, const float* b_hh, int32_t pool_mode, float* save, float* hprev, float* pooled,
                         int32_t* argmax, void* stream);
int nisqa_lstm_train_bptt(const int32_t* seg_off, int32_t n_clips, const float* w_hh, const float* save, int32_t pool_mode,
                          const float* dpooled, const int32_t* argmax, float* dgates, double* dbias, void* stream);

/* torch.optim.Adam (betas 0.9 / 0.999, eps 1e-8, no weight decay), step counter t >= 1, on flat buffers */
int nisqa_adam_step(float* param, const float* grad, float* m, float* v, int64_t n, float lr, int32_t t, void* stream);

/* ---- The self-attention block + attention-pooling heads + loss of the training step as ONE call (csrc/train_td.hip) ----
 * Replaces, for the CNN-SA-AP model in train mode, SelfAttention.forward / SelfAttentionLayer.forward (NISQA_lib.py:988-996,
 * 1025-1040), PoolAttFF.forward (NISQA_lib.py:1171-1183), biasLoss.get_loss (NISQA_lib.py:1880-1892, 1946-1950) and autograd's
 * backward of all of them (NISQA_model.py:142-143): a dozen launches (token-tile kernels that chain their products through
 * registers, flash-style attention forward and backward with the dropout masks inside, one grouped split-K GEMM for every
 * weight gradient, one column-sum launch for every bias / LayerNorm gradient) instead of ~116 operator launches.  fp32 MFMA.
 *
 * Parameter offsets `poff` (HOST array, int32, offsets in floats into `params` and `grads`), in this order:
 *   [0] linear.weight as [64][384] with columns in the feature tensor's (y, c) order  [1] linear.bias  [2] norm1.weight  [3] norm1.bias
 *   per layer l at 4 + 12 l: in_proj_weight [192][64], in_proj_bias, out_proj.weight, out_proj.bias, norm1.weight, norm1.bias,
 *                            linear1.weight, linear1.bias, linear2.weight, linear2.bias, norm2.weight, norm2.bias
 *   per head h at 4 + 12 L + 6 h: linear1.weight [128][64], linear1.bias, linear2.weight [128], linear2.bias, linear3.weight [64],
 *                            linear3.bias
 * Token spaces: the caller's tokens (segments) are packed clip after clip (seg_off); inside the block every clip is padded to
 * whole 32-token tiles (ptok_off, multiples of 32; tile_clip[t] = clip of tile t).
 *
 * nisqa_tdtrain_plan (host only, no GPU work): out[0] = workspace floats, out[1] = fragment-buffer floats, out[2] = groups and
 *   out[3] = 64 x 64 tiles of the weight-gradient GEMM, out[4] = column-sum jobs, out[5] / out[6] / out[7] = offsets (floats)
 *   inside the workspace of the INPUT features [n_tokens][384] (the CNN writes them there), of their gradient [n_tokens][384]
 *   and of y_hat [n_clips][n_heads]; the loss (total, then one term per head) follows y_hat at out[7] + round_up(n_clips *
 *   n_heads, 4); from out[8]: the GEMM descriptors [groups][10] then the column-sum jobs [jobs][6] (int64), which the caller
 *   uploads and passes back as wgrad_desc / colsum_jobs.  cap = capacity of out in int64s.
 * nisqa_tdtrain_step: forward, loss, backward.  Adds every parameter gradient of the block into `grads` (zeroed by the
 *   caller), writes y_hat, loss and the feature gradient.  labels [n_clips][n_heads] (NaN = unlabelled), bias_map [n_clips][4]
 *   cubic coefficients (one mapping per clip, applied to every head) or NULL, inv_count [n_heads] = 1 / (labelled clips of the whole batch, all ranks) or 0.  mask_* are the
 *   dropout multipliers of each layer in the CALLER's token order (mask_p: [sum L^2] attention probabilities, row-major per
 *   clip at sq_off; mask_1 / mask_f / mask_2: [n_tokens][64]) or NULL.
 * nisqa_tdtrain_step_heads: the same step with bias_map read as [n_clips][n_heads][4], one mapping per clip and head (see
 *   nisqa_mse_loss_heads); everything else, the layout of the arguments included, is nisqa_tdtrain_step's. */
typedef struct nisqa_tdtrain_args {
    int32_t n_clips, n_tokens, n_tokens_padded, n_layers, n_heads, n_wgrad_groups, n_wgrad_tiles, n_colsum_jobs;
    const int32_t* seg_off;      /* device [n_clips + 1] */
    const int32_t* ptok_off;     /* device [n_clips + 1] */
    const int32_t* tile_clip;    /* device [n_tokens_padded / 32] */
    const int64_t* sq_off;       /* device [n_clips + 1]: prefix sum of L^2 */
    const float* params;         /* device, flat parameter buffer */
    float* grads;                /* device, flat gradient buffer (same offsets) */
    const int32_t* poff;         /* HOST */
    float* ws;                   /* device, out[0] floats */
    float* frags;                /* device, out[1] floats */
    const float* labels;         /* device */
    const float* bias_map;       /* device or NULL: [n_clips][4], or [n_clips][n_heads][4] for nisqa_tdtrain_step_heads */
    const float* inv_count;      /* device [n_heads] */
    const float* mask_p[4];
    const float* mask_1[4];
    const float* mask_f[4];
    const float* mask_2[4];
    const int64_t* wgrad_desc;   /* device [n_wgrad_groups][10] */
    const int64_t* colsum_jobs;  /* device [n_colsum_jobs][6] */
} nisqa_tdtrain_args;
int nisqa_tdtrain_plan(int32_t n_clips, int32_t n_tokens, int32_t n_tokens_padded, int32_t n_layers, int32_t n_heads,
                       const int32_t* poff, int64_t* out, int64_t cap);
int nisqa_tdtrain_step(const nisqa_tdtrain_args* args, void* stream);
int nisqa_tdtrain_step_heads(const nisqa_tdtrain_args* args, void* stream);

/* ---- NISQA_DE (double-ended) training: alignment + fusion between the two self-attention blocks, forward and backward --------
 * Replaces, in the training step, Alignment.forward with AttDot / AttCosine and ApplyHardAttention (nisqa/NISQA_lib.py:
 * 1264-1294, 1359-1366), Fusion.forward without lin_fusion (:1405-1417) as NISQA_DE.forward calls them (:414-419), and what
 * autograd derives from them in loss.backward() (NISQA_model.py:139).
 *
 * Layout (both entries): PACKED token rows, as the training step keeps them -- no padding rows anywhere.  x / d_deg / d_ref are
 * [tokens][64]; pair b's degraded tokens are rows deg_tok_off[b] .. + deg_n_wins[b] - 1, its reference tokens rows
 * ref_tok_off[b] .. + ref_n_wins[b] - 1 (offsets in rows; every n_wins >= 1).  out / d_fused / idx are indexed by the DEGRADED
 * rows: row deg_tok_off[b] + i holds token i of pair b (ld_out / ld floats per row, the fused width F = 192 for fuse 0 'x/y/-',
 * 128 for 1 '+/-' and 2 'x/y' in columns 0 .. F-1; columns behind F are neither read nor written).
 *
 * nisqa_de_align_fuse_packed: nisqa_de_align_fuse (nisqa_hip.h: same kernel source, same arithmetic, same argmax rule -- raw
 *   scores, lowest index on a tie) with apply = hard at packed offsets.  tile_off [n_pairs + 1]: exclusive prefix sum of
 *   ceil(deg_n_wins[b] / 64); n_tiles = tile_off[n_pairs].  Writes out and idx (the chosen reference token, 0-based within the
 *   pair's reference clip) for every degraded row and nothing else.
 *
 * nisqa_de_align_fuse_bwd: d_fused = d loss / d fused, idx as written by the forward ->
 *     d_deg[deg row i]  = g0 + g2 (fuse 0) | g0 + g1 (fuse 1) | g0 (fuse 2)
 *     d_ref[ref row j]  = sum over i with idx[i] == j of dya[i],  dya = g1 - g2 (0) | g0 - g1 (1) | g1 (2)
 *   with g0, g1, g2 the 64-column blocks of a d_fused row.  d_deg and d_ref may be the same buffer (the forward's x layout) or
 *   two buffers, each addressed by its own side's offsets.  max_n_wins >= every n_wins of both sides (it sizes the grid).
 *   Contract:
 *     - no floating-point atomics: each reference row's sum is taken in ascending i, in fp32, starting from +0 -- deterministic,
 *       and bit for bit the sequential fp32 sum;
 *     - every row of every token of both sides is written, reference rows no degraded token chose as zeros: the caller does
 *       not pre-zero;
 *     - the layout has no padding rows; no other row of d_deg / d_ref is touched;
 *     - an idx outside [0, ref_n_wins[b]) matches no row and contributes nowhere (it cannot cause an access out of bounds). */
int nisqa_de_align_fuse_packed(const float* x, const int32_t* deg_tok_off, const int32_t* deg_n_wins, const int32_t* ref_tok_off,
                               const int32_t* ref_n_wins, const int32_t* tile_off, int32_t n_pairs, int32_t n_tiles, int32_t align,
                               int32_t fuse, int32_t ld_out, float* out, int32_t* idx_out, void* stream);
int nisqa_de_align_fuse_bwd(const float* d_fused, int32_t ld, const int32_t* idx, const int32_t* deg_tok_off,
                            const int32_t* deg_n_wins, const int32_t* ref_tok_off, const int32_t* ref_n_wins, int32_t n_pairs,
                            int32_t max_n_wins, int32_t fuse, float* d_deg, float* d_ref, void* stream);

/* ---- SOFT alignment at the packed layout, forward with kept statistics, and its backward (d model(x, n_wins) / d x of NISQA_DE
 * checkpoints with de_align_apply = soft, nisqa_amd/input_grad.py) -------------------------------------------
 * Layout and arguments as above.  lse [degraded rows] and aligned [degraded rows][64] are indexed like out / d_fused.
 *
 * nisqa_de_align_soft_packed: nisqa_de_align_fuse with apply = soft at packed offsets (the same kernel source, the same
 *   arithmetic: the fused rows are bit for bit those of nisqa_de_align_fuse(apply = 1) on the same valid rows).  Per degraded
 *   row i it also writes lse[i] = M_i + log L_i (the row's score maximum and its sum of exp(s_ij - M_i) over the pair's valid
 *   reference tokens), so that the attention weights are p_ij = exp(s_ij - lse[i]), and aligned[i] = a_i = sum_j p_ij y_j, the
 *   row the fusion combined with x_i.  Writes out, lse and aligned for every degraded row and nothing else.
 *
 * nisqa_de_align_soft_bwd: x, lse and aligned as the forward read / wrote them, d_fused = d loss / d fused ->
 *     s_ij = q^_i . y^_j     p_ij = exp(s_ij - lse[i])     delta_i = ga_i . a_i     ds_ij = p_ij (ga_i . y_j - delta_i)
 *     d_deg[deg row i] = gx_i + N'(q_i)[ sum_j ds_ij y^_j ]
 *     d_ref[ref row j] = sum_i p_ij ga_i + N'(y_j)[ sum_i ds_ij q^_i ]
 *   q_i / y_j: the pair's degraded / reference rows of x; q^, y^: the rows divided by max(||.||, 1e-8) for align 1 (cosine), the
 *   rows themselves for align 0 (dot); gx_i / ga_i: d_deg and dya of nisqa_de_align_fuse_bwd; N'(v)[u] = (u - v^ (v^ . u)) / ||v||
 *   for cosine (u / 1e-8 for a row whose norm is at or under the clamp), u for dot.  Sums over the pair's valid tokens only.
 *   Contract:
 *     - a score is recomputed with the forward's k-ordered fp32 fma chain on the forward's operands; everything is fp32;
 *     - two launches (one workgroup per 64 degraded tokens of a pair, then one per 64 reference tokens), no floating-point
 *       atomics, every sum in a fixed order: two runs give the same bits;
 *     - every row of every token of both sides is written once (the caller does not pre-zero), no other row is touched;
 *       d_deg and d_ref may be one buffer in x's layout;
 *     - ld is a multiple of 4 and d_fused 16-byte aligned (rows are read as 16-byte vectors).
 * Both return NISQA_ERR_ARG before any launch for a NULL pointer, n_pairs <= 0, align outside {0, 1}, fuse outside {0, 1, 2},
 * ld_out / ld below the fused width or not a multiple of 4, n_tiles < n_pairs, max_n_wins <= 0 or n_pairs > 65535. */
int nisqa_de_align_soft_packed(const float* x, const int32_t* deg_tok_off, const int32_t* deg_n_wins, const int32_t* ref_tok_off,
                               const int32_t* ref_n_wins, const int32_t* tile_off, int32_t n_pairs, int32_t n_tiles, int32_t align,
                               int32_t fuse, int32_t ld_out, float* out, float* lse, float* aligned, void* stream);
int nisqa_de_align_soft_bwd(const float* x, const float* d_fused, int32_t ld, const float* lse, const float* aligned,
                            const int32_t* deg_tok_off, const int32_t* deg_n_wins, const int32_t* ref_tok_off,
                            const int32_t* ref_n_wins, int32_t n_pairs, int32_t max_n_wins, int32_t align, int32_t fuse,
                            float* d_deg, float* d_ref, void* stream);

/* ---- resident training spectrograms (tr_ds_to_memory): one batch out of the store --------------------------------------------
 * The store (nisqa_amd/melstore.py) keeps the dB spectrogram of every clip of a dataset in ONE device arena, store
 * [store_rows][48] float32, clip after clip: clip i's rows are clip_row[i] .. clip_row[i + 1] - 1 (clip_row [n_store + 1], int64,
 * an exclusive prefix sum; clip_row[n_store] = store_rows) and store_floor[i] is its top_db floor.  nisqa_mel_gather copies the n
 * clips ids[0 .. n-1] (any order, repeats allowed) into out_mel [out_frames][48]: clip ids[c] to the rows out_frame_off[c] ..
 * out_frame_off[c + 1] - 1 (out_frame_off [n + 1], int32, an exclusive prefix sum of the clips' stored lengths; out_frame_off[n]
 * = out_frames), and writes out_floor[c] = store_floor[ids[c]].  Every pointer is device memory; store and out_mel are 16-byte
 * aligned (a row is 192 B = twelve 16-byte units; the copy moves whole units).  One launch on `stream`, no workspace.
 *
 * Returns NISQA_ERR_ARG before any launch for a NULL pointer, a store or out_mel that is not 16-byte aligned, n <= 0,
 * n_store <= 0, out_frames <= 0 or store_rows <= 0.  The tables themselves are the caller's to check (melstore.MelStore.batch does,
 * on the host).  On the device an entry is skipped, not trusted, if its id is outside [0, n_store), if its output span is not
 * exactly the stored length, or if its stored rows leave [0, store_rows): its output rows are left unwritten and its floor is set
 * to NaN; every other entry is copied exactly.  No address outside [store, store + store_rows * 48) or outside out_mel
 * [out_frames][48] / out_floor [n] is ever formed.  The offsets of at most NISQA_MEL_GATHER_LDS_CLIPS clips are staged in LDS; a
 * longer list is searched in global memory.  Bitwise copies: no arithmetic, no atomics. */
#define NISQA_MEL_GATHER_LDS_CLIPS 1024
int nisqa_mel_gather(const float* store, int64_t store_rows, const int64_t* clip_row, const float* store_floor, int32_t n_store,
                     const int32_t* ids, const int32_t* out_frame_off, int32_t n, int32_t out_frames, float* out_mel,
                     float* out_floor, void* stream);

/* ---- the gradient of model(x, n_wins) with respect to x: the eval-mode AdaptCNN with its activations kept (csrc/input_grad.hip) ----
 * After model.eval() the reference's NISQA / NISQA_DIM are differentiable functions of the segment tensor x [B, L, 1, 48, 15]
 * (nisqa/NISQA_lib.py:137-142, 260-268, 688-710): BatchNorm normalises by the RUNNING statistics and there is no dropout, so
 * neither the forward nor the backward of the training step's layers applies (no statistics terms), and conv1 needs an input
 * gradient.  Activations and arg as above: [S][H*W][C] over the S VALID segments packed clip after clip (seg_off [n_clips + 1]);
 * valid segment seg_off[b] + k is row b * l_max + k of x.  The attention half of the backward runs on the training operators.
 *
 *   nisqa_bn_eval_act_pool_fwd  y[S][ho*wo][c] = adaptive_max_pool(relu(scale z + shift)), scale = gamma / sqrt(running_var + 1e-5),
 *                               shift = beta - running_mean scale; arg = the pixel (y * w + x) of each maximum, the first one in
 *                               (y, x) order on a tie -- NOT written (and may be NULL) when ho == h and wo == w, as in
 *                               nisqa_bn_act_pool_fwd.  The running statistics are read only.
 *   nisqa_bn_eval_act_pool_bwd  dz[S][h*w][c] = scale * (sum of dy over the cells whose maximum the pixel is) where the
 *                               pre-activation scale z + shift is positive, 0 elsewhere.  Every element of dz is written (no
 *                               clearing pass); a gather per pixel in a fixed order, no atomics.
 *   nisqa_conv1_segments_fwd    z[S][720][16] = conv1(x rows) + bias, w [16][9] with tap = dy * 3 + dx, pixel = band * 15 + frame.
 *   nisqa_conv1_segments_dgrad  dx [n_clips][l_max][48][15] (the layout of x): row (b, l) = sum_co sum_tap dz[seg_off[b] + l]
 *                               [pixel - tap offset][co] w[co][tap] for l < the clip's segment count, zeros for the padding
 *                               rows.  Every element of dx is written; a gather per pixel in a fixed order, no atomics: two
 *                               runs give the same bits.
 * c % 4 == 0, c <= 256, 16-byte aligned buffers.  NULL pointers and non-positive sizes return NISQA_ERR_ARG before any launch. */
int nisqa_bn_eval_act_pool_fwd(const float* z, const float* gamma, const float* beta, const float* running_mean,
                               const float* running_var, int32_t n_segments, int32_t h, int32_t w, int32_t c, int32_t ho, int32_t wo,
                               float* y, int32_t* arg, void* stream);
int nisqa_bn_eval_act_pool_bwd(const float* dy, const int32_t* arg, const float* z, const float* gamma, const float* beta,
                               const float* running_mean, const float* running_var, int32_t n_segments, int32_t h, int32_t w,
                               int32_t c, int32_t ho, int32_t wo, float* dz, void* stream);
int nisqa_conv1_segments_fwd(const float* x, int32_t l_max, const int32_t* seg_off, int32_t n_clips, int32_t n_segments,
                             const float* w, const float* bias, float* z, void* stream);
int nisqa_conv1_segments_dgrad(const float* dz, const int32_t* seg_off, int32_t n_clips, int32_t l_max, const float* w, float* dx,
                               void* stream);
/* The same pair for the pooled layers of the StandardCNN (NISQA_lib.py:712-836: pool_first = MaxPool2d(2, stride 2, padding (0, 1))
 * after conv1, MaxPool2d(2) after conv2 and conv4), which no adaptive window expresses: ho = h / 2, wo = (w + 2 pad_w - 2) / 2 + 1,
 * cell (oy, ox) = rows 2 oy, 2 oy + 1 x columns 2 ox - pad_w, 2 ox - pad_w + 1 (48 x 15, pad_w 1 -> 24 x 8 with the column windows
 * {0}, {1, 2}, ..., {13, 14}).  The padding column never wins; arg [S][ho*wo][c] is always written.  The windows do not overlap:
 * the backward gathers nothing, dz[pixel] = scale * dy[its cell] where the pixel is the cell's maximum and scale z + shift > 0,
 * 0 elsewhere (also for a last column that no window covers).  h even, pad_w 0 or 1, w + 2 pad_w >= 2, c as above; anything else
 * returns NISQA_ERR_ARG.  The layers without a pool use nisqa_bn_eval_act_pool_fwd / _bwd with ho = h, wo = w. */
int nisqa_bn_eval_act_maxpool2_fwd(const float* z, const float* gamma, const float* beta, const float* running_mean,
                                   const float* running_var, int32_t n_segments, int32_t h, int32_t w, int32_t c, int32_t pad_w,
                                   float* y, int32_t* arg, void* stream);
int nisqa_bn_eval_act_maxpool2_bwd(const float* dy, const int32_t* arg, const float* z, const float* gamma, const float* beta,
                                   const float* running_mean, const float* running_var, int32_t n_segments, int32_t h, int32_t w,
                                   int32_t c, int32_t pad_w, float* dz, void* stream);

/* ---- the gradient with respect to the AUDIO: backward of the mel front end and of the segmenting (csrc/mel_bwd.hip) ----
 * Carries d L / d x of model(x, n_wins) back to the samples: segments -> clamped dB rows -> top_db floor -> dB -> filter bank ->
 * |STFT| -> window -> reflect padding.  The function differentiated is the forward's (nisqa_mel_db + nisqa_mel_finalize), per clip
 * of L samples: frame f, tap n < win reads sample refl(f hop + start0 + n), start0 = -n_fft / 2 + (n_fft - win) / 2, refl: i -> -i
 * below 0, i -> 2 (L - 1) - i from L on; X_k = sum_n w_n x_n e^(-2 pi i k n / 4096), k = 0 .. 2048; M_m = sum_k fb[m][k] |X_k|;
 * db = 10 log10(max(amin_sq, M_m^2)); out = max(db, max_clip(db) - top_db).  cfg and the tables are the forward's.
 *
 *   nisqa_segments_to_mel_bwd      dmel[TT][48]: element (t, m) of clip b = sum over the segments k < n_wins[b] with seg_hop k <= t <=
 *                                  seg_hop k + 14 of dx[b][k][0][m][t - seg_hop k], k ascending; 0 for a frame no segment holds.
 *                                  dx is [n_clips][l_max][1][48][15]; its rows k >= n_wins[b] are never read.
 *   nisqa_mel_db_bwd_gate          dmel_amp[TT][48] = d L / d M from g = d L / d out, the forward's UNCLAMPED dB rows and its clip_floor:
 *                                  an element passes g where db > clip_floor; the g of every other element of the clip goes to the
 *                                  clip's maximum (the derivative of max(db) - top_db), on a tie the FIRST maximum in (frame, band)
 *                                  order; d db / d M = 20 / (ln 10 M) where db is above the forward's value of 10 log10(amin_sq), else
 *                                  0.  Both gates are taken on the forward's own bits; M is recovered from the stored dB.
 *   nisqa_mel_bwd_workspace_bytes  total_frames * win floats (0 for sizes the entries refuse)
 *   nisqa_mel_frame_bwd            ws[TT][win]: per frame the gradient of its win windowed samples.  X is recomputed (4096-point FFT
 *                                  in LDS), d L / d |X_k| = sum_m fb[m][k] dmel_amp[m], d L / d x_n = w_n Re sum_{k = 0}^{2048}
 *                                  (d L / d |X_k| X_k / |X_k|) e^(+2 pi i k n / 4096) -- one-sided, not doubled; a term is 0 where
 *                                  |X_k| = 0.  A frame whose 48 gradients are all 0 writes exact zeros.  A clip's frames read that
 *                                  clip's samples only.  The sparse bank must be triangular: bands m and m + 2 share no bin with a
 *                                  non-zero weight.
 *   nisqa_mel_overlap_add_bwd      dpcm[total_samples]: per sample the taps of every frame over every padded position that reflects
 *                                  onto it (itself, the left and the right reflection), in a fixed order.  Exact for clips whose
 *                                  padding reflects once (L > win / 2 + hop, as every clip of >= 15 frames).
 * No atomics: every output element is written once, two calls give the same bits.  float PCM only (int16 PCM has no gradient).
 * NULL pointers, non-positive or impossible sizes (n_clips > total_frames, win outside [2, 4096], n_fft != 4096, ...) return
 * NISQA_ERR_ARG before any launch; a workspace smaller than nisqa_mel_bwd_workspace_bytes returns NISQA_ERR_WORKSPACE. */
int nisqa_segments_to_mel_bwd(const float* dx, int32_t l_max, const int32_t* n_wins, const int32_t* frame_off, int32_t n_clips,
                              int32_t total_frames, int32_t seg_hop, float* dmel, void* stream);
int nisqa_mel_db_bwd_gate(const float* g, const float* mel_db, const float* clip_floor, const int32_t* frame_off, int32_t n_clips,
                          int32_t total_frames, const nisqa_mel_cfg* cfg, float* dmel_amp, void* stream);
int64_t nisqa_mel_bwd_workspace_bytes(int32_t total_frames, int32_t win);
int nisqa_mel_frame_bwd(const float* pcm, const int64_t* clip_off, const int32_t* frame_off, int32_t n_clips, int32_t total_frames,
                        const nisqa_mel_cfg* cfg, const float* window, const float* twiddle, const int32_t* band_start,
                        const int32_t* band_len, const int32_t* band_woff, const float* band_w, const float* dmel_amp, float* ws,
                        int64_t ws_bytes, void* stream);
int nisqa_mel_overlap_add_bwd(const float* ws, const int64_t* clip_off, const int32_t* frame_off, int32_t n_clips,
                              int32_t total_frames, int64_t total_samples, const nisqa_mel_cfg* cfg, float* dpcm, void* stream);
/* The forward counterpart of nisqa_segments_to_mel_bwd: the clamped segment tensor the segment-fed CNN reads, cut on the device
 * from the UNCLAMPED dB rows and the clip floors of nisqa_mel_db + nisqa_mel_finalize(clamp = 0).
 *   x[b][k][0][m][j] = fmaxf(mel_db[frame_off[b] + seg_hop k + j][m], clip_floor[b])   for k < n_wins[b], m < 48, j < 15
 *   x[b][k][0][m][j] = 0                                                               for n_wins[b] <= k < L
 * x is [n_clips][L][1][48][15] and may be uninitialised: every element is written once, by one thread (no atomics: two calls
 * give the same bits); nothing behind it is touched.  No arithmetic but the clamp: the values are mel_db's or clip_floor's bits.
 * The caller keeps L >= the largest n_wins[b] (a smaller L cuts the first L segments of a clip) and the plan's invariant
 * seg_hop (n_wins[b] - 1) + 15 <= frame_off[b + 1] - frame_off[b]; a segment that would read past its clip's frames is written
 * as zeros instead.  Offsets into x are 64-bit.  mel_db and x must be 16-byte aligned (the rows move as 128-bit words).
 * NULL pointers, n_clips <= 0, total_frames <= 0, n_clips > total_frames, seg_hop < 1, L < 1, n_clips * L >= 2^31 or a misaligned
 * mel_db / x return NISQA_ERR_ARG before any launch. */
int nisqa_mel_segments_fwd(const float* mel_db, const float* clip_floor, const int32_t* frame_off, const int32_t* n_wins,
                           int32_t n_clips, int32_t total_frames, int32_t seg_hop, int32_t L, float* x, void* stream);

#ifdef __cplusplus
}
#endif
#endif
