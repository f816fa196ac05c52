// The eval-mode AdaptCNN with its activations kept, and its gradient with respect to the INPUT segments: what autograd does for
// d model(x, n_wins) / d x after model.eval() (BatchNorm on the running statistics, no dropout; nisqa/NISQA_lib.py:688-710).  The
// training step cannot lend its kernels here: its BatchNorm normalises by batch statistics and its backward carries their terms,
// and it has no input gradient of conv1 because a spectrogram never needed one.  Host side: nisqa_amd/input_grad.py.
// The StandardCNN of the BiLSTM models (NISQA_lib.py:712-836) shares conv1 and the identity layers and has its own pools: the
// bn_eval_act_maxpool2 pair below.
//
// Layouts are the training step's (include/nisqa_train.h): activations [S][H*W][C] with the channels contiguous, S = the VALID
// segments of the batch packed clip after clip (seg_off), arg = pixel (y * W + x) of every pooled maximum.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.hpp"
#include "../../include/nisqa_hip.h"
#include "../../include/nisqa_train.h"

// BatchNorm on the running statistics as one multiply-add per element: y = z * scale + shift, scale = gamma / sqrt(var + eps),
// shift = beta - mean * scale, for four consecutive channels.  Forward and backward derive the ReLU gate from this one
// expression (bn_apply), so the two agree on every element's side of zero.
NQ_DEV void bn_eval_affine4(const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ mean,
                            const float* __restrict__ var, int ch, f32x4& scale, f32x4& shift) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const double s = (double)gamma[ch + e] / sqrt((double)var[ch + e] + 1e-5);
        scale[e] = (float)s;
        shift[e] = (float)((double)beta[ch + e] - (double)mean[ch + e] * s);
    }
}

NQ_DEV f32x4 bn_apply(const f32x4 z, const f32x4 scale, const f32x4 shift) {
    f32x4 y;
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = fmaf(z[e], scale[e], shift[e]);
    return y;
}

// One thread = four consecutive channels of one OUTPUT cell.  In the compiled shapes c / 4 divides the 256-thread stride: a
// thread meets the same four channels in every iteration and derives their constants once.
template <int H, int W, int C, int HO, int WO>
__global__ __launch_bounds__(256) void bn_eval_act_pool_fwd_kernel(
    const float* __restrict__ z, const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ mean,
    const float* __restrict__ var, int64_t total4, int h_, int w_, int c_, int ho_, int wo_, float* __restrict__ y,
    int32_t* __restrict__ arg) {
    const int h = H ? H : h_, w = H ? W : w_, c = H ? C : c_, ho = H ? HO : ho_, wo = H ? WO : wo_;
    const int c4 = c / 4;
    constexpr bool INV = H != 0 && 256 % ((C ? C : 4) / 4) == 0;
    const bool identity = h == ho && w == wo;               // layers 3, 5, 6: the winner is the cell itself, arg is not written
    f32x4 sc, sh;
    if (INV) bn_eval_affine4(gamma, beta, mean, var, 4 * ((int)threadIdx.x % c4), sc, sh);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int ch = 4 * (int)(i % c4);
        const int64_t op = i / c4;
        const int64_t s = op / (ho * wo);
        const int o = (int)(op - s * (ho * wo));
        const int oy = o / wo, ox = o % wo;
        if (!INV) bn_eval_affine4(gamma, beta, mean, var, ch, sc, sh);
        f32x4 best = {-3.0e38f, -3.0e38f, -3.0e38f, -3.0e38f};
        i32x4 bp = {0, 0, 0, 0};
        for (int yy = win_lo(oy, h, ho); yy < win_hi(oy, h, ho); ++yy)
            for (int xx = win_lo(ox, w, wo); xx < win_hi(ox, w, wo); ++xx) {
                const int p = yy * w + xx;
                const f32x4 v = bn_apply(*(const f32x4*)(z + (s * (h * w) + p) * c + ch), sc, sh);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float r = fmaxf(v[e], 0.f);
                    if (r > best[e]) { best[e] = r; bp[e] = p; }         // the first maximum in (y, x) order, as PyTorch
                }
            }
        ((f32x4*)y)[i] = best;
        if (!identity) ((i32x4*)arg)[i] = bp;
    }
}

// One thread = four consecutive channels of one INPUT pixel: it gathers the gradient of every pooling cell whose window holds
// the pixel and whose maximum it is (adaptive windows overlap: up to 2 x 2 cells), gates it with the ReLU and scales it.  Every
// element of dz is written exactly once, by one thread, in a fixed order of additions: no clearing pass, no atomics.
template <int H, int W, int C, int HO, int WO>
__global__ __launch_bounds__(256) void bn_eval_act_pool_bwd_kernel(
    const float* __restrict__ dy, const int32_t* __restrict__ arg, const float* __restrict__ z, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ mean, const float* __restrict__ var, int64_t total4, int h_, int w_,
    int c_, int ho_, int wo_, float* __restrict__ dz) {
    const int h = H ? H : h_, w = H ? W : w_, c = H ? C : c_, ho = H ? HO : ho_, wo = H ? WO : wo_;
    const int c4 = c / 4;
    constexpr bool INV = H != 0 && 256 % ((C ? C : 4) / 4) == 0;
    f32x4 sc, sh;
    if (INV) bn_eval_affine4(gamma, beta, mean, var, 4 * ((int)threadIdx.x % c4), sc, sh);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int ch = 4 * (int)(i % c4);
        const int64_t pix = i / c4;
        const int64_t s = pix / (h * w);
        const int p = (int)(pix - s * (h * w));
        const int yy = p / w, xx = p % w;
        if (!INV) bn_eval_affine4(gamma, beta, mean, var, ch, sc, sh);
        const f32x4 yb = bn_apply(((const f32x4*)z)[i], sc, sh);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const bool live = yb[0] > 0.f || yb[1] > 0.f || yb[2] > 0.f || yb[3] > 0.f;
        if (h == ho && w == wo) {                           // identity pooling: the only window of pixel p is p itself
            acc = ((const f32x4*)dy)[i];
        } else if (live) {
            const int oy0 = max(0, (yy * ho) / h - 1), oy1 = min(ho - 1, ((yy + 1) * ho) / h + 1);
            const int ox0 = max(0, (xx * wo) / w - 1), ox1 = min(wo - 1, ((xx + 1) * wo) / w + 1);
            for (int oy = oy0; oy <= oy1; ++oy) {
                if (yy < win_lo(oy, h, ho) || yy >= win_hi(oy, h, ho)) continue;
                for (int ox = ox0; ox <= ox1; ++ox) {
                    if (xx < win_lo(ox, w, wo) || xx >= win_hi(ox, w, wo)) continue;
                    const int64_t o = (s * (ho * wo) + oy * wo + ox) * c + ch;
                    const i32x4 ag = *(const i32x4*)(arg + o);
                    const f32x4 d = *(const f32x4*)(dy + o);
#pragma unroll
                    for (int e = 0; e < 4; ++e) if (ag[e] == p) acc[e] += d[e];
                }
            }
        }
        f32x4 out;
#pragma unroll
        for (int e = 0; e < 4; ++e) out[e] = yb[e] > 0.f ? sc[e] * acc[e] : 0.f;
        ((f32x4*)dz)[i] = out;
    }
}

// the six layer shapes of the AdaptCNN get their own instantiation, anything else the generic one
#define NQ_EVAL_POOL_DISPATCH(KERNEL, GRID, ST, ...)                                                              \
    do {                                                                                                          \
        if (h == 48 && w == 15 && c == 16 && ho == 24 && wo == 7) hipLaunchKernelGGL((KERNEL<48, 15, 16, 24, 7>), GRID, dim3(256), 0, ST, __VA_ARGS__);   \
        else if (h == 24 && w == 7 && c == 32 && ho == 12 && wo == 5) hipLaunchKernelGGL((KERNEL<24, 7, 32, 12, 5>), GRID, dim3(256), 0, ST, __VA_ARGS__); \
        else if (h == 12 && w == 5 && c == 64 && ho == 12 && wo == 5) hipLaunchKernelGGL((KERNEL<12, 5, 64, 12, 5>), GRID, dim3(256), 0, ST, __VA_ARGS__); \
        else if (h == 12 && w == 5 && c == 64 && ho == 6 && wo == 3) hipLaunchKernelGGL((KERNEL<12, 5, 64, 6, 3>), GRID, dim3(256), 0, ST, __VA_ARGS__);   \
        else if (h == 6 && w == 3 && c == 64 && ho == 6 && wo == 3) hipLaunchKernelGGL((KERNEL<6, 3, 64, 6, 3>), GRID, dim3(256), 0, ST, __VA_ARGS__);     \
        else if (h == 6 && w == 1 && c == 64 && ho == 6 && wo == 1) hipLaunchKernelGGL((KERNEL<6, 1, 64, 6, 1>), GRID, dim3(256), 0, ST, __VA_ARGS__);     \
        else hipLaunchKernelGGL((KERNEL<0, 0, 0, 0, 0>), GRID, dim3(256), 0, ST, __VA_ARGS__);                     \
    } while (0)

// one resident round of workgroups (256 CUs x 8 blocks x 2): a thread sees several elements and its constants are worth keeping
static int grid_resident(int64_t total) {
    const int64_t g = (total + 255) / 256;
    return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

static bool pool_shape_ok(int32_t n_segments, int32_t h, int32_t w, int32_t c, int32_t ho, int32_t wo) {
    return n_segments > 0 && h > 0 && w > 0 && c > 0 && c <= 256 && !(c & 3) && ho > 0 && wo > 0 && ho <= h && wo <= w;
}

extern "C" int nisqa_bn_eval_act_pool_fwd(const float* z, const float* gamma, const float* beta, const float* running_mean,
                                          const float* running_var, int32_t n_segments, int32_t h, int32_t w, int32_t c, int32_t ho,
                                          int32_t wo, float* y, int32_t* arg, void* stream) {
    if (!z || !gamma || !beta || !running_mean || !running_var || !y || !pool_shape_ok(n_segments, h, w, c, ho, wo) ||
        (!arg && !(h == ho && w == wo)))
        return NISQA_ERR_ARG;
    const int64_t total = (int64_t)n_segments * ho * wo * c / 4;
    NQ_LAUNCH_BEGIN();
    NQ_EVAL_POOL_DISPATCH(bn_eval_act_pool_fwd_kernel, dim3(grid_resident(total)), (hipStream_t)stream, z, gamma, beta, running_mean,
                          running_var, total, h, w, c, ho, wo, y, arg);
    return NQ_LAUNCH_STATUS();
}

extern "C" int nisqa_bn_eval_act_pool_bwd(const float* dy, const int32_t* arg, const float* z, const float* gamma, const float* beta,
                                          const float* running_mean, const float* running_var, int32_t n_segments, int32_t h,
                                          int32_t w, int32_t c, int32_t ho, int32_t wo, float* dz, void* stream) {
    if (!dy || !z || !gamma || !beta || !running_mean || !running_var || !dz || !pool_shape_ok(n_segments, h, w, c, ho, wo) ||
        (!arg && !(h == ho && w == wo)))
        return NISQA_ERR_ARG;
    const int64_t total = (int64_t)n_segments * h * w * c / 4;
    NQ_LAUNCH_BEGIN();
    NQ_EVAL_POOL_DISPATCH(bn_eval_act_pool_bwd_kernel, dim3(grid_resident(total)), (hipStream_t)stream, dy, arg, z, gamma, beta,
                          running_mean, running_var, total, h, w, c, ho, wo, dz);
    return NQ_LAUNCH_STATUS();
}

// ---------------------------------------------------------------------------------------------------------
// The StandardCNN's pools: MaxPool2d(2, stride 2, padding (0, pad_w)) behind the frozen BatchNorm + ReLU
// ---------------------------------------------------------------------------------------------------------
// Output cell (oy, ox) covers rows 2 oy, 2 oy + 1 and columns 2 ox - pad_w, 2 ox - pad_w + 1; a column outside [0, w) is padding
// (-inf in PyTorch: it never wins, and every window holds at least one real column).  The windows do not overlap, and with an
// odd w + 2 pad_w the last real column belongs to no window (floor mode).  pool_first of the StandardCNN is pad_w = 1 on 48 x 15:
// 8 columns with the windows {0}, {1, 2}, ..., {13, 14} (NISQA_lib.py:712-836).
NQ_DEV int mp2_wo(int w, int pad_w) { return (w + 2 * pad_w - 2) / 2 + 1; }

// One thread = four consecutive channels of one OUTPUT cell, as bn_eval_act_pool_fwd_kernel.
template <int H, int W, int C, int PAD>
__global__ __launch_bounds__(256) void bn_eval_act_maxpool2_fwd_kernel(
    const float* __restrict__ z, const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ mean,
    const float* __restrict__ var, int64_t total4, int h_, int w_, int c_, int pad_, float* __restrict__ y,
    int32_t* __restrict__ arg) {
    const int h = H ? H : h_, w = H ? W : w_, c = H ? C : c_, pad = H ? PAD : pad_;
    const int ho = h / 2, wo = mp2_wo(w, pad);
    const int c4 = c / 4;
    constexpr bool INV = H != 0 && 256 % ((C ? C : 4) / 4) == 0;
    f32x4 sc, sh;
    if (INV) bn_eval_affine4(gamma, beta, mean, var, 4 * ((int)threadIdx.x % c4), sc, sh);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int ch = 4 * (int)(i % c4);
        const int64_t op = i / c4;
        const int64_t s = op / (ho * wo);
        const int o = (int)(op - s * (ho * wo));
        const int oy = o / wo, ox = o % wo;
        if (!INV) bn_eval_affine4(gamma, beta, mean, var, ch, sc, sh);
        f32x4 best = {-3.0e38f, -3.0e38f, -3.0e38f, -3.0e38f};
        i32x4 bp = {0, 0, 0, 0};
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int yy = 2 * oy + dy, xx = 2 * ox - pad + dx;
                if ((unsigned)xx >= (unsigned)w) continue;                   // the padding column
                const int p = yy * w + xx;
                const f32x4 v = bn_apply(*(const f32x4*)(z + (s * (h * w) + p) * c + ch), sc, sh);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float r = fmaxf(v[e], 0.f);
                    if (r > best[e]) { best[e] = r; bp[e] = p; }         // the first maximum in (y, x) order, as PyTorch
                }
            }
        ((f32x4*)y)[i] = best;
        ((i32x4*)arg)[i] = bp;
    }
}

// One thread = four consecutive channels of one INPUT pixel.  The pixel belongs to at most one cell, so there is nothing to
// gather: dz = scale * dy of that cell where the pixel is its maximum and the pre-activation is positive, 0 elsewhere (and for
// the column no window covers).  Every element of dz is written exactly once: no clearing pass, no atomics.
template <int H, int W, int C, int PAD>
__global__ __launch_bounds__(256) void bn_eval_act_maxpool2_bwd_kernel(
    const float* __restrict__ dy, const int32_t* __restrict__ arg, const float* __restrict__ z, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ mean, const float* __restrict__ var, int64_t total4, int h_, int w_,
    int c_, int pad_, float* __restrict__ dz) {
    const int h = H ? H : h_, w = H ? W : w_, c = H ? C : c_, pad = H ? PAD : pad_;
    const int ho = h / 2, wo = mp2_wo(w, pad);
    const int c4 = c / 4;
    constexpr bool INV = H != 0 && 256 % ((C ? C : 4) / 4) == 0;
    f32x4 sc, sh;
    if (INV) bn_eval_affine4(gamma, beta, mean, var, 4 * ((int)threadIdx.x % c4), sc, sh);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int ch = 4 * (int)(i % c4);
        const int64_t pix = i / c4;
        const int64_t s = pix / (h * w);
        const int p = (int)(pix - s * (h * w));
        const int oy = (p / w) / 2, ox = (p % w + pad) / 2;
        if (!INV) bn_eval_affine4(gamma, beta, mean, var, ch, sc, sh);
        const f32x4 yb = bn_apply(((const f32x4*)z)[i], sc, sh);
        f32x4 out = {0.f, 0.f, 0.f, 0.f};
        if (ox < wo && (yb[0] > 0.f || yb[1] > 0.f || yb[2] > 0.f || yb[3] > 0.f)) {
            const int64_t o = (s * (ho * wo) + oy * wo + ox) * c + ch;
            const i32x4 ag = *(const i32x4*)(arg + o);
            const f32x4 d = *(const f32x4*)(dy + o);
#pragma unroll
            for (int e = 0; e < 4; ++e) out[e] = (ag[e] == p && yb[e] > 0.f) ? sc[e] * d[e] : 0.f;
        }
        ((f32x4*)dz)[i] = out;
    }
}

// the three pooled layers of the StandardCNN get their own instantiation, anything else the generic one
#define NQ_EVAL_MAXPOOL2_DISPATCH(KERNEL, GRID, ST, ...)                                                          \
    do {                                                                                                          \
        if (h == 48 && w == 15 && c == 16 && pad_w == 1) hipLaunchKernelGGL((KERNEL<48, 15, 16, 1>), GRID, dim3(256), 0, ST, __VA_ARGS__);     \
        else if (h == 24 && w == 8 && c == 32 && pad_w == 0) hipLaunchKernelGGL((KERNEL<24, 8, 32, 0>), GRID, dim3(256), 0, ST, __VA_ARGS__); \
        else if (h == 12 && w == 4 && c == 64 && pad_w == 0) hipLaunchKernelGGL((KERNEL<12, 4, 64, 0>), GRID, dim3(256), 0, ST, __VA_ARGS__); \
        else hipLaunchKernelGGL((KERNEL<0, 0, 0, 0>), GRID, dim3(256), 0, ST, __VA_ARGS__);                        \
    } while (0)

static bool maxpool2_shape_ok(int32_t n_segments, int32_t h, int32_t w, int32_t c, int32_t pad_w) {
    return n_segments > 0 && h > 0 && !(h & 1) && w > 0 && c > 0 && c <= 256 && !(c & 3) && (pad_w == 0 || pad_w == 1) &&
           w + 2 * pad_w >= 2;
}

extern "C" int nisqa_bn_eval_act_maxpool2_fwd(const float* z, const float* gamma, const float* beta, const float* running_mean,
                                              const float* running_var, int32_t n_segments, int32_t h, int32_t w, int32_t c,
                                              int32_t pad_w, float* y, int32_t* arg, void* stream) {
    if (!z || !gamma || !beta || !running_mean || !running_var || !y || !arg || !maxpool2_shape_ok(n_segments, h, w, c, pad_w))
        return NISQA_ERR_ARG;
    const int64_t total = (int64_t)n_segments * (h / 2) * ((w + 2 * pad_w - 2) / 2 + 1) * c / 4;
    NQ_LAUNCH_BEGIN();
    NQ_EVAL_MAXPOOL2_DISPATCH(bn_eval_act_maxpool2_fwd_kernel, dim3(grid_resident(total)), (hipStream_t)stream, z, gamma, beta,
                              running_mean, running_var, total, h, w, c, pad_w, y, arg);
    return NQ_LAUNCH_STATUS();
}

extern "C" int nisqa_bn_eval_act_maxpool2_bwd(const float* dy, const int32_t* arg, const float* z, const float* gamma,
                                              const float* beta, const float* running_mean, const float* running_var,
                                              int32_t n_segments, int32_t h, int32_t w, int32_t c, int32_t pad_w, float* dz,
                                              void* stream) {
    if (!dy || !arg || !z || !gamma || !beta || !running_mean || !running_var || !dz ||
        !maxpool2_shape_ok(n_segments, h, w, c, pad_w))
        return NISQA_ERR_ARG;
    const int64_t total = (int64_t)n_segments * h * w * c / 4;
    NQ_LAUNCH_BEGIN();
    NQ_EVAL_MAXPOOL2_DISPATCH(bn_eval_act_maxpool2_bwd_kernel, dim3(grid_resident(total)), (hipStream_t)stream, dy, arg, z, gamma,
                              beta, running_mean, running_var, total, h, w, c, pad_w, dz);
    return NQ_LAUNCH_STATUS();
}

// ---------------------------------------------------------------------------------------------------------
// conv1 on the segment tensor x [B][L][1][48][15]: valid segment s = seg_off[b] + k is row b * L + k of x
// ---------------------------------------------------------------------------------------------------------
// Forward, activations kept: z[s][m * 15 + j][co] = bias[co] + sum_tap w[co][tap] x[m + dy - 1][j + dx - 1] (tap = dy * 3 + dx, zero
// outside the 48 x 15 segment).  The arithmetic of conv1_fwd_kernel (csrc/train.hip) behind the loader of the segment-fed inference
// kernels: a row of x is copied into a zero-bordered LDS plane as it lies, [band][frame].
__global__ __launch_bounds__(256) void conv1_segments_fwd_kernel(const float* __restrict__ x, int l_max,
                                                                 const int32_t* __restrict__ seg_off, int n_clips,
                                                                 const float* __restrict__ w, const float* __restrict__ bias,
                                                                 float* __restrict__ z) {
    __shared__ float patch[50][17];                         // [band + 1][frame + 1]
    __shared__ float ws[16 * 9 + 16];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int b = find_segment(seg_off, n_clips, s);
    const int k = s - seg_off[b];
    const float* src = x + ((int64_t)b * l_max + k) * 720;
    for (int i = tid; i < 50 * 17; i += 256) {
        const int m = i / 17 - 1, j = i % 17 - 1;
        patch[0][i] = ((unsigned)m < 48u && (unsigned)j < 15u) ? src[m * 15 + j] : 0.f;
    }
    if (tid < 144) ws[tid] = w[tid];
    else if (tid < 160) ws[tid] = bias[tid - 144];
    __syncthreads();
    for (int p = tid; p < 720; p += 256) {
        const int m = p / 15, j = p % 15;
        float v[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) v[t] = patch[m + t / 3][j + t % 3];
        f32x4* dst = (f32x4*)(z + ((int64_t)s * 720 + p) * 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float acc = ws[144 + 4 * q + e];
#pragma unroll
                for (int t = 0; t < 9; ++t) acc = fmaf(v[t], ws[(4 * q + e) * 9 + t], acc);
                o[e] = acc;
            }
            dst[q] = o;
        }
    }
}

// Input gradient: one workgroup per ROW of the gradient tensor dx [B][L][1][48][15].  A valid row gathers, per pixel, the 9 x 16
// products dz[s][pixel - tap offset][co] * w[co][tap] in a fixed order (taps outer, channels inner); a padding row (l >= the
// clip's segment count) is written as zeros.  Every element of dx is written once: no clearing pass, no atomics.
__global__ __launch_bounds__(256) void conv1_segments_dgrad_kernel(const float* __restrict__ dz, const int32_t* __restrict__ seg_off,
                                                                   int l_max, const float* __restrict__ w, float* __restrict__ dx) {
    __shared__ float ws[9 * 16];                            // [tap][co]
    const int b = blockIdx.x / l_max, l = blockIdx.x - b * l_max, tid = threadIdx.x;
    float* dst = dx + (int64_t)blockIdx.x * 720;
    const int s0 = seg_off[b], n = seg_off[b + 1] - s0;
    if (l >= n) {
        for (int p = tid; p < 720; p += 256) dst[p] = 0.f;
        return;
    }
    if (tid < 144) ws[(tid % 9) * 16 + tid / 9] = w[tid];   // w is [co][tap]
    __syncthreads();
    const float* src = dz + (int64_t)(s0 + l) * (720 * 16);
    for (int p = tid; p < 720; p += 256) {
        const int m = p / 15, j = p % 15;
        float acc = 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int mm = m - (t / 3 - 1), jj = j - (t % 3 - 1);      // the output pixel that read x[m][j] through tap t
            if ((unsigned)mm < 48u && (unsigned)jj < 15u) {
                const f32x4* d = (const f32x4*)(src + (mm * 15 + jj) * 16);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 v = d[q];
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc = fmaf(v[e], ws[t * 16 + 4 * q + e], acc);
                }
            }
        }
        dst[p] = acc;
    }
}

extern "C" int nisqa_conv1_segments_fwd(const float* x, int32_t l_max, const int32_t* seg_off, int32_t n_clips, int32_t n_segments,
                                        const float* w, const float* bias, float* z, void* stream) {
    if (!x || !seg_off || !w || !bias || !z || l_max <= 0 || n_clips <= 0 || n_segments <= 0) return NISQA_ERR_ARG;
    NQ_LAUNCH_BEGIN();
    hipLaunchKernelGGL(conv1_segments_fwd_kernel, dim3(n_segments), dim3(256), 0, (hipStream_t)stream, x, l_max, seg_off, n_clips, w,
                       bias, z);
    return NQ_LAUNCH_STATUS();
}

extern "C" int nisqa_conv1_segments_dgrad(const float* dz, const int32_t* seg_off, int32_t n_clips, int32_t l_max, const float* w,
                                          float* dx, void* stream) {
    if (!dz || !seg_off || !w || !dx || n_clips <= 0 || l_max <= 0 || (int64_t)n_clips * l_max > 0x7fffffffLL) return NISQA_ERR_ARG;
    NQ_LAUNCH_BEGIN();
    hipLaunchKernelGGL(conv1_segments_dgrad_kernel, dim3((unsigned)(n_clips * l_max)), dim3(256), 0, (hipStream_t)stream, dz, seg_off,
                       l_max, w, dx);
    return NQ_LAUNCH_STATUS();
}
