// Per-segment profile of a pooled score (nisqa_pool_profile, include/nisqa_hip.h): what the reference's users read off a hook on
// model.pool -- PoolAttFF.forward (nisqa/NISQA_lib.py:1171-1183) and PoolAvg.forward (:1196-1205) -- taken apart per token.
//
//   PoolAttFF:  score = linear3(sum_t a_t x_t) with sum_t a_t = 1, hence score = sum_t a_t (w3 . x_t + b3): the attention weight
//               a_t = softmax_t(w2 . relu(W1 x_t + b1) + b2) over the clip's valid tokens and the local score s_t = w3 . x_t + b3.
//   PoolAvg:    score = linear(mean_t h_t) = sum_t (1 / n) (w . h_t + b).
//
// ONE launch, one workgroup of 256 threads per (clip, head).  A thread owns one token at a time (token t = 256 i + thread): it holds
// the token's 64 features in registers and runs every dot product as ONE k-ordered fp32 fmaf chain that starts from the bias -- the
// hidden layer unit by unit (the weights are wave-uniform: they come through the scalar cache), the logit over the 128 hidden units
// in ascending order.  Plain VALU in every engine precision form: 64 x 128 MACs per token and head is nothing next to the CNN, and
// the result does not depend on how the x it reads was produced.  The logits wait in weights_out; after a barrier the workgroup
// takes the clip's maximum and the sum of the exponentials -- per thread in ascending token order, then a fixed binary tree over
// the 256 partial results in LDS -- and normalises in place.  No atomics, no order left to the scheduler: two calls give the same
// bits.  Rows behind n_wins (up to the next clip's first row; for the last clip up to total_tok_padded) are written as zeros and
// never read.
#include "common.hpp"
#include "../../include/nisqa_hip.h"

namespace {

constexpr int PP_D = 64;                                // PoolAttFF input width (d_model)
constexpr int PP_H = 128;                               // PoolAttFF hidden width (pool_att_h)
constexpr int PP_LSTM_D = 256;                          // PoolAvg input width (BiLSTM output)
constexpr int PP_THREADS = 256;
// blob of one PoolAttFF head, natural order (nisqa_amd.weights.pack_pool_profile): W1 [128][64], b1 [128], w2 [128], b2, w3 [64], b3
constexpr int PP_W1 = 0;
constexpr int PP_B1 = PP_W1 + PP_H * PP_D;
constexpr int PP_W2 = PP_B1 + PP_H;
constexpr int PP_B2 = PP_W2 + PP_H;
constexpr int PP_W3 = PP_B2 + 1;
constexpr int PP_B3 = PP_W3 + PP_D;
constexpr int PP_FLOATS = PP_B3 + 1;
// blob of PoolAvg (pack_pool_profile_avg): w [256], b

// the workgroup's maximum / sum of v through LDS: a fixed binary tree, every thread gets the result
template <bool MAX>
__device__ __forceinline__ float block_reduce(float v, float* red, int t) {
    __syncthreads();                                    // red may still be read from the previous reduction
    red[t] = v;
    __syncthreads();
    for (int s = PP_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) red[t] = MAX ? fmaxf(red[t], red[t + s]) : red[t] + red[t + s];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(PP_THREADS) void pool_profile_kernel(const float* __restrict__ x,
                                                                  const int32_t* __restrict__ tok_off,
                                                                  const int32_t* __restrict__ n_wins, int n_clips, int total_tok,
                                                                  int n_heads, int mode, const float* __restrict__ w,
                                                                  float* __restrict__ weights_out, float* __restrict__ local_out) {
    __shared__ float red[PP_THREADS];
    const int c = blockIdx.x, h = blockIdx.y, t = threadIdx.x;
    const int row0 = tok_off[c];
    // the rows this workgroup writes end where the next clip's begin; the last clip takes what is left of the buffers
    const int row1 = min(c + 1 < n_clips ? tok_off[c + 1] : total_tok, total_tok);
    if (row0 < 0 || row0 >= row1) return;
    const int n = max(0, min(n_wins[c], row1 - row0));  // valid tokens; never more than the rows the clip owns
    float* __restrict__ wo = weights_out + (size_t)row0 * n_heads + h;
    float* __restrict__ lo = local_out + (size_t)row0 * n_heads + h;

    for (int i = n + t; i < row1 - row0; i += PP_THREADS) {       // padding rows: zeros, x is not read
        wo[(size_t)i * n_heads] = 0.f;
        lo[(size_t)i * n_heads] = 0.f;
    }
    if (n == 0) return;

    if (mode == 1) {                                    // PoolAvg: local = w . h_t + b, weights = 1 / n
        const float inv = 1.0f / (float)n;
        for (int i = t; i < n; i += PP_THREADS) {
            const float* __restrict__ xr = x + (size_t)(row0 + i) * PP_LSTM_D;
            float acc = w[PP_LSTM_D];
            for (int k = 0; k < PP_LSTM_D; k += 4) {
                const f32x4 v = *(const f32x4*)(xr + k);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = fmaf(w[k + e], v[e], acc);
            }
            lo[(size_t)i * n_heads] = acc;
            wo[(size_t)i * n_heads] = inv;
        }
        return;
    }

    const float* __restrict__ wh = w + (size_t)h * PP_FLOATS;
    float tmax = -INFINITY;
    for (int i = t; i < n; i += PP_THREADS) {
        const float* __restrict__ xr = x + (size_t)(row0 + i) * PP_D;
        float xv[PP_D];
#pragma unroll
        for (int k = 0; k < PP_D; k += 4) {
            const f32x4 v = *(const f32x4*)(xr + k);
#pragma unroll
            for (int e = 0; e < 4; ++e) xv[k + e] = v[e];
        }
        float local = wh[PP_B3];
#pragma unroll
        for (int k = 0; k < PP_D; ++k) local = fmaf(wh[PP_W3 + k], xv[k], local);
        float logit = wh[PP_B2];
#pragma unroll 1
        for (int j = 0; j < PP_H; ++j) {
            float a = wh[PP_B1 + j];
#pragma unroll
            for (int k = 0; k < PP_D; ++k) a = fmaf(wh[PP_W1 + j * PP_D + k], xv[k], a);
            logit = fmaf(wh[PP_W2 + j], fmaxf(a, 0.f), logit);
        }
        lo[(size_t)i * n_heads] = local;
        wo[(size_t)i * n_heads] = logit;              // read back below by the thread that wrote it
        tmax = fmaxf(tmax, logit);
    }
    const float m = block_reduce<true>(tmax, red, t);
    float tsum = 0.f;
    for (int i = t; i < n; i += PP_THREADS) {
        const float e = expf(wo[(size_t)i * n_heads] - m);
        wo[(size_t)i * n_heads] = e;
        tsum += e;
    }
    const float sum = block_reduce<false>(tsum, red, t);
    for (int i = t; i < n; i += PP_THREADS) wo[(size_t)i * n_heads] = wo[(size_t)i * n_heads] / sum;
}

}  // namespace

extern "C" int nisqa_pool_profile(const float* x, int32_t ld, const int32_t* tok_off, const int32_t* n_wins, int32_t n_clips,
                                  int32_t total_tok_padded, int32_t n_heads, int32_t mode, const float* w, float* weights_out,
                                  float* local_out, void* stream) {
    if (!x || !tok_off || !n_wins || !w || !weights_out || !local_out || n_clips <= 0 || total_tok_padded <= 0 || n_heads < 1 ||
        n_heads > 5 || mode < 0 || mode > 1 || ld != (mode == 0 ? PP_D : PP_LSTM_D) || (mode == 1 && n_heads != 1))
        return NISQA_ERR_ARG;
    NQ_LAUNCH_BEGIN();
    hipLaunchKernelGGL(pool_profile_kernel, dim3(n_clips, n_heads), dim3(PP_THREADS), 0, (hipStream_t)stream, x, tok_off, n_wins,
                       n_clips, total_tok_padded, n_heads, mode, w, weights_out, local_out);
    return NQ_LAUNCH_STATUS();
}
