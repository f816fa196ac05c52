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
constexpr int PP_GATES = 8;                             // backward: first word of a parked dx row that holds ReLU gates (logits: 0 .. 4)
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

// one row of PP_D floats into registers
__device__ __forceinline__ void load_row(const float* __restrict__ xr, float (&xv)[PP_D]) {
#pragma unroll
    for (int k = 0; k < PP_D; k += 4) {
        const f32x4 v = *(const f32x4*)(xr + k);
#pragma unroll
        for (int e = 0; e < 4; ++e) xv[k + e] = v[e];
    }
}

// logit = w2 . relu(W1 x + b1) + b2 of one PoolAttFF head: every hidden unit one k-ordered fmaf chain from its bias, the logit one
// chain over the 128 units in ascending order from b2.  The forward and the backward both get their logits here.  GATES: the ReLU
// gates [u_j > 0] go out as PP_H / 32 words, unit j in bit j % 32 of word j / 32.
template <bool GATES>
__device__ __forceinline__ float logit_of(const float* __restrict__ wh, const float (&xv)[PP_D], uint32_t* gates = nullptr) {
    float logit = wh[PP_B2];
#pragma unroll 1
    for (int q = 0; q < PP_H / 32; ++q) {
        uint32_t word = 0;
#pragma unroll 1
        for (int j = 32 * q; j < 32 * q + 32; ++j) {
            float a = wh[PP_B1 + j];
#pragma unroll
            for (int k = 0; k < PP_D; ++k) a = fmaf(wh[PP_W1 + j * PP_D + k], xv[k], a);
            logit = fmaf(wh[PP_W2 + j], fmaxf(a, 0.f), logit);
            if (GATES) word |= (uint32_t)(a > 0.f) << (j & 31);
        }
        if (GATES) gates[q] = word;
    }
    return logit;
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
        load_row(xr, xv);
        float local = wh[PP_B3];
#pragma unroll
        for (int k = 0; k < PP_D; ++k) local = fmaf(wh[PP_W3 + k], xv[k], local);
        const float logit = logit_of<false>(wh, xv);
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

// The backward of the PoolAttFF profile in x (nisqa_pool_profile_bwd): d / d x_t of sum (da . weights + ds . local + de . x) for
// cotangents da, ds [tok][heads] and de [tok][64], each of which may be absent (zero).
//   dz_t = a_t (da_t - r),  r = sum_u a_u da_u;   du_t = dz_t w2 * [u_t > 0];   dx_t = de_t + sum_heads (W1^T du_t + ds_t w3)
// ONE launch, one workgroup of 256 threads per CLIP, which walks the heads in order: the head sum is a thread's own register
// accumulation, never a race.  A thread owns token t = 256 i + thread in every pass.  Nothing of the forward is taken over: pass 1
// recomputes every head's logit with the forward's chains (load_row / logit_of are the forward's) and parks it, with the hidden
// layer's 128 ReLU gates as four words, in the token's own, still unwritten dx row (logits: columns 0 .. heads - 1, gates: from
// PP_GATES on); per head the workgroup takes the maximum, the sum of the exponentials and r the way the forward reduces -- per
// thread in ascending token order, then the fixed LDS tree; pass 2 reads the parked logits and gates back, accumulates the 64 dx
// components in registers -- W1^T du unit by unit in ascending order -- and writes the row once.  x is read in pass 1 only.
// Without da there is no softmax to differentiate and only the last pass runs.  Padding rows: zeros, x and cotangents not read.
__global__ __launch_bounds__(PP_THREADS) void pool_profile_bwd_kernel(const float* __restrict__ x,
                                                                      const int32_t* __restrict__ tok_off,
                                                                      const int32_t* __restrict__ n_wins, int n_clips, int total_tok,
                                                                      int n_heads, const float* __restrict__ w,
                                                                      const float* __restrict__ da, const float* __restrict__ ds,
                                                                      const float* __restrict__ de, float* dx) {
    __shared__ float red[PP_THREADS];
    __shared__ float stat[5][3];                        // per head: the clip's maximum logit, the sum of the exponentials, r
    const int c = blockIdx.x, t = threadIdx.x;
    const int row0 = tok_off[c];
    const int row1 = min(c + 1 < n_clips ? tok_off[c + 1] : total_tok, total_tok);
    if (row0 < 0 || row0 >= row1) return;
    const int n = max(0, min(n_wins[c], row1 - row0));

    for (int i = n + t; i < row1 - row0; i += PP_THREADS) {       // padding rows: zeros, nothing is read
        f32x4* __restrict__ o = (f32x4*)(dx + (size_t)(row0 + i) * PP_D);
#pragma unroll
        for (int k = 0; k < PP_D / 4; ++k) o[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (n == 0) return;

    if (da) {
        for (int i = t; i < n; i += PP_THREADS) {                 // pass 1: the logits of every head, parked in the token's dx row
            float xv[PP_D];
            load_row(x + (size_t)(row0 + i) * PP_D, xv);
            float* park = dx + (size_t)(row0 + i) * PP_D;
            for (int h = 0; h < n_heads; ++h)
                park[h] = logit_of<true>(w + (size_t)h * PP_FLOATS, xv, (uint32_t*)park + PP_GATES + h * (PP_H / 32));
        }
        for (int h = 0; h < n_heads; ++h) {                       // read back by the thread that wrote them
            const float* z = dx + (size_t)row0 * PP_D + h;
            const float* __restrict__ dah = da + (size_t)row0 * n_heads + h;
            float tmax = -INFINITY;
            for (int i = t; i < n; i += PP_THREADS) tmax = fmaxf(tmax, z[(size_t)i * PP_D]);
            const float m = block_reduce<true>(tmax, red, t);
            float tsum = 0.f;
            for (int i = t; i < n; i += PP_THREADS) tsum += expf(z[(size_t)i * PP_D] - m);
            const float sum = block_reduce<false>(tsum, red, t);
            float tr = 0.f;
            for (int i = t; i < n; i += PP_THREADS) tr = fmaf(expf(z[(size_t)i * PP_D] - m) / sum, dah[(size_t)i * n_heads], tr);
            const float r = block_reduce<false>(tr, red, t);
            if (t == 0) {
                stat[h][0] = m;
                stat[h][1] = sum;
                stat[h][2] = r;
            }
        }
        __syncthreads();
    }

    for (int i = t; i < n; i += PP_THREADS) {                     // pass 2: the token's dx row
        const size_t row = (size_t)(row0 + i);
        float acc[PP_D];
        if (de) {
            load_row(de + row * PP_D, acc);
        } else {
#pragma unroll
            for (int k = 0; k < PP_D; ++k) acc[k] = 0.f;
        }
        for (int h = 0; h < n_heads; ++h) {
            const float* __restrict__ wh = w + (size_t)h * PP_FLOATS;
            if (ds) {
                const float dsv = ds[row * n_heads + h];
#pragma unroll
                for (int k = 0; k < PP_D; ++k) acc[k] = fmaf(dsv, wh[PP_W3 + k], acc[k]);
            }
            if (!da) continue;
            const float a = expf(dx[row * PP_D + h] - stat[h][0]) / stat[h][1];      // the forward's weight, bit for bit
            const float dz = a * (da[row * n_heads + h] - stat[h][2]);
            const uint32_t* gates = (const uint32_t*)(dx + row * PP_D) + PP_GATES + h * (PP_H / 32);
#pragma unroll 1
            for (int q = 0; q < PP_H / 32; ++q) {
                const uint32_t word = gates[q];
#pragma unroll 1
                for (int j = 32 * q; j < 32 * q + 32; ++j) {
                    const float du = (word >> (j & 31)) & 1u ? dz * wh[PP_W2 + j] : 0.f;
#pragma unroll
                    for (int k = 0; k < PP_D; ++k) acc[k] = fmaf(du, wh[PP_W1 + j * PP_D + k], acc[k]);
                }
            }
        }
        f32x4* o = (f32x4*)(dx + row * PP_D);
#pragma unroll
        for (int k = 0; k < PP_D; k += 4) o[k / 4] = f32x4{acc[k], acc[k + 1], acc[k + 2], acc[k + 3]};
    }
}

}  // namespace

extern "C" int nisqa_pool_profile_bwd(const float* x, int32_t ld, const int32_t* tok_off, const int32_t* n_wins, int32_t n_clips,
                                      int32_t total_tok_padded, int32_t n_heads, int32_t mode, const float* w, const float* d_weights,
                                      const float* d_local, const float* d_embed, float* dx, void* stream) {
    if (!x || !tok_off || !n_wins || !w || !dx || n_clips <= 0 || total_tok_padded <= 0 || n_heads < 1 || n_heads > 5 || mode != 0 ||
        ld != PP_D)
        return NISQA_ERR_ARG;
    NQ_LAUNCH_BEGIN();
    hipLaunchKernelGGL(pool_profile_bwd_kernel, dim3(n_clips), dim3(PP_THREADS), 0, (hipStream_t)stream, x, tok_off, n_wins, n_clips,
                       total_tok_padded, n_heads, w, d_weights, d_local, d_embed, dx);
    return NQ_LAUNCH_STATUS();
}

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
