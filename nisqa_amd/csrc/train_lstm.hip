// BiLSTM of the StandardCNN + BiLSTM models in training (include/nisqa_train.h): the train-mode forward of
// nn.LSTM over each clip's n_wins segments (reference nisqa/NISQA_lib.py:897-943, packed sequence) with PoolAvg / PoolMax /
// PoolLastStepBi's reduction (NL:1099-1115, 1185-1224), and its backward through time.
//
// Both kernels keep lstm.hip's shape: ONE launch for all clips and both directions, one 512-thread workgroup per (clip,
// direction), one LDS exchange and one barrier per step.  The inference kernels (lstm_dir_kernel and its pooled siblings)
// are not touched; the forward here is their step plus the stores of what the backward needs.
//
// Saved state per valid token and direction (save[tokens][2][640]): the activated gates i, f, g, o (PyTorch order) and the
// cell state c after the step; hprev[tokens][2][128] = the hidden state the step READ (h_{t-1}, zero at the direction's
// first step), which is the right operand of dW_hh = dgates^T h_prev.  Steps are counted in each direction's own order:
// direction 0 walks tokens seg_off[b] .. seg_off[b+1]-1, direction 1 the same tokens backwards.
//
// BPTT: thread (u, q) owns column u of W_hh restricted to gate q's 128 rows (W_hh[q*128 + j][u], j < 128, in registers).
// Per step, walking the direction's steps in reverse, lane q of the quad of unit u forms d pre-activation of gate q from
// dh = dh_rec + dh_out (dh_out from the pooling: w / n at every step for avg, one-hot at the arg-max step for max, the
// direction's last step for last_step_bi -- no [T][256] tensor is ever written), the carried dc and the saved gates; it
// publishes it in a double-buffered LDS vector and writes it to dgates[tokens][2][512]; after the barrier every lane
// reads the 128 published values of its gate and the quad sum of the four partial products is dh_rec = W_hh^T dgates for
// the next (earlier) step.  The bias gradient (sum of dgates over steps) is accumulated in float64 beside the recurrence.
#include <math.h>
#include "common.hpp"
#include "../../include/nisqa_hip.h"
#include "../../include/nisqa_train.h"

#define LT_H 128
#define LT_G 512                      /* 4 gates x 128 */
#define LT_SAVE 640                   /* i, f, g, o, c */

NQ_DEV float lt_quad_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
    return v;
}

template <int N>
NQ_DEV float lt_quad_bcast(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), N * 0x55, 0xF, 0xF, true));
}

NQ_DEV float lt_tanh(float x) { return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(2.0f * x)); }

// ---- forward -------------------------------------------------------------------------------------------------------
// thread (u, q): the four gate rows of unit u over h[32 q .. 32 q + 31] and x[5 q .. 5 q + 4], as in lstm_dir_kernel
__global__ __launch_bounds__(512, 1) void lstm_train_fwd_kernel(
    const float* __restrict__ x20, const int32_t* __restrict__ seg_off, const float* __restrict__ w_ih,
    const float* __restrict__ w_hh, const float* __restrict__ b_ih, const float* __restrict__ b_hh, int pool_mode,
    float* __restrict__ save, float* __restrict__ hprev, float* __restrict__ pooled, int32_t* __restrict__ argmax) {
    __shared__ __attribute__((aligned(16))) float hbuf[2][LT_H];
    const int i = threadIdx.x, b = blockIdx.x, dir = blockIdx.y;
    const int lane = i & 63, wave = __builtin_amdgcn_readfirstlane(i >> 6);
    const int u = 16 * wave + (lane >> 2), q = lane & 3;
    const int c0 = seg_off[b], n = seg_off[b + 1] - c0;
    const float* whh_d = w_hh + (size_t)dir * LT_G * LT_H;
    const float* wih_d = w_ih + (size_t)dir * LT_G * 20;
    float whh[4][32], wih[4][5], bias[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int row = g * LT_H + u;
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
            const f32x4 v = *(const f32x4*)(whh_d + (size_t)row * LT_H + 32 * q + 4 * kk);
#pragma unroll
            for (int e = 0; e < 4; ++e) whh[g][4 * kk + e] = v[e];
        }
#pragma unroll
        for (int j = 0; j < 5; ++j) wih[g][j] = wih_d[row * 20 + 5 * q + j];
        bias[g] = q == 0 ? b_ih[dir * LT_G + row] + b_hh[dir * LT_G + row] : 0.f;
    }
    const float gk = q == 2 ? 2.0f : 1.0f, gb = q == 2 ? -1.0f : 0.0f;
    float c = 0.f, h = 0.f;
    double hsum = 0.0;                                  // avg: float64 sum of the states, as lstm_dir_avg_kernel
    float hmax = -__builtin_inff();
    int targ = 0;
    if (i < 2 * LT_H) ((float*)hbuf)[i] = 0.f;
    __syncthreads();
    auto xload = [&](int t, float (&xv)[5]) {
        const int tok = c0 + (dir == 0 ? t : n - 1 - t);
        const float* x = x20 + (size_t)tok * 20 + 5 * q;
#pragma unroll
        for (int j = 0; j < 5; ++j) xv[j] = x[j];
    };
    float xv[5];
    if (n > 0) xload(0, xv);
    for (int t = 0; t < n; ++t) {
        const int tok = c0 + (dir == 0 ? t : n - 1 - t);
        const f32x4* hp = (const f32x4*)(hbuf[t & 1] + 32 * q);
        f32x4 hv[8];
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) hv[kk] = hp[kk];
        float a[4][2];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            a[g][0] = bias[g];
            a[g][1] = 0.f;
#pragma unroll
            for (int j = 0; j < 5; ++j) a[g][j & 1] = fmaf(wih[g][j], xv[j], a[g][j & 1]);
        }
        if (t + 1 < n) xload(t + 1, xv);
#pragma unroll
        for (int kk = 0; kk < 8; ++kk)
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int e = 0; e < 4; ++e) a[g][e & 1] = fmaf(whh[g][4 * kk + e], hv[kk][e], a[g][e & 1]);
        const float p0 = lt_quad_sum(a[0][0] + a[0][1]), p1 = lt_quad_sum(a[1][0] + a[1][1]);
        const float p2 = lt_quad_sum(a[2][0] + a[2][1]), p3 = lt_quad_sum(a[3][0] + a[3][1]);
        const float pre = q == 0 ? p0 : q == 1 ? p1 : q == 2 ? p2 : p3;
        const float act = fmaf(gk, __builtin_amdgcn_rcpf(1.0f + __expf(-gk * pre)), gb);
        const float ig = lt_quad_bcast<0>(act), fg = lt_quad_bcast<1>(act), gg = lt_quad_bcast<2>(act), og = lt_quad_bcast<3>(act);
        float* sv = save + ((size_t)tok * 2 + dir) * LT_SAVE;
        sv[q * LT_H + u] = act;                         // lane q: gate q
        if (q == 1) hprev[((size_t)tok * 2 + dir) * LT_H + u] = h;
        c = fmaf(fg, c, ig * gg);
        h = og * lt_tanh(c);
        if (q == 0) {
            sv[4 * LT_H + u] = c;
            hbuf[(t + 1) & 1][u] = h;
        }
        if (pool_mode == NISQA_LSTM_POOL_AVG) hsum += (double)h;
        else if (pool_mode == NISQA_LSTM_POOL_MAX && h > hmax) { hmax = h; targ = t; }
        __syncthreads();
    }
    if (q == 0) {
        const size_t o = (size_t)b * 2 * LT_H + dir * LT_H + u;
        if (pool_mode == NISQA_LSTM_POOL_AVG) pooled[o] = (float)(hsum / (double)n);
        else if (pool_mode == NISQA_LSTM_POOL_MAX) { pooled[o] = hmax; argmax[o] = targ; }
        else pooled[o] = h;                             // direction 0: its last step; direction 1: position 0
    }
}

// ---- backward through time -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(512, 1) void lstm_train_bptt_kernel(
    const int32_t* __restrict__ seg_off, const float* __restrict__ w_hh, const float* __restrict__ save, int pool_mode,
    const float* __restrict__ dpooled, const int32_t* __restrict__ argmax, float* __restrict__ dgates,
    double* __restrict__ dbias) {
    __shared__ __attribute__((aligned(16))) float dbuf[2][LT_G];
    const int i = threadIdx.x, b = blockIdx.x, dir = blockIdx.y;
    const int lane = i & 63, wave = __builtin_amdgcn_readfirstlane(i >> 6);
    const int u = 16 * wave + (lane >> 2), q = lane & 3;
    const int c0 = seg_off[b], n = seg_off[b + 1] - c0;
    const float* whh_d = w_hh + (size_t)dir * LT_G * LT_H;
    float wt[LT_H];                                     // W_hh[q * 128 + j][u]
#pragma unroll
    for (int j = 0; j < LT_H; ++j) wt[j] = whh_d[(size_t)(q * LT_H + j) * LT_H + u];
    const size_t po = (size_t)b * 2 * LT_H + dir * LT_H + u;
    const float dp = dpooled[po];
    const int tsel = pool_mode == NISQA_LSTM_POOL_MAX ? argmax[po] : n - 1;
    const float dh_avg = pool_mode == NISQA_LSTM_POOL_AVG ? (float)((double)dp / (double)n) : 0.f;
    // saved values of a step: i, f, g, o, c and the c of the step before (0 at the direction's first step)
    auto sload = [&](int t, float (&v)[6]) {
        const int tok = c0 + (dir == 0 ? t : n - 1 - t);
        const float* sv = save + ((size_t)tok * 2 + dir) * LT_SAVE;
#pragma unroll
        for (int g = 0; g < 5; ++g) v[g] = sv[g * LT_H + u];
        v[5] = t > 0 ? save[((size_t)(dir == 0 ? tok - 1 : tok + 1) * 2 + dir) * LT_SAVE + 4 * LT_H + u] : 0.f;
    };
    float sv[6];
    if (n > 0) sload(n - 1, sv);
    float dh_rec = 0.f, dc = 0.f;
    double db = 0.0;
    for (int t = n - 1; t >= 0; --t) {
        const int tok = c0 + (dir == 0 ? t : n - 1 - t);
        const float ig = sv[0], fg = sv[1], gg = sv[2], og = sv[3], cc = sv[4], cp = sv[5];
        if (t > 0) sload(t - 1, sv);                    // in flight across the step
        const float dh = dh_rec + (pool_mode == NISQA_LSTM_POOL_AVG ? dh_avg : (t == tsel ? dp : 0.f));
        const float tc = tanhf(cc);
        dc = fmaf(dh * og, 1.0f - tc * tc, dc);
        const float d_i = dc * gg * ig * (1.0f - ig);
        const float d_f = dc * cp * fg * (1.0f - fg);
        const float d_g = dc * ig * (1.0f - gg * gg);
        const float d_o = dh * tc * og * (1.0f - og);
        const float dg = q == 0 ? d_i : q == 1 ? d_f : q == 2 ? d_g : d_o;
        dc *= fg;                                       // carried to the step before
        dbuf[t & 1][q * LT_H + u] = dg;
        dgates[((size_t)tok * 2 + dir) * LT_G + q * LT_H + u] = dg;
        db += (double)dg;
        __syncthreads();
        const f32x4* dv = (const f32x4*)(dbuf[t & 1] + q * LT_H);
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < LT_H / 4; ++kk) {
            const f32x4 v = dv[kk];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = fmaf(wt[4 * kk + e], v[e], acc[e]);
        }
        dh_rec = lt_quad_sum((acc[0] + acc[1]) + (acc[2] + acc[3]));
    }
    if (dbias) atomicAdd(dbias + dir * LT_G + q * LT_H + u, db);
}

extern "C" int nisqa_lstm_train_fwd(const float* x20, const int32_t* seg_off, int32_t n_clips, const float* w_ih,
                                    const float* w_hh, const float* b_ih, const float* b_hh, int32_t pool_mode, float* save,
                                    float* hprev, float* pooled, int32_t* argmax, void* stream) {
    if (!x20 || !seg_off || !w_ih || !w_hh || !b_ih || !b_hh || !save || !hprev || !pooled || n_clips <= 0)
        return NISQA_ERR_ARG;
    if (pool_mode != NISQA_LSTM_POOL_LAST_STEP_BI && pool_mode != NISQA_LSTM_POOL_AVG && pool_mode != NISQA_LSTM_POOL_MAX)
        return NISQA_ERR_ARG;
    if (pool_mode == NISQA_LSTM_POOL_MAX && !argmax) return NISQA_ERR_ARG;
    NQ_LAUNCH_BEGIN();
    hipLaunchKernelGGL(lstm_train_fwd_kernel, dim3(n_clips, 2), dim3(512), 0, (hipStream_t)stream, x20, seg_off, w_ih, w_hh, b_ih,
                       b_hh, (int)pool_mode, save, hprev, pooled, argmax);
    return NQ_LAUNCH_STATUS();
}

extern "C" int nisqa_lstm_train_bptt(const int32_t* seg_off, int32_t n_clips, const float* w_hh, const float* save,
                                     int32_t pool_mode, const float* dpooled, const int32_t* argmax, float* dgates,
                                     double* dbias, void* stream) {
    if (!seg_off || !w_hh || !save || !dpooled || !dgates || n_clips <= 0) return NISQA_ERR_ARG;
    if (pool_mode != NISQA_LSTM_POOL_LAST_STEP_BI && pool_mode != NISQA_LSTM_POOL_AVG && pool_mode != NISQA_LSTM_POOL_MAX)
        return NISQA_ERR_ARG;
    if (pool_mode == NISQA_LSTM_POOL_MAX && !argmax) return NISQA_ERR_ARG;
    NQ_LAUNCH_BEGIN();
    hipLaunchKernelGGL(lstm_train_bptt_kernel, dim3(n_clips, 2), dim3(512), 0, (hipStream_t)stream, seg_off, w_hh, save,
                       (int)pool_mode, dpooled, argmax, dgates, dbias);
    return NQ_LAUNCH_STATUS();
}
