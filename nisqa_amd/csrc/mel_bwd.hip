// Backward of the mel front end (csrc/mel.hip) and the adjoint of the segmenting: what carries d L / d x of model(x, n_wins) back
// to the audio samples.  Host side: engine.HipNisqa.grad_audio; DESIGN.md 4.6.3.
//
// The function differentiated is the forward's, per clip of L samples (cfg: the forward's nisqa_mel_cfg):
//   frame f, tap n < win    x_n = w_n y[refl(f hop + start0 + n)], start0 = -n_fft / 2 + (n_fft - win) / 2, refl: i -> -i below 0 and
//                           i -> 2 (L - 1) - i from L on (load_frame of mel.hip); zero-padded to 4096
//   X_k = sum_n x_n e^(-2 pi i k n / 4096), k = 0 .. 2048   (the taps sit at n = 0 .. win - 1 here and centred in the frame in
//                           librosa: a circular shift, which changes neither |X_k| nor the derivative below)
//   M_m = sum_k fb[m][k] |X_k|,  db = 10 log10(max(amin_sq, M_m^2)),  out = max(db, max_clip(db) - top_db)
// and its derivative, walked back by four launches without an atomic (every output element is written once, by one thread, in a
// fixed order of additions: two calls give the same bits):
//   nisqa_mel_db_bwd_gate      d L / d M from d L / d out, the forward's unclamped dB rows and clip_floor
//   nisqa_mel_frame_bwd        per frame: X recomputed, d L / d |X_k| = sum_m fb[m][k] d L / d M_m, then
//                              d L / d x_n = w_n Re sum_{k <= 2048} (d L / d |X_k| X_k / |X_k|) e^(+2 pi i k n / 4096) -> ws [TT][win]
//   nisqa_mel_overlap_add_bwd  per sample: the frames over each padded position that reflects onto it, gathered from ws
//   nisqa_segments_to_mel_bwd  d L / d out [TT][48] from d L / d x [B][L][1][48][15]
// and, for the way there, nisqa_mel_segments_fwd: the clamped segment tensor x [B][L][1][48][15] from the unclamped dB rows.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.hpp"
#include "../../include/nisqa_hip.h"
#include "../../include/nisqa_train.h"

#define MB_N 4096                 // NISQA_N_FFT
#define MB_BINS 2049
#define MB_GATE_THREADS 1024

typedef float2 cf;
NQ_DEV cf mb_cmul(cf a, cf b) { return cf{fmaf(a.x, b.x, -(a.y * b.y)), fmaf(a.x, b.y, a.y * b.x)}; }

// the sample a padded position of the clip reads: np.pad(mode='reflect') as load_frame of mel.hip applies it
NQ_DEV int mb_reflect(int i, int L) {
    i = i < 0 ? -i : i;
    i = i >= L ? 2 * (L - 1) - i : i;
    return min(max(i, 0), L - 1);
}
NQ_DEV int mb_start0(int win) { return -MB_N / 2 + (MB_N - win) / 2; }      // first windowed sample of frame 0

// ---------------------------------------------------------------------------------------------------------
// d L / d out -> d L / d M: the top_db clamp and the dB conversion
// ---------------------------------------------------------------------------------------------------------
// One workgroup per clip.  out = max(db, floor), floor = max(db) - top_db: an element above the floor passes its g, an element at
// or below it hands its g to the floor and so to the clip's maximum -- the FIRST one in (frame, band) order where several are
// equal, as torch.max picks one.  Both sides of the floor are decided on the forward's own bits (its unclamped dB rows and its
// clip_floor), and so is the side of amin: an element whose dB is the forward's 10 log10f(amin_sq) sat under amin (its power was
// replaced by a constant: derivative 0).  M is recovered from the stored dB: 1 / M = 10^(-db / 20), fp32-exact to 5e-7.
// The sums run in a fixed order: a thread adds its elements in ascending order, the threads are combined by a tree.
__global__ __launch_bounds__(MB_GATE_THREADS) void mel_db_bwd_gate_kernel(
    const float* __restrict__ g, const float* __restrict__ db, const float* __restrict__ clip_floor,
    const int32_t* __restrict__ frame_off, float amin_sq, float* __restrict__ dm) {
    __shared__ float s_sum[MB_GATE_THREADS];
    __shared__ float s_max[MB_GATE_THREADS];
    __shared__ int s_arg[MB_GATE_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t e0 = (int64_t)frame_off[b] * NISQA_N_MELS;
    const int n = (frame_off[b + 1] - frame_off[b]) * NISQA_N_MELS;
    const float fl = clip_floor[b];
    float sum = 0.f, mx = -3.0e38f;
    int arg = 0x7fffffff;
    for (int i = tid; i < n; i += MB_GATE_THREADS) {
        const float d = db[e0 + i];
        if (!(d > fl)) sum += g[e0 + i];
        if (d > mx) { mx = d; arg = i; }
    }
    s_sum[tid] = sum; s_max[tid] = mx; s_arg[tid] = arg;
    __syncthreads();
    for (int o = MB_GATE_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) {
            s_sum[tid] += s_sum[tid + o];
            const float m2 = s_max[tid + o];
            const int a2 = s_arg[tid + o];
            if (m2 > s_max[tid] || (m2 == s_max[tid] && a2 < s_arg[tid])) { s_max[tid] = m2; s_arg[tid] = a2; }
        }
        __syncthreads();
    }
    const float routed = s_sum[0];
    const int amax = s_arg[0];
    const float db_amin = 10.0f * log10f(amin_sq);            // the forward's value of every element under amin
    for (int i = tid; i < n; i += MB_GATE_THREADS) {
        const float d = db[e0 + i];
        float gd = d > fl ? g[e0 + i] : 0.f;
        if (i == amax) gd += routed;
        // d db / d M = 20 / (ln 10 M)
        dm[e0 + i] = d > db_amin ? gd * (8.6858896380650365530f * exp2f(d * -0.16609640474436811739f)) : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------------
// per frame: d L / d M [48] -> d L / d (the frame's win samples)
// ---------------------------------------------------------------------------------------------------------
// 4096-point complex FFT in LDS, in place, autosort (Stockham): a thread takes its butterflies into registers, the workgroup meets,
// the results are written in the sorted order.  Stage 1 is radix 16 (two radix-4 levels in registers, constant twiddles W16^(m0 p1)):
// in[j + 256 m] -> out[16 j + p], sixteen consecutive values per thread, stored as 128-bit words.  Stages 2..5 are radix 4 with
// Ns = 16, 64, 256, 1024: in[j + 1024 r] * W_(4 Ns)^(r k) -> DFT4 -> out[4 (j - k) + k + r Ns], k = j mod Ns.  Twiddles from the
// first quarter of the forward's table (cos, -sin)(2 pi m / 4096), staged in LDS: W^(1024 q + r) = W^r (-i)^q, q <= 2.
// Element i lives at mb_at(i): two complex values of padding behind every sixteen, so that the 128-byte runs of stage 1 (and the
// strided writes of stage 2) spread over the LDS banks instead of all starting on one.
#define MB_BUF (MB_N + MB_N / 8)
NQ_DEV int mb_at(int i) { return i + ((i >> 4) << 1); }
NQ_DEV cf mb_twiddle(const cf* tw, int m) {
    const cf w = tw[m & 1023];
    const int q = m >> 10;
    return q == 0 ? w : (q == 1 ? cf{w.y, -w.x} : cf{-w.x, -w.y});
}
// a[p] <- sum_s a[s] exp(-2 pi i s p / 4), natural order
NQ_DEV void mb_dft4(cf& a0, cf& a1, cf& a2, cf& a3) {
    const cf t0 = cf{a0.x + a2.x, a0.y + a2.y}, t1 = cf{a0.x - a2.x, a0.y - a2.y};
    const cf t2 = cf{a1.x + a3.x, a1.y + a3.y}, d = cf{a1.x - a3.x, a1.y - a3.y};
    a0 = cf{t0.x + t2.x, t0.y + t2.y};
    a1 = cf{t1.x + d.y, t1.y - d.x};                          // t1 - i d
    a2 = cf{t0.x - t2.x, t0.y - t2.y};
    a3 = cf{t1.x - d.y, t1.y + d.x};                          // t1 + i d
}
NQ_DEV void mb_fft4096(cf* buf, const cf* tw, int tid) {
    {
        cf x[16];
#pragma unroll
        for (int m = 0; m < 16; ++m) x[m] = buf[mb_at(tid + 256 * m)];
#pragma unroll
        for (int m0 = 0; m0 < 4; ++m0) mb_dft4(x[m0], x[4 + m0], x[8 + m0], x[12 + m0]);      // over m1: x[4 p1 + m0]
        const float c1 = 0.92387953251128675613f, s1 = 0.38268343236508977173f, r2 = 0.70710678118654752440f;
        x[5] = mb_cmul(x[5], cf{c1, -s1});   x[6] = mb_cmul(x[6], cf{r2, -r2});    x[7] = mb_cmul(x[7], cf{s1, -c1});      // W16^1, 2, 3
        x[9] = mb_cmul(x[9], cf{r2, -r2});   x[10] = cf{x[10].y, -x[10].x};        x[11] = mb_cmul(x[11], cf{-r2, -r2});   // W16^2, 4, 6
        x[13] = mb_cmul(x[13], cf{s1, -c1}); x[14] = mb_cmul(x[14], cf{-r2, -r2}); x[15] = mb_cmul(x[15], cf{-c1, s1});    // W16^3, 6, 9
#pragma unroll
        for (int p1 = 0; p1 < 4; ++p1) mb_dft4(x[4 * p1], x[4 * p1 + 1], x[4 * p1 + 2], x[4 * p1 + 3]);   // over m0: x[4 p1 + p0] = X[p1 + 4 p0]
        __syncthreads();
        f32x4* dst = (f32x4*)(buf + mb_at(16 * tid));
#pragma unroll
        for (int p0 = 0; p0 < 4; ++p0) {
            dst[2 * p0] = f32x4{x[p0].x, x[p0].y, x[4 + p0].x, x[4 + p0].y};                  // X[4 p0], X[4 p0 + 1]
            dst[2 * p0 + 1] = f32x4{x[8 + p0].x, x[8 + p0].y, x[12 + p0].x, x[12 + p0].y};    // X[4 p0 + 2], X[4 p0 + 3]
        }
        __syncthreads();
    }
    for (int ns = 16; ns < MB_N; ns <<= 2) {
        cf v[4][4];
        const int tstep = 1024 / ns;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = tid + 256 * q, k = j & (ns - 1);
            v[q][0] = buf[mb_at(j)];
            v[q][1] = mb_cmul(buf[mb_at(j + 1024)], mb_twiddle(tw, k * tstep));
            v[q][2] = mb_cmul(buf[mb_at(j + 2048)], mb_twiddle(tw, 2 * k * tstep));
            v[q][3] = mb_cmul(buf[mb_at(j + 3072)], mb_twiddle(tw, 3 * k * tstep));
            mb_dft4(v[q][0], v[q][1], v[q][2], v[q][3]);
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = tid + 256 * q, k = j & (ns - 1);
            const int j0 = ((j - k) << 2) + k;
#pragma unroll
            for (int r = 0; r < 4; ++r) buf[mb_at(j0 + r * ns)] = v[q][r];
        }
        __syncthreads();
    }
}

// One workgroup of 256 threads per frame.  d L / d |X_k| is scattered band by band into LDS, the even bands first, then the odd
// ones: the supports of two triangles m and m + 2 share no bin (only zero padding of the sparse rows overlaps, and zero weights
// are skipped), so a bin has one writer per pass and its two terms are added in band order.  The frame is loaded as the forward
// loads it -- through the clip's own offsets, reflected at the clip's own ends: no sample of another clip is read.
// (Measured and dropped: one thread per ENTRY of band_w with the band found by bisection -- 3.7 ms against 2.8 ms at 64 x 10 s.)
__global__ __launch_bounds__(256) void mel_frame_bwd_kernel(
    const float* __restrict__ pcm, const int64_t* __restrict__ clip_off, const int32_t* __restrict__ frame_off, int n_clips,
    int hop, int win, int w_floats, const float* __restrict__ window, const float2* __restrict__ twg,
    const int32_t* __restrict__ band_start, const int32_t* __restrict__ band_len, const int32_t* __restrict__ band_woff,
    const float* __restrict__ band_w, const float* __restrict__ dm, float* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) cf buf[MB_BUF];
    __shared__ float da[MB_BINS + 3];
    __shared__ float s_dm[NISQA_N_MELS];
    __shared__ cf tw[1024];
    const int tid = threadIdx.x, f = blockIdx.x;
    float* out = ws + (int64_t)f * win;
    if (tid < NISQA_N_MELS) s_dm[tid] = dm[(int64_t)f * NISQA_N_MELS + tid];
    for (int i = tid; i < MB_BINS + 3; i += 256) da[i] = 0.f;
    __syncthreads();
    bool live = false;                                        // block-uniform: any band with a gradient
    for (int m = 0; m < NISQA_N_MELS; ++m) live = live || s_dm[m] != 0.f;
    if (!live) {                                              // silent, sub-amin or uncovered frame: exact zeros
        for (int n = tid; n < win; n += 256) out[n] = 0.f;
        return;
    }
    const int b = find_segment(frame_off, n_clips, f);
    const int64_t c0 = clip_off[b];
    const int L = (int)(clip_off[b + 1] - c0);
    const int s0 = (f - frame_off[b]) * hop + mb_start0(win);
    const float* y = pcm + c0;
    for (int n = tid; n < MB_N; n += 256) buf[mb_at(n)] = cf{n < win ? y[mb_reflect(s0 + n, L)] * window[n] : 0.f, 0.f};
    for (int i = tid; i < 1024; i += 256) tw[i] = twg[i];
    for (int par = 0; par < 2; ++par) {
        for (int m = par; m < NISQA_N_MELS; m += 2) {
            const int st = band_start[m], len = band_len[m], wo = band_woff[m];
            const float d = s_dm[m];
            for (int j = tid; j < len; j += 256) {
                const int k = st + j;
                if ((unsigned)k < (unsigned)MB_BINS && (unsigned)(wo + j) < (unsigned)w_floats) {
                    const float w = band_w[wo + j];
                    if (w != 0.f) da[k] = fmaf(w, d, da[k]);
                }
            }
        }
        __syncthreads();
    }
    mb_fft4096(buf, tw, tid);
    // conj of the Hermitian extension of G_k = d L / d |X_k| X_k / |X_k| (half weight inside, the real part at k = 0 and 2048), so
    // that one more forward transform returns conj(sum_k H_k e^(+2 pi i k n / 4096)), whose real part is the wanted sum.  Bin k is
    // read and bins k and 4096 - k are written by one thread; reads touch [0, 2048], the mirrored writes (2048, 4096).
    for (int k = tid; k < MB_BINS; k += 256) {
        const cf x = buf[mb_at(k)];
        const float p = fmaf(x.x, x.x, x.y * x.y);
        const float s = p > 0.f ? da[k] / sqrtf(p) : 0.f;   // |X_k| = 0 (or below fp32's square): no direction, contribution 0
        const cf gk = cf{s * x.x, s * x.y};
        if (k == 0 || k == MB_N / 2) buf[mb_at(k)] = cf{gk.x, 0.f};
        else {
            buf[mb_at(k)] = cf{0.5f * gk.x, -0.5f * gk.y};
            buf[mb_at(MB_N - k)] = cf{0.5f * gk.x, 0.5f * gk.y};
        }
    }
    __syncthreads();
    mb_fft4096(buf, tw, tid);
    for (int n = tid; n < win; n += 256) out[n] = buf[mb_at(n)].x * window[n];
}

// ---------------------------------------------------------------------------------------------------------
// ws [TT][win] -> d L / d pcm: the adjoint of framing and reflect padding
// ---------------------------------------------------------------------------------------------------------
// One thread per sample j of a clip of L samples.  The padded positions that read it are j itself, -j (the left reflection) and
// 2 (L - 1) - j (the right one), each checked against mb_reflect; position p is tap p - start0 - f hop of every frame f with
// 0 <= that tap < win.  Added in the order (position, frame ascending).
__global__ __launch_bounds__(256) void mel_overlap_add_bwd_kernel(
    const float* __restrict__ ws, const int64_t* __restrict__ clip_off, const int32_t* __restrict__ frame_off, int n_clips,
    int64_t total, int hop, int win, float* __restrict__ dpcm) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    int lo = 0, hi = n_clips;                                 // clip_off[lo] <= i < clip_off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (clip_off[mid] <= i) lo = mid; else hi = mid;
    }
    const int b = lo;
    const int64_t c0 = clip_off[b];
    const int L = (int)(clip_off[b + 1] - c0), j = (int)(i - c0);
    const int fb = frame_off[b], T = frame_off[b + 1] - fb;
    const int start0 = mb_start0(win);
    float acc = 0.f;
    for (int c = 0; c < 3; ++c) {
        if ((c == 1 && j == 0) || (c == 2 && j >= L - 1)) continue;
        const int p = c == 0 ? j : (c == 1 ? -j : 2 * (L - 1) - j);
        if (mb_reflect(p, L) != j) continue;
        const int q = p - start0;                             // tap of frame 0
        if (q < 0) continue;
        const int f_hi = min(q / hop, T - 1);
        const int f_lo = q - win + 1 <= 0 ? 0 : (q - win + hop) / hop;
        for (int f = f_lo; f <= f_hi; ++f) acc += ws[(int64_t)(fb + f) * win + (q - f * hop)];
    }
    dpcm[i] = acc;
}

// ---------------------------------------------------------------------------------------------------------
// d L / d x [B][l_max][1][48][15] -> d L / d (clamped mel) [TT][48]: the adjoint of cutting segments
// ---------------------------------------------------------------------------------------------------------
// Segment k of clip b holds frames seg_hop k .. seg_hop k + 14.  One thread per (frame, band) adds the segments k < n_wins[b] that
// hold the frame, k ascending; a frame no segment holds gets 0; rows k >= n_wins[b] are never read.
__global__ __launch_bounds__(256) void segments_to_mel_bwd_kernel(
    const float* __restrict__ dx, int l_max, const int32_t* __restrict__ n_wins, const int32_t* __restrict__ frame_off, int n_clips,
    int64_t total, int seg_hop, float* __restrict__ dmel) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int tg = (int)(i / NISQA_N_MELS), m = (int)(i - (int64_t)tg * NISQA_N_MELS);
    const int b = find_segment(frame_off, n_clips, tg);
    const int t = tg - frame_off[b];
    const int n = min(n_wins[b], l_max);
    const int k_lo = t <= 14 ? 0 : (t - 14 + seg_hop - 1) / seg_hop;
    const int k_hi = min(t / seg_hop, n - 1);
    float acc = 0.f;
    for (int k = k_lo; k <= k_hi; ++k) acc += dx[(((int64_t)b * l_max + k) * NISQA_N_MELS + m) * 15 + (t - seg_hop * k)];
    dmel[i] = acc;
}

// ---------------------------------------------------------------------------------------------------------
// unclamped dB rows [TT][48] + clip_floor -> x [n_clips][L][1][48][15]: clamp and cut segments (the forward of the kernel above)
// ---------------------------------------------------------------------------------------------------------
// One wave per row (b, k) of x, four rows per workgroup.  A segment's source is 15 consecutive rows of mel_db: 720 contiguous
// floats, read as 180 128-bit words, lane after lane (three wave loads), clamped at the clip's floor and written to LDS at their
// place in the destination [48][15]; the 720 floats of the destination are contiguous too and leave as 180 128-bit words, lane
// after lane.  (The transposing LDS write is 32-bit: element (frame j, band m) goes to 15 m + j, at most two lanes of a group on
// one bank.)  Rows k >= n_wins[b] -- and a segment that would read past its clip's frames, which a consistent plan never has --
// are written as zeros.  Every element of x is written once, by one lane.
#define MS_SEG (NISQA_N_MELS * 15)           // floats of one segment: 720
#define MS_WORDS (MS_SEG / 4)                // 128-bit words of one segment: 180
__global__ __launch_bounds__(256) void mel_segments_fwd_kernel(
    const float* __restrict__ mel_db, const float* __restrict__ clip_floor, const int32_t* __restrict__ frame_off,
    const int32_t* __restrict__ n_wins, int n_rows, int total_frames, int seg_hop, int L, float* __restrict__ x) {
    __shared__ __attribute__((aligned(16))) float tile[4][MS_SEG];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + wave;                      // wave-uniform: row b * L + k of x
    const bool in_x = r < n_rows;
    bool cut = false;
    if (in_x) {
        const int b = r / L, k = r - b * L;
        const int64_t f0 = frame_off[b] + (int64_t)seg_hop * k;
        cut = k < n_wins[b] && frame_off[b] >= 0 && f0 + 15 <= frame_off[b + 1] && f0 + 15 <= total_frames;
        if (cut) {
            const float fl = clip_floor[b];
            const f32x4* src = (const f32x4*)(mel_db + (int64_t)f0 * NISQA_N_MELS);
#pragma unroll
            for (int it = 0; it < 3; ++it) {
                const int i = lane + 64 * it;
                if (i < MS_WORDS) {
                    const f32x4 v = src[i];
                    const int j = i / 12, m = 4 * (i - 12 * j);
#pragma unroll
                    for (int e = 0; e < 4; ++e) tile[wave][(m + e) * 15 + j] = fmaxf(v[e], fl);
                }
            }
        }
    }
    __syncthreads();
    if (!in_x) return;
    f32x4* dst = (f32x4*)(x + (int64_t)r * MS_SEG);
    const f32x4* t4 = (const f32x4*)tile[wave];
#pragma unroll
    for (int it = 0; it < 3; ++it) {
        const int i = lane + 64 * it;
        if (i < MS_WORDS) dst[i] = cut ? t4[i] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

static bool mel_bwd_cfg_ok(const nisqa_mel_cfg* cfg) {
    return cfg && cfg->n_fft == MB_N && cfg->n_mels == NISQA_N_MELS && cfg->win >= 2 && cfg->win <= MB_N && cfg->hop >= 1 &&
           cfg->w_floats >= 1 && cfg->w_floats <= 8192 && cfg->amin_sq > 0.f;
}

extern "C" int nisqa_mel_db_bwd_gate(const float* g, const float* mel_db, const float* clip_floor, const int32_t* frame_off,
                                     int32_t n_clips, int32_t total_frames, const nisqa_mel_cfg* cfg, float* dmel_amp, void* stream) {
    if (!g || !mel_db || !clip_floor || !frame_off || !dmel_amp || n_clips <= 0 || total_frames <= 0 || n_clips > total_frames ||
        (int64_t)total_frames * NISQA_N_MELS > 0x7fffffffLL || !mel_bwd_cfg_ok(cfg))
        return NISQA_ERR_ARG;
    NQ_LAUNCH_BEGIN();
    hipLaunchKernelGGL(mel_db_bwd_gate_kernel, dim3(n_clips), dim3(MB_GATE_THREADS), 0, (hipStream_t)stream, g, mel_db, clip_floor,
                       frame_off, cfg->amin_sq, dmel_amp);
    return NQ_LAUNCH_STATUS();
}

extern "C" int64_t nisqa_mel_bwd_workspace_bytes(int32_t total_frames, int32_t win) {
    if (total_frames <= 0 || win < 2 || win > MB_N) return 0;
    return (int64_t)total_frames * win * (int64_t)sizeof(float);
}

extern "C" int nisqa_mel_frame_bwd(const float* pcm, const int64_t* clip_off, const int32_t* frame_off, int32_t n_clips,
                                   int32_t total_frames, const nisqa_mel_cfg* cfg, const float* window, const float* twiddle,
                                   const int32_t* band_start, const int32_t* band_len, const int32_t* band_woff, const float* band_w,
                                   const float* dmel_amp, float* ws, int64_t ws_bytes, void* stream) {
    if (!pcm || !clip_off || !frame_off || !window || !twiddle || !band_start || !band_len || !band_woff || !band_w || !dmel_amp ||
        !ws || n_clips <= 0 || total_frames <= 0 || n_clips > total_frames || !mel_bwd_cfg_ok(cfg))
        return NISQA_ERR_ARG;
    if (ws_bytes < nisqa_mel_bwd_workspace_bytes(total_frames, cfg->win)) return NISQA_ERR_WORKSPACE;
    NQ_LAUNCH_BEGIN();
    hipLaunchKernelGGL(mel_frame_bwd_kernel, dim3(total_frames), dim3(256), 0, (hipStream_t)stream, pcm, clip_off, frame_off, n_clips,
                       cfg->hop, cfg->win, cfg->w_floats, window, (const float2*)twiddle, band_start, band_len, band_woff, band_w,
                       dmel_amp, ws);
    return NQ_LAUNCH_STATUS();
}

extern "C" int nisqa_mel_overlap_add_bwd(const float* ws, const int64_t* clip_off, const int32_t* frame_off, int32_t n_clips,
                                         int32_t total_frames, int64_t total_samples, const nisqa_mel_cfg* cfg, float* dpcm,
                                         void* stream) {
    if (!ws || !clip_off || !frame_off || !dpcm || n_clips <= 0 || total_frames <= 0 || n_clips > total_frames ||
        total_samples < n_clips || (total_samples + 255) / 256 > 0x7fffffffLL || !mel_bwd_cfg_ok(cfg))
        return NISQA_ERR_ARG;
    NQ_LAUNCH_BEGIN();
    hipLaunchKernelGGL(mel_overlap_add_bwd_kernel, dim3((unsigned)((total_samples + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ws,
                       clip_off, frame_off, n_clips, total_samples, cfg->hop, cfg->win, dpcm);
    return NQ_LAUNCH_STATUS();
}

extern "C" int nisqa_segments_to_mel_bwd(const float* dx, int32_t l_max, const int32_t* n_wins, const int32_t* frame_off,
                                         int32_t n_clips, int32_t total_frames, int32_t seg_hop, float* dmel, void* stream) {
    if (!dx || !n_wins || !frame_off || !dmel || l_max <= 0 || n_clips <= 0 || total_frames <= 0 || n_clips > total_frames ||
        seg_hop <= 0 || (int64_t)total_frames * NISQA_N_MELS > 0x7fffffffLL)
        return NISQA_ERR_ARG;
    const int64_t total = (int64_t)total_frames * NISQA_N_MELS;
    NQ_LAUNCH_BEGIN();
    hipLaunchKernelGGL(segments_to_mel_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dx, l_max,
                       n_wins, frame_off, n_clips, total, seg_hop, dmel);
    return NQ_LAUNCH_STATUS();
}

extern "C" int nisqa_mel_segments_fwd(const float* mel_db, const float* clip_floor, const int32_t* frame_off, const int32_t* n_wins,
                                      int32_t n_clips, int32_t total_frames, int32_t seg_hop, int32_t L, float* x, void* stream) {
    if (!mel_db || !clip_floor || !frame_off || !n_wins || !x || n_clips <= 0 || total_frames <= 0 || n_clips > total_frames ||
        seg_hop < 1 || L < 1 || (int64_t)n_clips * L > 0x7fffffffLL - 3 || (int64_t)total_frames * NISQA_N_MELS > 0x7fffffffLL ||
        ((uintptr_t)mel_db & 15) || ((uintptr_t)x & 15))
        return NISQA_ERR_ARG;
    const int n_rows = n_clips * L;
    NQ_LAUNCH_BEGIN();
    hipLaunchKernelGGL(mel_segments_fwd_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, mel_db, clip_floor,
                       frame_off, n_wins, n_rows, total_frames, seg_hop, L, x);
    return NQ_LAUNCH_STATUS();
}
