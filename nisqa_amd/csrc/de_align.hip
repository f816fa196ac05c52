// Alignment + fusion of the double-ended model (NISQA_DE, reference nisqa/NISQA_lib.py:406-424): for every degraded token i the
// reference's token it aligns to, then the fused feature row -- Alignment.forward (NISQA_lib.py:1264-1270) with AttDot / AttCosine
// (:1272-1294) and ApplyHardAttention / ApplySoftAttention (:1359-1378), then Fusion.forward (:1405-1417) without lin_fusion.
//
// One workgroup (4 waves) per 64-token tile of one degraded clip.  Each lane keeps ONE degraded token's 64 features in registers
// (lane i of every wave: token i of the tile); the clip's reference tokens stream through LDS in 64-token blocks (16 KB), wave w
// scoring rows 16 w .. 16 w + 15 of each block.  Every lane of a wave reads the same LDS row at the same time (a broadcast), so the
// score loop is conflict-free; a score is a k-ordered fp32 fma chain over the 64 features -- exact fp32 in every precision form.
//   hard: a running (max, index) per lane over its rows, ascending, strict '>' (the lowest index wins a tie, as torch's argmax);
//         the four waves' winners are merged the same way.  The reference takes the argmax of the SOFTMAX of the scores; the two
//         can only differ where rounding of the softmax merges scores a few ulps apart -- this kernel takes it over the raw scores
//         (DESIGN.md 4.8).
//   soft: an online softmax per lane (block max, one rescale of the 64 accumulators per block), the four waves' (max, sum, rows)
//         merged through LDS in a fixed order (deterministic).
//   cosine: every row divided by max(||row||, 1e-8) once, then the dot product -- torch's CosineSimilarity, which normalises each
//         operand before the product (not q.y / (|q| |y|)).
// Reference tokens j >= n_wins_y are never read (the reference masks their scores to -inf).  Rows of degraded tokens >= n_wins_x
// are written as zeros: the second self-attention multiplies them by zero probabilities, where a NaN would survive.
#include "common.hpp"
#include "../../include/nisqa_hip.h"
#include "../../include/nisqa_train.h"

namespace {

constexpr int DA_D = 64;                               // feature width of the first self-attention (d_model)
constexpr int DA_TILE = 64;                            // degraded tokens per workgroup
constexpr int DA_BLK = 64;                             // reference tokens per LDS block
constexpr int DA_WAVES = 4;
constexpr int DA_ROWS = DA_BLK / DA_WAVES;             // rows of a block one wave scores

// The two ways a row reaches the score loop, shared by the forward and the soft backward.  A DEGRADED row's squared norm is ONE
// k-ordered chain over its 64 features, a REFERENCE row's four 16-feature chains added as (s0 + s1) + (s2 + s3): the forward
// holds degraded rows one per lane (load_row<true>) and stages reference rows four threads per row (stage_rows<false>); the
// backward's reference-side kernel has the roles swapped (load_row<false>, stage_rows<true>) and must still get the forward's
// bits for every normalised row, hence the DEG_SIDE switch on how the norm is summed.
//
// stage_rows: rows r0 .. r0 + 63 of a clip of n rows at `rows` into LDS, thread t -> row t >> 2, features 16 (t & 3) .. + 15; rows
// behind n as zeros.  dst: the rows as the scores read them (normalised for cosine); raw (cosine only, may be null): the rows
// themselves.  With DEG_SIDE each of a row's four threads runs the whole 64-feature chain.  Every thread of the workgroup calls it.
template <bool DEG_SIDE>
__device__ __forceinline__ void stage_rows(const float* __restrict__ rows, int r0, int n, int cosine, int t, float (*dst)[DA_D],
                                           float (*raw)[DA_D]) {
    const int jr = t >> 2, f0 = 16 * (t & 3), j = r0 + jr;
    f32x4 v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = j < n ? *(const f32x4*)(rows + (size_t)j * DA_D + f0 + 4 * e) : f32x4{0.f, 0.f, 0.f, 0.f};
    if (cosine) {
        if (raw)
#pragma unroll
            for (int e = 0; e < 4; ++e) *(f32x4*)(&raw[jr][f0 + 4 * e]) = v[e];
        float ss = 0.f;
        if constexpr (DEG_SIDE) {
            if (j < n)
#pragma unroll
                for (int d = 0; d < DA_D; d += 4) {
                    const f32x4 r4 = *(const f32x4*)(rows + (size_t)j * DA_D + d);
#pragma unroll
                    for (int k = 0; k < 4; ++k) ss = fmaf(r4[k], r4[k], ss);
                }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int k = 0; k < 4; ++k) ss = fmaf(v[e][k], v[e][k], ss);
            ss += __shfl_xor(ss, 1);
            ss += __shfl_xor(ss, 2);
        }
        const float nrm = fmaxf(sqrtf(ss), 1e-8f);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int k = 0; k < 4; ++k) v[e][k] = v[e][k] / nrm;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) *(f32x4*)(&dst[jr][f0 + 4 * e]) = v[e];
}

// load_row: this lane's row (zeros when !valid) -> v (normalised for cosine), returns ||row|| (1 for dot)
template <bool DEG_SIDE>
__device__ __forceinline__ float load_row(const float* __restrict__ p, bool valid, int cosine, float (&v)[DA_D]) {
    if (valid) {
#pragma unroll
        for (int d = 0; d < DA_D; d += 4) {
            const f32x4 x4 = *(const f32x4*)(p + d);
            v[d] = x4[0]; v[d + 1] = x4[1]; v[d + 2] = x4[2]; v[d + 3] = x4[3];
        }
    } else {
#pragma unroll
        for (int d = 0; d < DA_D; ++d) v[d] = 0.f;
    }
    if (!cosine) return 1.f;
    float ss = 0.f;
    if constexpr (DEG_SIDE) {
#pragma unroll
        for (int d = 0; d < DA_D; ++d) ss = fmaf(v[d], v[d], ss);
    } else {
        float s4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int d = 0; d < 16; ++d) s4[c] = fmaf(v[16 * c + d], v[16 * c + d], s4[c]);
        ss = (s4[0] + s4[1]) + (s4[2] + s4[3]);
    }
    const float len = sqrtf(ss), nrm = fmaxf(len, 1e-8f);
#pragma unroll
    for (int d = 0; d < DA_D; ++d) v[d] = v[d] / nrm;
    return len;
}

// PACKED = false: the inference layout -- every degraded clip starts at a multiple of 64 rows, workgroup g owns rows 64 g .. 64 g
// + 63 of x / out / idx_out, rows behind a clip's n_wins are padding and written as zeros.  PACKED = true: the training layout
// (nisqa_de_align_fuse_packed, nisqa_train.h) -- clips back to back at deg_off[b], tile_off the exclusive prefix sum of
// ceil(n_wins / 64) over the pairs, workgroup g owns up to 64 VALID rows of one clip and touches no other row.  Everything else,
// the arithmetic included, is the same code.
template <bool PACKED>
__global__ __launch_bounds__(256) void de_align_fuse_kernel(const float* __restrict__ x, const int32_t* __restrict__ deg_off,
                                                            const int32_t* __restrict__ deg_n, const int32_t* __restrict__ ref_off,
                                                            const int32_t* __restrict__ ref_n, int n_pairs, int cosine, int soft,
                                                            int fuse, int ld_out, float* __restrict__ out,
                                                            int32_t* __restrict__ idx_out, const int32_t* __restrict__ tile_off,
                                                            float* __restrict__ lse_out, float* __restrict__ a_out) {
    __shared__ float yb[DA_BLK][DA_D];                                 // one block of reference rows (normalised for cosine)
    __shared__ float mm[DA_WAVES][DA_TILE], ml[DA_WAVES][DA_TILE];     // (max, sum) or (best score, index) per wave and token
    const int t = threadIdx.x, i = t & 63, w = t >> 6;
    int tile0, b;                                                      // row of lane 0 in x / out / idx_out, the pair
    if constexpr (PACKED) {
        b = find_segment(tile_off, n_pairs, (int)blockIdx.x);
        tile0 = deg_off[b] + ((int)blockIdx.x - tile_off[b]) * DA_TILE;
    } else {
        tile0 = blockIdx.x * DA_TILE;
        b = find_segment(deg_off, n_pairs, tile0);
    }
    const int nx = deg_n[b], ny = ref_n[b];
    const int ti = tile0 - deg_off[b] + i;                             // this lane's token within its clip
    const bool valid = ti < nx;
    const int F = fuse == 0 ? 3 * DA_D : 2 * DA_D;
    const int q0 = 16 * w;                                             // output: features q0 .. q0 + 15 of every part
    if (!PACKED && tile0 - deg_off[b] >= nx) {                         // a tile of padding rows only
        float* o = out + (size_t)(tile0 + i) * ld_out;
        for (int p = 0; p < F / DA_D; ++p)
#pragma unroll
            for (int e = 0; e < 16; e += 4) *(f32x4*)(o + p * DA_D + q0 + e) = f32x4{0.f, 0.f, 0.f, 0.f};
        if (idx_out && w == 0) idx_out[tile0 + i] = -1;
        return;
    }
    const float* xr = x + (size_t)(tile0 + i) * DA_D;
    const float* yr0 = x + (size_t)ref_off[b] * DA_D;

    float q[DA_D];
    load_row<true>(xr, valid, cosine, q);

    float best = -INFINITY, m = -INFINITY, l = 0.f;                    // hard: (best, bi); soft: (m, l, o)
    int bi = 0;
    float o[DA_D];
#pragma unroll
    for (int d = 0; d < DA_D; ++d) o[d] = 0.f;

    const int nblk = (ny + DA_BLK - 1) / DA_BLK;
    for (int jb = 0; jb < nblk; ++jb) {
        __syncthreads();                                               // the previous block is consumed
        stage_rows<false>(yr0, jb * DA_BLK, ny, cosine, t, yb, nullptr);     // thread t -> row t >> 2, features 16 (t & 3) .. + 15
        __syncthreads();
        const int j0 = jb * DA_BLK + q0;                               // this wave's first row of the block
        const int nr = min(DA_ROWS, ny - j0);                          // valid rows of it (may be <= 0)
        if (!valid || nr <= 0) continue;
        float s[DA_ROWS];
#pragma unroll
        for (int r = 0; r < DA_ROWS; ++r) {
            float acc = 0.f;
#pragma unroll
            for (int d = 0; d < DA_D; d += 4) {
                const f32x4 y4 = *(const f32x4*)(&yb[q0 + r][d]);
                acc = fmaf(q[d], y4[0], acc);
                acc = fmaf(q[d + 1], y4[1], acc);
                acc = fmaf(q[d + 2], y4[2], acc);
                acc = fmaf(q[d + 3], y4[3], acc);
            }
            s[r] = r < nr ? acc : -INFINITY;                           // key mask (NISQA_lib.py:1258-1262)
        }
        if (!soft) {
#pragma unroll
            for (int r = 0; r < DA_ROWS; ++r)
                if (s[r] > best) { best = s[r]; bi = j0 + r; }
        } else {
            float mb = -INFINITY;
#pragma unroll
            for (int r = 0; r < DA_ROWS; ++r) mb = fmaxf(mb, s[r]);
            const float mn = fmaxf(m, mb);                             // finite: row j0 is valid
            const float alpha = expf(m - mn);                          // 0 while m is still -inf
            l *= alpha;
#pragma unroll
            for (int d = 0; d < DA_D; ++d) o[d] *= alpha;
#pragma unroll
            for (int r = 0; r < DA_ROWS; ++r) {
                if (r >= nr) break;
                const float p = expf(s[r] - mn);
                l += p;
#pragma unroll
                for (int d = 0; d < DA_D; d += 4) {                    // the RAW reference row (ApplySoftAttention: bmm(att, y))
                    const f32x4 y4 = *(const f32x4*)(yr0 + (size_t)(j0 + r) * DA_D + d);
                    o[d] = fmaf(p, y4[0], o[d]);
                    o[d + 1] = fmaf(p, y4[1], o[d + 1]);
                    o[d + 2] = fmaf(p, y4[2], o[d + 2]);
                    o[d + 3] = fmaf(p, y4[3], o[d + 3]);
                }
            }
            m = mn;
        }
    }

    // merge the four waves' partial results (through LDS, wave 1, 2, 3 in turn: a fixed order); wave 0 ends with the aligned row
    // (soft, left in yb as [feature][token]) or index (hard) of every token
    float (*buf)[DA_TILE] = yb;                                        // yb is free once the last block is scored
    mm[w][i] = soft ? m : best;
    ml[w][i] = soft ? l : __int_as_float(bi);
    __syncthreads();
    if (!soft) {
        if (w == 0 && valid) {
            for (int v = 1; v < DA_WAVES; ++v) {                       // a wave's rows ascend within a block but not across
                const float sv = mm[v][i];                             // blocks: compare (score, index) explicitly
                const int iv = __float_as_int(ml[v][i]);
                if (sv > best || (sv == best && iv < bi)) { best = sv; bi = iv; }
            }
            ml[0][i] = __int_as_float(bi);
        }
    } else {
        float M = -INFINITY, L = 0.f;
        for (int v = 0; v < DA_WAVES; ++v) M = fmaxf(M, mm[v][i]);
        for (int v = 0; v < DA_WAVES; ++v) L = fmaf(ml[v][i], valid ? expf(mm[v][i] - M) : 0.f, L);
        const float a = valid ? expf(m - M) : 0.f;                     // 0 for a wave that saw no valid row
#pragma unroll
        for (int d = 0; d < DA_D; ++d) o[d] *= a;
        for (int v = 1; v < DA_WAVES; ++v) {
            if (w == v)
#pragma unroll
                for (int d = 0; d < DA_D; ++d) buf[d][i] = o[d];
            __syncthreads();
            if (w == 0)
#pragma unroll
                for (int d = 0; d < DA_D; ++d) o[d] += buf[d][i];
            __syncthreads();
        }
        if (w == 0) {
            const float inv = valid ? 1.0f / L : 0.f;
#pragma unroll
            for (int d = 0; d < DA_D; ++d) buf[d][i] = o[d] * inv;
            if (lse_out && valid) lse_out[tile0 + i] = M + logf(L);    // p_ij = exp(s_ij - lse_i): what the backward rebuilds
        }
    }
    __syncthreads();

    // fusion: every wave writes features q0 .. q0 + 15 of each part of row i
    float* orow = out + (size_t)(tile0 + i) * ld_out;
    if (!valid) {
        if constexpr (PACKED) return;                                  // the next clip's row: not this workgroup's
        for (int p = 0; p < F / DA_D; ++p)
#pragma unroll
            for (int e = 0; e < 16; e += 4) *(f32x4*)(orow + p * DA_D + q0 + e) = f32x4{0.f, 0.f, 0.f, 0.f};
        if (idx_out && w == 0) idx_out[tile0 + i] = -1;
        return;
    }
    const int jsel = soft ? 0 : __float_as_int(ml[0][i]);
    if (idx_out && w == 0) idx_out[tile0 + i] = soft ? -1 : jsel;
#pragma unroll
    for (int e = 0; e < 16; e += 4) {
        const f32x4 xv = *(const f32x4*)(xr + q0 + e);
        f32x4 yv;
        if (soft) yv = f32x4{buf[q0 + e][i], buf[q0 + e + 1][i], buf[q0 + e + 2][i], buf[q0 + e + 3][i]};
        else yv = *(const f32x4*)(yr0 + (size_t)jsel * DA_D + q0 + e);
        if (a_out) *(f32x4*)(a_out + (size_t)(tile0 + i) * DA_D + q0 + e) = yv;     // the aligned row, kept for the backward
        if (fuse == 0) {                                              // 'x/y/-': [x, y, x - y]
            *(f32x4*)(orow + q0 + e) = xv;
            *(f32x4*)(orow + DA_D + q0 + e) = yv;
            *(f32x4*)(orow + 2 * DA_D + q0 + e) = xv - yv;
        } else if (fuse == 1) {                                        // '+/-': [x + y, x - y]
            *(f32x4*)(orow + q0 + e) = xv + yv;
            *(f32x4*)(orow + DA_D + q0 + e) = xv - yv;
        } else {                                                       // 'x/y': [x, y]
            *(f32x4*)(orow + q0 + e) = xv;
            *(f32x4*)(orow + DA_D + q0 + e) = yv;
        }
    }
}

// Backward of hard alignment + fusion (nisqa_de_align_fuse_bwd, nisqa_train.h): the argmax carries no gradient, so what is left
// is the adjoint of Fusion.forward (NISQA_lib.py:1405-1417) and of the gather ApplyHardAttention does (:1359-1366).
// Workgroup (r, b, side): four waves, wave w owns row 4 r + w of pair b's degraded (side 0) or reference (side 1) clip; lane =
// feature, so every row read or written is one 256-byte access.
//   side 0: dx[i] = g0 + g2 ('x/y/-'), g0 + g1 ('+/-'), g0 ('x/y') of row i of d_fused.
//   side 1: d_ref[j] = sum over the degraded tokens i with idx[i] == j, ASCENDING i, of dya[i] = g1 - g2, g0 - g1, g1 -- a gather:
//           the pair's idx goes through LDS in chunks of DB_CHUNK, every wave scans it 64 entries at a time (one ballot) and adds
//           the rows that chose its j, lowest i first, to one fp32 accumulator per lane, starting from 0.  No atomics: the bits are those of the sequential
//           sum.  A reference row nobody chose ends as zeros.
constexpr int DB_ROWS = 4;                             // rows (waves) per workgroup
constexpr int DB_CHUNK = 1024;                         // idx entries staged per pass

__global__ __launch_bounds__(64 * DB_ROWS) void de_align_fuse_bwd_kernel(const float* __restrict__ dF, int ld,
                                                                        const int32_t* __restrict__ idx,
                                                                        const int32_t* __restrict__ deg_off,
                                                                        const int32_t* __restrict__ deg_n,
                                                                        const int32_t* __restrict__ ref_off,
                                                                        const int32_t* __restrict__ ref_n, int fuse,
                                                                        float* __restrict__ d_deg, float* __restrict__ d_ref) {
    __shared__ int32_t sidx[DB_CHUNK];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int nx = deg_n[b], ny = ref_n[b];
    const int r = blockIdx.x * DB_ROWS + w;
    const size_t x0 = (size_t)deg_off[b];
    if (blockIdx.z == 0) {
        if (r >= nx) return;
        const float* g = dF + (x0 + r) * ld;
        float v = g[lane];
        if (fuse == 0) v = v + g[2 * DA_D + lane];
        else if (fuse == 1) v = v + g[DA_D + lane];
        d_deg[(x0 + r) * DA_D + lane] = v;
        return;
    }
    if ((int)blockIdx.x * DB_ROWS >= ny) return;                      // uniform over the workgroup: no wave of it has a row
    float acc = 0.f;
    for (int c0 = 0; c0 < nx; c0 += DB_CHUNK) {
        const int nc = min(DB_CHUNK, nx - c0);
        __syncthreads();                                               // the previous chunk is consumed
        for (int k = threadIdx.x; k < nc; k += 64 * DB_ROWS) sidx[k] = idx[x0 + c0 + k];
        __syncthreads();
        if (r < ny)                                                    // (r is uniform over the wave)
            for (int k0 = 0; k0 < nc; k0 += 64) {                      // 64 entries per ballot, then the matches in ascending order
                unsigned long long hit = __ballot(k0 + lane < nc && sidx[k0 + lane] == r);
                while (hit) {
                    const int k = k0 + __ffsll(hit) - 1;
                    hit &= hit - 1;
                    const float* g = dF + (x0 + c0 + k) * ld;
                    const float dya = fuse == 0 ? g[DA_D + lane] - g[2 * DA_D + lane] : fuse == 1 ? g[lane] - g[DA_D + lane] : g[DA_D + lane];
                    acc = acc + dya;
                }
            }
    }
    if (r < ny) d_ref[((size_t)ref_off[b] + r) * DA_D + lane] = acc;
}

// Backward of SOFT alignment + fusion (nisqa_de_align_soft_bwd, nisqa_train.h).  With q_i / y_j the degraded / reference rows, q^ /
// y^ the rows the scores are taken of (divided by max(||.||, 1e-8) for cosine, the rows themselves for dot), lse_i and a_i as the
// forward kept them, and (gx_i, ga_i) the fusion's adjoints of a d_fused row (the hard backward's dx and dya):
//     s_ij = q^_i . y^_j     p_ij = exp(s_ij - lse_i)     delta_i = ga_i . a_i     ds_ij = p_ij (ga_i . y_j - delta_i)
//     d_deg[i] = gx_i + N'(q_i)[ sum_j ds_ij y^_j ]
//     d_ref[j] = sum_i p_ij ga_i + N'(y_j)[ sum_i ds_ij q^_i ]
//     N'(v)[u] = (u - v^ (v^ . u)) / ||v|| for cosine (u / 1e-8 for a row at or under the clamp), u for dot.
// Two kernels in the forward's shape, no atomics: the degraded side keeps one degraded token per lane (q^, ga and one accumulator
// in registers) and streams the pair's reference rows through LDS in 64-row blocks; the reference side keeps one reference token
// per lane (y^ and two accumulators) and streams the degraded rows, their ga, lse and delta.  Wave w takes rows 16 w .. 16 w + 15
// of every block, ascending; the four waves' sums are merged through LDS, wave 1, 2, 3 in turn: a fixed order, so two runs give
// the same bits.  A score is the forward's k-ordered fp32 fma chain over the same operands, so p is the forward's p.
// fusion adjoints of features d .. d + 3 of one d_fused row
__device__ __forceinline__ void fuse_adjoint(const float* __restrict__ g, int fuse, int d, f32x4& gx, f32x4& ga) {
    const f32x4 g0 = *(const f32x4*)(g + d), g1 = *(const f32x4*)(g + DA_D + d);
    if (fuse == 0) {
        const f32x4 g2 = *(const f32x4*)(g + 2 * DA_D + d);
        gx = g0 + g2;
        ga = g1 - g2;
    } else if (fuse == 1) {
        gx = g0 + g1;
        ga = g0 - g1;
    } else {
        gx = g0;
        ga = g1;
    }
}

// u -> N'(v)[u] in place, for the lane that holds the whole row: vh = v^, nrm = ||v|| (unclamped)
__device__ __forceinline__ void cosine_adjoint(float (&u)[DA_D], const float (&vh)[DA_D], float nrm) {
    if (nrm > 1e-8f) {
        float dot = 0.f;
#pragma unroll
        for (int d = 0; d < DA_D; ++d) dot = fmaf(vh[d], u[d], dot);
#pragma unroll
        for (int d = 0; d < DA_D; ++d) u[d] = (u[d] - vh[d] * dot) / nrm;
    } else {
#pragma unroll
        for (int d = 0; d < DA_D; ++d) u[d] = u[d] / 1e-8f;
    }
}

// grid (ceil(max_n_wins / 64), n_pairs): workgroup (g, b) owns degraded tokens 64 g .. 64 g + 63 of pair b
__global__ __launch_bounds__(256) void de_align_soft_bwd_deg_kernel(const float* __restrict__ x, const float* __restrict__ dF, int ld,
                                                                    const float* __restrict__ lse, const float* __restrict__ al,
                                                                    const int32_t* __restrict__ deg_off,
                                                                    const int32_t* __restrict__ deg_n,
                                                                    const int32_t* __restrict__ ref_off,
                                                                    const int32_t* __restrict__ ref_n, int cosine, int fuse,
                                                                    float* __restrict__ d_deg) {
    __shared__ float yb[DA_BLK][DA_D];                                 // a block of reference rows as the scores read them
    __shared__ float yw[DA_BLK][DA_D];                                 // cosine: the same rows, raw
    const int t = threadIdx.x, i = t & 63, w = t >> 6, b = blockIdx.y;
    const int nx = deg_n[b], ny = ref_n[b];
    if ((int)blockIdx.x * DA_TILE >= nx) return;                       // uniform over the workgroup
    const int ti = blockIdx.x * DA_TILE + i;
    const bool valid = ti < nx;
    const size_t row = (size_t)deg_off[b] + ti;                        // in x, dF, lse, al and d_deg (read / written when valid)
    const float* yr0 = x + (size_t)ref_off[b] * DA_D;
    const int q0 = 16 * w;

    float q[DA_D], ga[DA_D], u[DA_D];
    const float len = load_row<true>(x + row * DA_D, valid, cosine, q);
    float delta = 0.f, ls = 0.f;
    if (valid) {
        const float* g = dF + row * ld;
        const float* ar = al + row * DA_D;
#pragma unroll
        for (int d = 0; d < DA_D; d += 4) {
            f32x4 gx, g4;
            fuse_adjoint(g, fuse, d, gx, g4);
            ga[d] = g4[0]; ga[d + 1] = g4[1]; ga[d + 2] = g4[2]; ga[d + 3] = g4[3];
            const f32x4 a4 = *(const f32x4*)(ar + d);
            delta = fmaf(g4[0], a4[0], delta);
            delta = fmaf(g4[1], a4[1], delta);
            delta = fmaf(g4[2], a4[2], delta);
            delta = fmaf(g4[3], a4[3], delta);
        }
        ls = lse[row];
    } else {
#pragma unroll
        for (int d = 0; d < DA_D; ++d) ga[d] = 0.f;
    }
#pragma unroll
    for (int d = 0; d < DA_D; ++d) u[d] = 0.f;

    float (*yt)[DA_D] = cosine ? yw : yb;                              // the rows ga is multiplied with: raw
    const int nblk = (ny + DA_BLK - 1) / DA_BLK;
    for (int jb = 0; jb < nblk; ++jb) {
        __syncthreads();                                               // the previous block is consumed
        stage_rows<false>(yr0, jb * DA_BLK, ny, cosine, t, yb, yw);
        __syncthreads();
        const int nr = min(DA_ROWS, ny - (jb * DA_BLK + q0));          // valid rows of this wave's part (may be <= 0): key mask
        if (!valid || nr <= 0) continue;
        for (int r = 0; r < nr; ++r) {
            const float* yh = yb[q0 + r];
            const float* yy = yt[q0 + r];
            float sc = 0.f, tt = 0.f;
#pragma unroll
            for (int d = 0; d < DA_D; d += 4) {                        // the forward's chain
                const f32x4 y4 = *(const f32x4*)(yh + d);
                sc = fmaf(q[d], y4[0], sc);
                sc = fmaf(q[d + 1], y4[1], sc);
                sc = fmaf(q[d + 2], y4[2], sc);
                sc = fmaf(q[d + 3], y4[3], sc);
            }
#pragma unroll
            for (int d = 0; d < DA_D; d += 4) {
                const f32x4 y4 = *(const f32x4*)(yy + d);
                tt = fmaf(ga[d], y4[0], tt);
                tt = fmaf(ga[d + 1], y4[1], tt);
                tt = fmaf(ga[d + 2], y4[2], tt);
                tt = fmaf(ga[d + 3], y4[3], tt);
            }
            const float ds = expf(sc - ls) * (tt - delta);
#pragma unroll
            for (int d = 0; d < DA_D; d += 4) {
                const f32x4 y4 = *(const f32x4*)(yh + d);
                u[d] = fmaf(ds, y4[0], u[d]);
                u[d + 1] = fmaf(ds, y4[1], u[d + 1]);
                u[d + 2] = fmaf(ds, y4[2], u[d + 2]);
                u[d + 3] = fmaf(ds, y4[3], u[d + 3]);
            }
        }
    }

    float (*buf)[DA_TILE] = yb;                                        // [feature][token], free once the last block is consumed
    for (int v = 1; v < DA_WAVES; ++v) {
        __syncthreads();
        if (w == v)
#pragma unroll
            for (int d = 0; d < DA_D; ++d) buf[d][i] = u[d];
        __syncthreads();
        if (w == 0)
#pragma unroll
            for (int d = 0; d < DA_D; ++d) u[d] += buf[d][i];
    }
    __syncthreads();
    if (w == 0) {
        if (cosine) cosine_adjoint(u, q, len);
#pragma unroll
        for (int d = 0; d < DA_D; ++d) buf[d][i] = u[d];
    }
    __syncthreads();
    if (!valid) return;
    const float* g = dF + row * ld;
#pragma unroll
    for (int e = 0; e < 16; e += 4) {                                  // every wave writes features q0 .. q0 + 15 of row i
        f32x4 gx, g4;
        fuse_adjoint(g, fuse, q0 + e, gx, g4);
        *(f32x4*)(d_deg + row * DA_D + q0 + e) =
            gx + f32x4{buf[q0 + e][i], buf[q0 + e + 1][i], buf[q0 + e + 2][i], buf[q0 + e + 3][i]};
    }
}

// grid (ceil(max_n_wins / 64), n_pairs): workgroup (g, b) owns reference tokens 64 g .. 64 g + 63 of pair b
__global__ __launch_bounds__(256) void de_align_soft_bwd_ref_kernel(const float* __restrict__ x, const float* __restrict__ dF, int ld,
                                                                    const float* __restrict__ lse, const float* __restrict__ al,
                                                                    const int32_t* __restrict__ deg_off,
                                                                    const int32_t* __restrict__ deg_n,
                                                                    const int32_t* __restrict__ ref_off,
                                                                    const int32_t* __restrict__ ref_n, int cosine, int fuse,
                                                                    float* __restrict__ d_ref) {
    __shared__ float qb[DA_BLK][DA_D];                                 // a block of degraded rows as the scores read them
    __shared__ float gb[DA_BLK][DA_D];                                 // their ga
    __shared__ float sl[DA_BLK], sd[DA_BLK];                           // their lse and delta
    const int t = threadIdx.x, i = t & 63, w = t >> 6, b = blockIdx.y;
    const int nx = deg_n[b], ny = ref_n[b];
    if ((int)blockIdx.x * DA_TILE >= ny) return;                       // uniform over the workgroup
    const int tj = blockIdx.x * DA_TILE + i;
    const bool valid = tj < ny;
    const size_t row = (size_t)ref_off[b] + tj;                        // in x and d_ref (read / written when valid)
    const size_t x0 = (size_t)deg_off[b];
    const int q0 = 16 * w;

    float y[DA_D], acc_p[DA_D], acc_s[DA_D];                           // y^_j, sum_i p_ij ga_i, sum_i ds_ij q^_i
    const float len = load_row<false>(x + row * DA_D, valid, cosine, y);
    const float back = cosine ? fmaxf(len, 1e-8f) : 1.f;               // y_j = back * y^_j
#pragma unroll
    for (int d = 0; d < DA_D; ++d) acc_p[d] = acc_s[d] = 0.f;

    const int nblk = (nx + DA_BLK - 1) / DA_BLK;
    for (int ib = 0; ib < nblk; ++ib) {
        __syncthreads();                                               // the previous block is consumed
        stage_rows<true>(x + x0 * DA_D, ib * DA_BLK, nx, cosine, t, qb, nullptr);
        {   // ga, lse and delta of the same rows: thread t -> row t >> 2, features 16 (t & 3) .. + 15
            const int jr = t >> 2, f0 = 16 * (t & 3), k = ib * DA_BLK + jr;
            float dl = 0.f;
#pragma unroll
            for (int e = 0; e < 16; e += 4) {
                f32x4 gx, g4 = f32x4{0.f, 0.f, 0.f, 0.f};
                if (k < nx) {
                    fuse_adjoint(dF + (x0 + k) * ld, fuse, f0 + e, gx, g4);
                    const f32x4 a4 = *(const f32x4*)(al + (x0 + k) * DA_D + f0 + e);
                    dl = fmaf(g4[0], a4[0], dl);
                    dl = fmaf(g4[1], a4[1], dl);
                    dl = fmaf(g4[2], a4[2], dl);
                    dl = fmaf(g4[3], a4[3], dl);
                }
                *(f32x4*)(&gb[jr][f0 + e]) = g4;
            }
            dl += __shfl_xor(dl, 1);
            dl += __shfl_xor(dl, 2);
            if ((t & 3) == 0) {
                sd[jr] = dl;
                sl[jr] = k < nx ? lse[x0 + k] : 0.f;
            }
        }
        __syncthreads();
        const int nr = min(DA_ROWS, nx - (ib * DA_BLK + q0));          // valid rows of this wave's part (may be <= 0)
        if (!valid || nr <= 0) continue;
        for (int r = 0; r < nr; ++r) {
            const float* qh = qb[q0 + r];
            const float* gg = gb[q0 + r];
            float sc = 0.f, tt = 0.f;
#pragma unroll
            for (int d = 0; d < DA_D; d += 4) {                        // the forward's chain: q^_i[k] * y^_j[k], k ascending
                const f32x4 q4 = *(const f32x4*)(qh + d);
                sc = fmaf(q4[0], y[d], sc);
                sc = fmaf(q4[1], y[d + 1], sc);
                sc = fmaf(q4[2], y[d + 2], sc);
                sc = fmaf(q4[3], y[d + 3], sc);
            }
#pragma unroll
            for (int d = 0; d < DA_D; d += 4) {
                const f32x4 g4 = *(const f32x4*)(gg + d);
                tt = fmaf(g4[0], y[d], tt);
                tt = fmaf(g4[1], y[d + 1], tt);
                tt = fmaf(g4[2], y[d + 2], tt);
                tt = fmaf(g4[3], y[d + 3], tt);
            }
            const float p = expf(sc - sl[q0 + r]);
            const float ds = p * (tt * back - sd[q0 + r]);             // ga_i . y_j = back (ga_i . y^_j)
#pragma unroll
            for (int d = 0; d < DA_D; d += 4) {
                const f32x4 g4 = *(const f32x4*)(gg + d);
                const f32x4 q4 = *(const f32x4*)(qh + d);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    acc_p[d + k] = fmaf(p, g4[k], acc_p[d + k]);
                    acc_s[d + k] = fmaf(ds, q4[k], acc_s[d + k]);
                }
            }
        }
    }

    float (*bp)[DA_TILE] = qb;                                         // [feature][token], free once the last block is consumed
    float (*bs)[DA_TILE] = gb;
    for (int v = 1; v < DA_WAVES; ++v) {
        __syncthreads();
        if (w == v)
#pragma unroll
            for (int d = 0; d < DA_D; ++d) { bp[d][i] = acc_p[d]; bs[d][i] = acc_s[d]; }
        __syncthreads();
        if (w == 0)
#pragma unroll
            for (int d = 0; d < DA_D; ++d) { acc_p[d] += bp[d][i]; acc_s[d] += bs[d][i]; }
    }
    __syncthreads();
    if (w == 0) {
        if (cosine) cosine_adjoint(acc_s, y, len);
#pragma unroll
        for (int d = 0; d < DA_D; ++d) bp[d][i] = acc_p[d] + acc_s[d];
    }
    __syncthreads();
    if (!valid) return;
#pragma unroll
    for (int e = 0; e < 16; e += 4)
        *(f32x4*)(d_ref + row * DA_D + q0 + e) = f32x4{bp[q0 + e][i], bp[q0 + e + 1][i], bp[q0 + e + 2][i], bp[q0 + e + 3][i]};
}

}  // namespace

extern "C" int nisqa_de_align_fuse(const float* x, const int32_t* deg_tok_off, const int32_t* deg_n_wins, const int32_t* ref_tok_off,
                                   const int32_t* ref_n_wins, int32_t n_pairs, int32_t total_deg_tok_padded, int32_t align,
                                   int32_t apply, int32_t fuse, int32_t ld_out, float* out, int32_t* idx_out, void* stream) {
    const int F = fuse == 0 ? 3 * DA_D : 2 * DA_D;
    if (n_pairs <= 0 || total_deg_tok_padded <= 0 || (total_deg_tok_padded % DA_TILE) || align < 0 || align > 1 || apply < 0 ||
        apply > 1 || fuse < 0 || fuse > 2 || ld_out < F || (ld_out & 3))
        return NISQA_ERR_ARG;
    NQ_LAUNCH_BEGIN();
    hipLaunchKernelGGL(de_align_fuse_kernel<false>, dim3(total_deg_tok_padded / DA_TILE), dim3(256), 0, (hipStream_t)stream, x,
                       deg_tok_off, deg_n_wins, ref_tok_off, ref_n_wins, n_pairs, align, apply, fuse, ld_out, out, idx_out,
                       (const int32_t*)nullptr, (float*)nullptr, (float*)nullptr);
    return NQ_LAUNCH_STATUS();
}

extern "C" int nisqa_de_align_fuse_packed(const float* x, const int32_t* deg_tok_off, const int32_t* deg_n_wins,
                                          const int32_t* ref_tok_off, const int32_t* ref_n_wins, const int32_t* tile_off,
                                          int32_t n_pairs, int32_t n_tiles, int32_t align, int32_t fuse, int32_t ld_out, float* out,
                                          int32_t* idx_out, void* stream) {
    const int F = fuse == 0 ? 3 * DA_D : 2 * DA_D;
    if (!x || !deg_tok_off || !deg_n_wins || !ref_tok_off || !ref_n_wins || !tile_off || !out || !idx_out || n_pairs <= 0 ||
        n_tiles < n_pairs || align < 0 || align > 1 || fuse < 0 || fuse > 2 || ld_out < F || (ld_out & 3))
        return NISQA_ERR_ARG;
    NQ_LAUNCH_BEGIN();
    hipLaunchKernelGGL(de_align_fuse_kernel<true>, dim3(n_tiles), dim3(256), 0, (hipStream_t)stream, x, deg_tok_off, deg_n_wins,
                       ref_tok_off, ref_n_wins, n_pairs, align, 0, fuse, ld_out, out, idx_out, tile_off, (float*)nullptr, (float*)nullptr);
    return NQ_LAUNCH_STATUS();
}

extern "C" int nisqa_de_align_fuse_bwd(const float* d_fused, int32_t ld, const int32_t* idx, const int32_t* deg_tok_off,
                                       const int32_t* deg_n_wins, const int32_t* ref_tok_off, const int32_t* ref_n_wins,
                                       int32_t n_pairs, int32_t max_n_wins, int32_t fuse, float* d_deg, float* d_ref, void* stream) {
    const int F = fuse == 0 ? 3 * DA_D : 2 * DA_D;
    if (!d_fused || !idx || !deg_tok_off || !deg_n_wins || !ref_tok_off || !ref_n_wins || !d_deg || !d_ref || n_pairs <= 0 ||
        n_pairs > 65535 || max_n_wins <= 0 || fuse < 0 || fuse > 2 || ld < F)
        return NISQA_ERR_ARG;
    NQ_LAUNCH_BEGIN();
    hipLaunchKernelGGL(de_align_fuse_bwd_kernel, dim3((max_n_wins + DB_ROWS - 1) / DB_ROWS, n_pairs, 2), dim3(64 * DB_ROWS), 0,
                       (hipStream_t)stream, d_fused, ld, idx, deg_tok_off, deg_n_wins, ref_tok_off, ref_n_wins, fuse, d_deg, d_ref);
    return NQ_LAUNCH_STATUS();
}

extern "C" int nisqa_de_align_soft_packed(const float* x, const int32_t* deg_tok_off, const int32_t* deg_n_wins,
                                          const int32_t* ref_tok_off, const int32_t* ref_n_wins, const int32_t* tile_off,
                                          int32_t n_pairs, int32_t n_tiles, int32_t align, int32_t fuse, int32_t ld_out, float* out,
                                          float* lse, float* aligned, void* stream) {
    const int F = fuse == 0 ? 3 * DA_D : 2 * DA_D;
    if (!x || !deg_tok_off || !deg_n_wins || !ref_tok_off || !ref_n_wins || !tile_off || !out || !lse || !aligned || n_pairs <= 0 ||
        n_tiles < n_pairs || align < 0 || align > 1 || fuse < 0 || fuse > 2 || ld_out < F || (ld_out & 3))
        return NISQA_ERR_ARG;
    NQ_LAUNCH_BEGIN();
    hipLaunchKernelGGL(de_align_fuse_kernel<true>, dim3(n_tiles), dim3(256), 0, (hipStream_t)stream, x, deg_tok_off, deg_n_wins,
                       ref_tok_off, ref_n_wins, n_pairs, align, 1, fuse, ld_out, out, (int32_t*)nullptr, tile_off, lse, aligned);
    return NQ_LAUNCH_STATUS();
}

extern "C" int nisqa_de_align_soft_bwd(const float* x, const float* d_fused, int32_t ld, const float* lse, const float* aligned,
                                       const int32_t* deg_tok_off, const int32_t* deg_n_wins, const int32_t* ref_tok_off,
                                       const int32_t* ref_n_wins, int32_t n_pairs, int32_t max_n_wins, int32_t align, int32_t fuse,
                                       float* d_deg, float* d_ref, void* stream) {
    const int F = fuse == 0 ? 3 * DA_D : 2 * DA_D;
    if (!x || !d_fused || !lse || !aligned || !deg_tok_off || !deg_n_wins || !ref_tok_off || !ref_n_wins || !d_deg || !d_ref ||
        n_pairs <= 0 || n_pairs > 65535 || max_n_wins <= 0 || align < 0 || align > 1 || fuse < 0 || fuse > 2 || ld < F || (ld & 3))
        return NISQA_ERR_ARG;
    const dim3 grid((max_n_wins + DA_TILE - 1) / DA_TILE, n_pairs);
    NQ_LAUNCH_BEGIN();
    hipLaunchKernelGGL(de_align_soft_bwd_deg_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, d_fused, ld, lse, aligned, deg_tok_off,
                       deg_n_wins, ref_tok_off, ref_n_wins, align, fuse, d_deg);
    hipLaunchKernelGGL(de_align_soft_bwd_ref_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, d_fused, ld, lse, aligned, deg_tok_off,
                       deg_n_wins, ref_tok_off, ref_n_wins, align, fuse, d_ref);
    return NQ_LAUNCH_STATUS();
}
