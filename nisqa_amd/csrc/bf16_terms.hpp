// Split-bf16 operands: fp32 values as sums of bf16 terms on the bf16 matrix pipe, shared by every kernel that runs fp32 operands
// that way.  A value splits into T terms, each the bf16 rounding (to nearest) of what the terms before it leave:
// |term t + 1| <= 2^-8 |term t|.  T = 2 (hi + lo, 16 of an fp32 operand's 24 significand bits) in the fast modes, T = 3 (hi + mid +
// lo) an EXACT split in the default 'bf16x6'.  The products of A term i and B term j are formed for i + j <= T - 1, smallest first.
// The order of the products is part of the arithmetic (fp32 accumulation is not associative): a loop that issues them in another
// order stays with its kernel.
#pragma once
#include "common.hpp"

#define NQ_AS3 __attribute__((address_space(3)))
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef unsigned short u16;
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// 32x32x16: A[i = l & 31][k = 8 * (l >> 5) + e], D in the layout of mfma32 (common.hpp)
NQ_DEV f32x16 mfma_bf(f32x4 a, f32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
// 16x16x32: A[i = l & 15][k = 8 * (l >> 4) + e], D row 4 * (l >> 4) + r
NQ_DEV f32x4 mfma_bf16x16(f32x4 a, f32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// fp32 -> bf16 (round to nearest even), two values per instruction: the compiler selects v_cvt_pk_bf16_f32 for
// this conversion, and -- unlike an inline-asm statement -- tracks its hazards and schedules around it
NQ_DEV unsigned cvt_pk_bf16(float a, float b) {
    const f32x2_t v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_t));
}
// (v0, v1) -> packed bf16 hi pair and packed bf16 lo pair
NQ_DEV void split2(float v0, float v1, unsigned& hi, unsigned& lo) {
    hi = cvt_pk_bf16(v0, v1);
    lo = cvt_pk_bf16(v0 - __uint_as_float(hi << 16), v1 - __uint_as_float(hi & 0xffff0000u));
}
// (v0, v1) -> T packed bf16 pairs, the residual as a packed subtraction; for T = 3, v = t[0] + t[1] + t[2] exactly
template <int T>
NQ_DEV void split2t(float v0, float v1, unsigned (&t)[T]) {
    f32x2_t r = {v0, v1};
#pragma unroll
    for (int q = 0; q < T; ++q) {
        t[q] = cvt_pk_bf16(r[0], r[1]);
        if (q + 1 < T) r = r - f32x2_t{__uint_as_float(t[q] << 16), __uint_as_float(t[q] & 0xffff0000u)};
    }
}

// ---- the term products, smallest first; within an order the product with the smaller A term first, consecutive MFMAs on
// different accumulators ----
// acc[m][nt] += a[m] x b[nt] (32x32x16)
template <int T, int MT, int NT>
NQ_DEV void mma_terms(f32x16 (&acc)[MT][NT], const f32x4 (&a)[MT][T], const f32x4 (&b)[NT][T]) {
#pragma unroll
    for (int order = T - 1; order >= 0; --order)
#pragma unroll
        for (int i = order; i >= 0; --i) {
            const int j = order - i;
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[m][nt] = mfma_bf(a[m][i], b[nt][j], acc[m][nt]);
        }
}
// acc[m] += a[m] x b (32x32x16, one B tile)
template <int T, int MT>
NQ_DEV void mma_terms(f32x16 (&acc)[MT], const f32x4 (&a)[MT][T], const f32x4 (&b)[T]) {
#pragma unroll
    for (int order = T - 1; order >= 0; --order)
#pragma unroll
        for (int i = order; i >= 0; --i)
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[m] = mfma_bf(a[m][i], b[order - i], acc[m]);
}
// acc[m] += a[m] x b (16x16x32, one B tile)
template <int T, int MT>
NQ_DEV void mma16_terms(f32x4 (&acc)[MT], const f32x4 (&a)[MT][T], const f32x4 (&b)[T]) {
#pragma unroll
    for (int order = T - 1; order >= 0; --order)
#pragma unroll
        for (int i = order; i >= 0; --i)
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[m] = mfma_bf16x16(a[m][i], b[order - i], acc[m]);
}
// acc[m][nt] += a[m] x b[nt] (16x16x32)
template <int T, int MT, int NT>
NQ_DEV void mma16_terms(f32x4 (&acc)[MT][NT], const f32x4 (&a)[MT][T], const f32x4 (&b)[NT][T]) {
#pragma unroll
    for (int order = T - 1; order >= 0; --order)
#pragma unroll
        for (int i = order; i >= 0; --i) {
            const int j = order - i;
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[m][nt] = mfma_bf16x16(a[m][i], b[nt][j], acc[m][nt]);
        }
}
