// nisqa_wav_decode: lb.load(path, sr=None, mono=...) (NISQA_lib.py:2299-2304) for a batch of WAV data chunks already in HBM --
// the bytes nisqa_ingest_read copied verbatim -> the float32 mono samples soundfile + librosa.to_mono return, bit for bit
// (nisqa_amd/wavio.py:_decode is the project's statement of both).  Bandwidth work: block_align bytes in, 4 bytes out per frame.
//
// One workgroup takes a tile of TILE frames of one clip, in passes of as many frames as fit STAGE bytes: the pass's byte range,
// widened to 16-byte boundaries (src_off is a multiple of 16, so the widening never leaves the clip's own slot by more than the
// pad in front of the next one), is staged with one 16-byte load per lane into LDS, and every lane then unpacks whole frames from
// LDS dwords -- no byte load ever goes to HBM.  A span that would cross raw_bytes is fetched byte by byte up to raw_bytes.
#include "common.hpp"
#include "../../include/nisqa_hip.h"

namespace {

constexpr int THREADS = 256;
constexpr int TILE = 1024;              // frames per workgroup
constexpr int STAGE = 16384;            // bytes of frames per pass (block_align <= MAX_BLOCK: at least 16 frames)
constexpr int MAX_BLOCK = 1024;         // channels * container the kernel takes
constexpr int SPANS = STAGE / 16 + 2;   // + the two partial spans at either end

NQ_DEV uint32_t bswap32(uint32_t v) { return __builtin_bswap32(v); }

// float64 bits -> float32 bits, round to nearest even, overflow to +-inf, results below the normal range as denormals (numpy's
// astype): integer arithmetic, so it depends on no floating-point mode of the kernel
NQ_DEV uint32_t f64_to_f32_bits(uint32_t lo, uint32_t hi) {
    const uint32_t sign = hi & 0x80000000u;
    const int e = (int)((hi >> 20) & 0x7FFu);
    const uint64_t mant = ((uint64_t)(hi & 0xFFFFFu) << 32) | lo;
    if (e == 0x7FF) return sign | 0x7F800000u | (mant ? (0x00400000u | (uint32_t)(mant >> 29)) : 0u);
    const int ef = e - 1023 + 127;
    if (ef >= 255) return sign | 0x7F800000u;
    if (ef <= 0) {
        if (e == 0 || ef < -24) return sign;                           // (below half of the smallest denormal)
        const uint64_t m = mant | (1ull << 52);
        const int sh = 30 - ef;                                        // 30 .. 54
        uint64_t q = m >> sh;
        const uint64_t rem = m & ((1ull << sh) - 1), half = 1ull << (sh - 1);
        q += (rem > half || (rem == half && (q & 1))) ? 1 : 0;
        return sign | (uint32_t)q;                                     // (a carry into bit 23 is the smallest normal)
    }
    uint32_t q = (uint32_t)(mant >> 29);
    const uint32_t rem = (uint32_t)mant & 0x1FFFFFFFu;
    q += (rem > 0x10000000u || (rem == 0x10000000u && (q & 1))) ? 1 : 0;
    return sign | (((uint32_t)ef << 23) + q);                          // (a carry runs into the exponent, up to inf)
}

// G.711 expansion to the 16-bit value (wavio._g711_tables)
NQ_DEV int mulaw16(uint32_t code) {
    const int u = (int)(~code & 0xFFu);
    const int mag = ((((u & 0x0F) << 3) + 0x84) << ((u >> 4) & 7)) - 0x84;
    return (u & 0x80) ? -mag : mag;
}
NQ_DEV int alaw16(uint32_t code) {
    const int a = (int)((code ^ 0x55u) & 0xFFu);
    const int e = (a >> 4) & 7, m = a & 0x0F;
    const int mag = e == 0 ? (m << 4) + 8 : ((m << 4) + 0x108) << (e - 1);
    return (a & 0x80) ? mag : -mag;
}

struct Format {
    int container, enc;
    bool be;
};

// the float32 bits of the sample whose first byte sits at byte ``off`` of the staged range
NQ_DEV uint32_t sample_bits(const uint32_t* __restrict__ lds, int off, const Format& f) {
    const int w = off >> 2, sh = (off & 3) * 8;
    uint32_t v = lds[w];
    if (f.container == 8) {
        uint32_t lo = v, hi = lds[w + 1];                              // (8-byte samples are 4-byte aligned: off is a multiple of 8)
        if (f.be) { const uint32_t t = bswap32(lo); lo = bswap32(hi); hi = t; }
        return f64_to_f32_bits(lo, hi);
    }
    if (sh + f.container * 8 > 32) v = __funnelshift_r(v, lds[w + 1], sh);
    else v >>= sh;
    switch (f.container) {
    case 1:
        v &= 0xFFu;
        if (f.enc == NISQA_WAVENC_MULAW) return __float_as_uint((float)mulaw16(v) * (1.0f / 32768.0f));
        if (f.enc == NISQA_WAVENC_ALAW) return __float_as_uint((float)alaw16(v) * (1.0f / 32768.0f));
        return __float_as_uint(((float)(int)v - 128.0f) * (1.0f / 128.0f));
    case 2:
        v &= 0xFFFFu;
        if (f.be) v = bswap32(v) >> 16;
        return __float_as_uint((float)(int16_t)v * (1.0f / 32768.0f));
    case 3:
        v &= 0xFFFFFFu;
        if (f.be) v = bswap32(v) >> 8;
        return __float_as_uint((float)((int)(v << 8) >> 8) * (1.0f / 8388608.0f));
    default:
        if (f.be) v = bswap32(v);
        if (f.enc == NISQA_WAVENC_FLOAT) return v;                     // the bits as they are
        return __float_as_uint((float)(int)v * (1.0f / 2147483648.0f));      // one rounding: int32 -> float32, then a power of two
    }
}

__global__ __launch_bounds__(THREADS) void wav_decode_kernel(const unsigned char* __restrict__ raw, int64_t raw_bytes,
                                                             const nisqa_wav_clip* __restrict__ clips, int tiles_per_clip,
                                                             float* __restrict__ out) {
    __shared__ uint4 stage[SPANS];
    const int clip = blockIdx.x / tiles_per_clip, tile = blockIdx.x % tiles_per_clip;
    const nisqa_wav_clip c = clips[clip];
    const int64_t t0 = (int64_t)tile * TILE;
    if (t0 >= c.n_frames) return;                                      // (uniform: the whole workgroup leaves)
    const int ch = c.channels, cont = c.container;
    const int enc = c.encoding & ~NISQA_WAVENC_BIG_ENDIAN;
    // an entry the kernel cannot take is left alone (the binding refuses it on the host before the launch)
    const bool enc_ok = (enc == NISQA_WAVENC_PCM && (cont >= 1 && cont <= 4)) || (enc == NISQA_WAVENC_FLOAT && (cont == 4 || cont == 8)) ||
                        ((enc == NISQA_WAVENC_ALAW || enc == NISQA_WAVENC_MULAW) && cont == 1);
    if (!enc_ok || ch < 1 || ch > MAX_BLOCK || ch * cont > MAX_BLOCK || c.channel >= ch || c.channel < -1 || (c.channel < 0 && ch > 32) ||
        c.src_off < 0 || (c.src_off & 15) || c.dst_off < 0 || c.n_frames > (raw_bytes - c.src_off) / (ch * cont))
        return;
    const int blk = ch * cont;
    const Format fmt = {cont, enc, (c.encoding & NISQA_WAVENC_BIG_ENDIAN) != 0};
    const int64_t t1 = t0 + TILE < c.n_frames ? t0 + TILE : c.n_frames;
    const int per_pass = STAGE / blk < TILE ? STAGE / blk : TILE;
    const int pick = ch == 1 ? 0 : c.channel;                          // >= 0: one channel; -1: the mean
    const uint32_t* lds = reinterpret_cast<const uint32_t*>(stage);
    float* dst = out + c.dst_off;

    for (int64_t p0 = t0; p0 < t1; p0 += per_pass) {
        const int nf = t1 - p0 < per_pass ? (int)(t1 - p0) : per_pass;
        const int64_t b0 = c.src_off + p0 * blk, b1 = b0 + (int64_t)nf * blk;     // the pass's bytes in raw
        const int64_t a0 = b0 & ~(int64_t)15;
        const int n_spans = (int)((b1 - a0 + 15) >> 4);                 // <= SPANS - 1
        for (int s = threadIdx.x; s < n_spans; s += THREADS) {
            const int64_t at = a0 + (int64_t)s * 16;
            uint4 v;
            if (at + 16 <= raw_bytes) {
                v = *reinterpret_cast<const uint4*>(raw + at);
            } else {                                                   // the last span of a buffer without a tail pad
                uint32_t w[4] = {0, 0, 0, 0};
                for (int k = 0; k < 16 && at + k < raw_bytes; ++k) w[k >> 2] |= (uint32_t)raw[at + k] << ((k & 3) * 8);
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
            stage[s] = v;
        }
        __syncthreads();
        const int skew = (int)(b0 - a0);
        for (int i = threadIdx.x; i < nf; i += THREADS) {
            const int off = skew + i * blk;
            uint32_t bits;
            if (pick >= 0) {
                bits = sample_bits(lds, off + pick * cont, fmt);
            } else {
#pragma clang fp contract(off)
                // librosa.to_mono = np.mean(y, axis=0, dtype=float32) over a channel-contiguous row: numpy adds in order below eight
                // addends and through eight accumulators from eight on, then divides (an IEEE division: 1 / ch is not exact)
                float s;
                if (ch < 8) {
                    s = __uint_as_float(sample_bits(lds, off, fmt));
                    for (int k = 1; k < ch; ++k) s += __uint_as_float(sample_bits(lds, off + k * cont, fmt));
                } else {
                    float r[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) r[j] = __uint_as_float(sample_bits(lds, off + j * cont, fmt));
                    const int full = ch >> 3;
                    for (int k = 1; k < full; ++k) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) r[j] += __uint_as_float(sample_bits(lds, off + (8 * k + j) * cont, fmt));
                    }
                    s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
                    for (int k = 8 * full; k < ch; ++k) s += __uint_as_float(sample_bits(lds, off + k * cont, fmt));
                }
                // (the reduction starts from its identity: +0.0 + sum, so a sum of -0.0 comes out as +0.0)
                bits = __float_as_uint(__fdiv_rn(0.0f + s, (float)ch));
            }
            reinterpret_cast<uint32_t*>(dst)[p0 + i] = bits;
        }
        __syncthreads();                                               // the next pass overwrites the stage
    }
}

}  // namespace

extern "C" int nisqa_wav_decode(const void* raw, int64_t raw_bytes, const nisqa_wav_clip* clips, int32_t n_clips,
                                int64_t max_frames, float* out, void* stream) {
    if (!raw || !clips || !out || ((uintptr_t)raw & 15) || raw_bytes <= 0 || n_clips <= 0 || max_frames <= 0) return NISQA_ERR_ARG;
    const int64_t tiles = (max_frames + TILE - 1) / TILE;
    if (tiles * n_clips > 0x7FFFFFFF) return NISQA_ERR_ARG;
    NQ_LAUNCH_BEGIN();
    hipLaunchKernelGGL(wav_decode_kernel, dim3((unsigned)(tiles * n_clips)), dim3(THREADS), 0, (hipStream_t)stream,
                       (const unsigned char*)raw, raw_bytes, clips, (int)tiles, out);
    return NQ_LAUNCH_STATUS();
}
