// nisqa_flac_decode: FLAC streams already in HBM -- the frame regions nisqa_ingest_flac_read copied verbatim, with their frame
// tables -- to what the host path hands the network for the same files, bit for bit: int16 samples for mono 16-bit streams, otherwise
// the float32 mono of wavio.read_wav (value / 2^(bits - 1), ms_channel or the mean of the two channels).  The decoder is
// flac_frame.hpp, the same source the host indexer and the CPU test program compile.
//
// Three kernels on the caller's stream:
//   frames  one LANE per frame (Rice codes make a subframe serial; frames are independent): header, subframes, CRC-16, and the frame
//           must end where the table says the next one starts.  Samples go to an int32 workspace laid out [group of 64 frames]
//           [channel][sample][lane], so that the 64 lanes of a wave, which walk their frames in step, store to 64 neighbouring words.
//   finish  a workgroup per (group of 64 frames, 64 samples): transposes the tile through LDS, undoes left/side, right/side and
//           mid/side, writes the output coalesced and, for a stream whose STREAMINFO carries an MD5 and whose output is not already
//           the little-endian samples, the interleaved (bits + 7) / 8-byte samples the MD5 is defined over.
//   md5     one lane per clip (MD5 is serial per stream): digest of those bytes against STREAMINFO's.
// A check that fails sets bits in the clip's status word; nothing is papered over.  Every row of the frame table is validated against
// its clip before anything is loaded or stored through it, in every kernel.
#include "common.hpp"
#include "flac_frame.hpp"
#include "../../include/nisqa_hip.h"

namespace {

constexpr int LANES = 64;
constexpr int TILE = 64;                 // samples per finish workgroup
constexpr int FINISH_THREADS = 256;

struct Launch {
    const unsigned char* raw;
    int64_t raw_bytes;
    const nisqa_flac_clip* clips;
    int n_clips;
    const nisqa_flac_frame* frames;
    int n_rows, max_block, max_ch, out_i16;
    void* out;
    int64_t out_samples;
    int32_t* ws;                         // [groups][max_ch][max_block][64]
    int32_t* row_ca;                     // [groups * 64]: channel assignment of every decoded frame
    unsigned char* md5_buf;
    int64_t md5_bytes;
    int32_t* status;                     // [n_clips + 1]; the last word: a row that names no clip
};

// Row g against its clip: the frame's samples are [first, first + bs) of the clip's own output, its bytes [offset, end) of the clip's
// own region.  False: the row is not used for any load or store.
NQ_DEV bool row_ok(const Launch& L, int g, nisqa_flac_frame& row, nisqa_flac_clip& c, uint32_t& end, bool& last) {
    row = L.frames[g];
    if (row.clip < 0 || row.clip >= L.n_clips) return false;
    c = L.clips[row.clip];
    if (c.src_off < 0 || (c.src_off & 15) || c.src_bytes <= 0 || c.src_bytes >= ((int64_t)1 << 31) || c.src_off > L.raw_bytes - c.src_bytes) return false;
    if (c.block_size < 1 || c.block_size > L.max_block || c.channels < 1 || c.channels > L.max_ch || c.channels > 2) return false;
    if (c.bits < 4 || c.bits > 24 || c.channel < -1 || c.channel >= c.channels) return false;
    if (L.out_i16 && (c.bits != 16 || c.channels != 1)) return false;
    if (c.n_samples < 1 || c.n_samples >= ((int64_t)1 << 31) || c.dst_off < 0 || c.dst_off > L.out_samples - c.n_samples) return false;
    if (c.frame0 < 0 || c.n_frames < 1 || c.frame0 > L.n_rows - c.n_frames || g < c.frame0 || g >= c.frame0 + c.n_frames) return false;
    const int64_t first = (int64_t)(g - c.frame0) * c.block_size;
    if (first >= c.n_samples || row.first_sample != first) return false;
    const int64_t left = c.n_samples - first;
    if (row.block_size != (left < c.block_size ? (int)left : c.block_size)) return false;
    last = g == c.frame0 + c.n_frames - 1;
    if (last != (left <= c.block_size)) return false;
    if (c.md5_set && !L.out_i16) {
        const int64_t need = c.n_samples * c.channels * ((c.bits + 7) / 8);
        if (c.md5_off < 0 || (c.md5_off & 3) || c.md5_off > L.md5_bytes - need) return false;
    }
    if (row.offset < 0 || row.offset >= c.src_bytes) return false;
    int64_t e = c.src_bytes;
    if (!last) {
        const nisqa_flac_frame next = L.frames[g + 1];
        if (next.clip != row.clip) return false;
        e = next.offset;
    }
    if (e <= row.offset || e > c.src_bytes) return false;
    end = (uint32_t)e;
    return true;
}

struct WsOut {
    int32_t* base;                       // this lane's column of its group's tile
    int32_t* cur;
    int bs, max_block;
    __device__ void channel(int c) { cur = base + (size_t)c * max_block * LANES; }
    __device__ void put(int i, int32_t v) {
        if ((unsigned)i < (unsigned)bs) cur[(size_t)i * LANES] = v;
    }
};

__global__ __launch_bounds__(LANES) void flac_frames_kernel(Launch L) {
    __shared__ nqff::Tables tab;
    for (int i = threadIdx.x; i < 256; i += LANES) nqff::table_entry(tab, i);
    __syncthreads();
    const int g = blockIdx.x * LANES + threadIdx.x;
    if (g >= L.n_rows) return;
    nisqa_flac_frame row;
    nisqa_flac_clip c;
    uint32_t end;
    bool last;
    if (!row_ok(L, g, row, c, end, last)) {
        const int who = row.clip >= 0 && row.clip < L.n_clips ? row.clip : L.n_clips;
        atomicOr(&L.status[who], NISQA_FLAC_BAD_TABLE);
        return;
    }
    WsOut out;
    out.base = L.ws + (size_t)blockIdx.x * L.max_ch * L.max_block * LANES + threadIdx.x;
    out.cur = out.base;
    out.bs = row.block_size;
    out.max_block = L.max_block;
    int ca = 0;
    // a frame behind which the file goes on (tags some writers append) may end before the region does; every other frame ends
    // exactly where the next one starts
    const int rc = nqff::frame(tab, L.raw + c.src_off + row.offset, end - (uint32_t)row.offset, !last, row.block_size, c.bits, c.channels, out, &ca);
    L.row_ca[g] = ca;
    if (rc != nqff::FRAME_OK) atomicOr(&L.status[row.clip], 1 << rc);
}

__global__ __launch_bounds__(FINISH_THREADS) void flac_finish_kernel(Launch L) {
    __shared__ int32_t tile[2][TILE][LANES + 1];
    const int grp = blockIdx.x, i0 = blockIdx.y * TILE;
    const int lo = threadIdx.x & 63, hi = threadIdx.x >> 6;
    const int32_t* src = L.ws + (size_t)grp * L.max_ch * L.max_block * LANES;
    for (int c = 0; c < L.max_ch && c < 2; ++c)
        for (int r = 0; r < TILE / 4; ++r) {
            const int il = r * 4 + hi;
            if (i0 + il < L.max_block) tile[c][il][lo] = src[((size_t)c * L.max_block + i0 + il) * LANES + lo];
        }
    __syncthreads();
    for (int r = 0; r < TILE / 4; ++r) {
        const int fl = r * 4 + hi, g = grp * LANES + fl, i = i0 + lo;
        if (g >= L.n_rows) break;                                      // (uniform per wave: fl does not depend on the lane)
        nisqa_flac_frame row;
        nisqa_flac_clip c;
        uint32_t end;
        bool last;
        if (!row_ok(L, g, row, c, end, last) || i >= row.block_size) continue;
        int32_t a = tile[0][lo][fl], b = 0;
        if (c.channels == 2) {
            b = tile[1][lo][fl];
            nqff::undo_stereo(L.row_ca[g], a, b);
        }
        const int64_t s = (int64_t)row.first_sample + i;
        if (L.out_i16) {
            reinterpret_cast<int16_t*>(L.out)[c.dst_off + s] = (int16_t)a;
            continue;
        }
        {
#pragma clang fp contract(off)
        const float scale = __uint_as_float((uint32_t)(127 - (c.bits - 1)) << 23);       // 2^-(bits - 1): the product is exact
        const float fa = (float)a * scale, fb = (float)b * scale;
        float y = fa;
        if (c.channels == 2) y = c.channel == 0 ? fa : c.channel == 1 ? fb : __fdiv_rn(0.0f + (fa + fb), 2.0f);   // (numpy's mean: the sum from +0.0, then a division)
        reinterpret_cast<float*>(L.out)[c.dst_off + s] = y;
        if (c.md5_set) {
            const int bytes = (c.bits + 7) / 8;
            unsigned char* w = L.md5_buf + c.md5_off + s * c.channels * bytes;
            for (int k = 0; k < bytes; ++k) w[k] = (unsigned char)((uint32_t)a >> (8 * k));
            if (c.channels == 2)
                for (int k = 0; k < bytes; ++k) w[bytes + k] = (unsigned char)((uint32_t)b >> (8 * k));
        }
        }
    }
}

// ---- MD5 (RFC 1321) ----
NQ_DEV uint32_t rol(uint32_t x, int c) { return (x << c) | (x >> (32 - c)); }
NQ_DEV void md5_block(uint32_t (&s)[4], const uint32_t (&m)[16]) {
    uint32_t a = s[0], b = s[1], c = s[2], d = s[3];
#define NQ_F(x, y, z) ((z) ^ ((x) & ((y) ^ (z))))
#define NQ_G(x, y, z) ((y) ^ ((z) & ((x) ^ (y))))
#define NQ_H(x, y, z) ((x) ^ (y) ^ (z))
#define NQ_I(x, y, z) ((y) ^ ((x) | ~(z)))
#define NQ_S(f, a, b, c, d, g, k, r) a = b + rol(a + f(b, c, d) + (k) + m[g], r)
    NQ_S(NQ_F, a, b, c, d, 0, 0xd76aa478u, 7);   NQ_S(NQ_F, d, a, b, c, 1, 0xe8c7b756u, 12);
    NQ_S(NQ_F, c, d, a, b, 2, 0x242070dbu, 17);  NQ_S(NQ_F, b, c, d, a, 3, 0xc1bdceeeu, 22);
    NQ_S(NQ_F, a, b, c, d, 4, 0xf57c0fafu, 7);   NQ_S(NQ_F, d, a, b, c, 5, 0x4787c62au, 12);
    NQ_S(NQ_F, c, d, a, b, 6, 0xa8304613u, 17);  NQ_S(NQ_F, b, c, d, a, 7, 0xfd469501u, 22);
    NQ_S(NQ_F, a, b, c, d, 8, 0x698098d8u, 7);   NQ_S(NQ_F, d, a, b, c, 9, 0x8b44f7afu, 12);
    NQ_S(NQ_F, c, d, a, b, 10, 0xffff5bb1u, 17); NQ_S(NQ_F, b, c, d, a, 11, 0x895cd7beu, 22);
    NQ_S(NQ_F, a, b, c, d, 12, 0x6b901122u, 7);  NQ_S(NQ_F, d, a, b, c, 13, 0xfd987193u, 12);
    NQ_S(NQ_F, c, d, a, b, 14, 0xa679438eu, 17); NQ_S(NQ_F, b, c, d, a, 15, 0x49b40821u, 22);
    NQ_S(NQ_G, a, b, c, d, 1, 0xf61e2562u, 5);   NQ_S(NQ_G, d, a, b, c, 6, 0xc040b340u, 9);
    NQ_S(NQ_G, c, d, a, b, 11, 0x265e5a51u, 14); NQ_S(NQ_G, b, c, d, a, 0, 0xe9b6c7aau, 20);
    NQ_S(NQ_G, a, b, c, d, 5, 0xd62f105du, 5);   NQ_S(NQ_G, d, a, b, c, 10, 0x02441453u, 9);
    NQ_S(NQ_G, c, d, a, b, 15, 0xd8a1e681u, 14); NQ_S(NQ_G, b, c, d, a, 4, 0xe7d3fbc8u, 20);
    NQ_S(NQ_G, a, b, c, d, 9, 0x21e1cde6u, 5);   NQ_S(NQ_G, d, a, b, c, 14, 0xc33707d6u, 9);
    NQ_S(NQ_G, c, d, a, b, 3, 0xf4d50d87u, 14);  NQ_S(NQ_G, b, c, d, a, 8, 0x455a14edu, 20);
    NQ_S(NQ_G, a, b, c, d, 13, 0xa9e3e905u, 5);  NQ_S(NQ_G, d, a, b, c, 2, 0xfcefa3f8u, 9);
    NQ_S(NQ_G, c, d, a, b, 7, 0x676f02d9u, 14);  NQ_S(NQ_G, b, c, d, a, 12, 0x8d2a4c8au, 20);
    NQ_S(NQ_H, a, b, c, d, 5, 0xfffa3942u, 4);   NQ_S(NQ_H, d, a, b, c, 8, 0x8771f681u, 11);
    NQ_S(NQ_H, c, d, a, b, 11, 0x6d9d6122u, 16); NQ_S(NQ_H, b, c, d, a, 14, 0xfde5380cu, 23);
    NQ_S(NQ_H, a, b, c, d, 1, 0xa4beea44u, 4);   NQ_S(NQ_H, d, a, b, c, 4, 0x4bdecfa9u, 11);
    NQ_S(NQ_H, c, d, a, b, 7, 0xf6bb4b60u, 16);  NQ_S(NQ_H, b, c, d, a, 10, 0xbebfbc70u, 23);
    NQ_S(NQ_H, a, b, c, d, 13, 0x289b7ec6u, 4);  NQ_S(NQ_H, d, a, b, c, 0, 0xeaa127fau, 11);
    NQ_S(NQ_H, c, d, a, b, 3, 0xd4ef3085u, 16);  NQ_S(NQ_H, b, c, d, a, 6, 0x04881d05u, 23);
    NQ_S(NQ_H, a, b, c, d, 9, 0xd9d4d039u, 4);   NQ_S(NQ_H, d, a, b, c, 12, 0xe6db99e5u, 11);
    NQ_S(NQ_H, c, d, a, b, 15, 0x1fa27cf8u, 16); NQ_S(NQ_H, b, c, d, a, 2, 0xc4ac5665u, 23);
    NQ_S(NQ_I, a, b, c, d, 0, 0xf4292244u, 6);   NQ_S(NQ_I, d, a, b, c, 7, 0x432aff97u, 10);
    NQ_S(NQ_I, c, d, a, b, 14, 0xab9423a7u, 15); NQ_S(NQ_I, b, c, d, a, 5, 0xfc93a039u, 21);
    NQ_S(NQ_I, a, b, c, d, 12, 0x655b59c3u, 6);  NQ_S(NQ_I, d, a, b, c, 3, 0x8f0ccc92u, 10);
    NQ_S(NQ_I, c, d, a, b, 10, 0xffeff47du, 15); NQ_S(NQ_I, b, c, d, a, 1, 0x85845dd1u, 21);
    NQ_S(NQ_I, a, b, c, d, 8, 0x6fa87e4fu, 6);   NQ_S(NQ_I, d, a, b, c, 15, 0xfe2ce6e0u, 10);
    NQ_S(NQ_I, c, d, a, b, 6, 0xa3014314u, 15);  NQ_S(NQ_I, b, c, d, a, 13, 0x4e0811a1u, 21);
    NQ_S(NQ_I, a, b, c, d, 4, 0xf7537e82u, 6);   NQ_S(NQ_I, d, a, b, c, 11, 0xbd3af235u, 10);
    NQ_S(NQ_I, c, d, a, b, 2, 0x2ad7d2bbu, 15);  NQ_S(NQ_I, b, c, d, a, 9, 0xeb86d391u, 21);
#undef NQ_S
#undef NQ_F
#undef NQ_G
#undef NQ_H
#undef NQ_I
    s[0] += a; s[1] += b; s[2] += c; s[3] += d;
}

// the 16 little-endian words of the stream from byte 64 * blk on: aligned dword loads (never a dword without a byte of the stream in
// it) shifted into place
NQ_DEV void md5_words(const uint32_t* __restrict__ al, int sh, int64_t n_al, int64_t blk, uint32_t (&m)[16]) {
    uint32_t a[17];
#pragma unroll
    for (int j = 0; j < 17; ++j) {
        const int64_t i = blk * 16 + j;
        a[j] = i < n_al ? al[i] : 0u;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) m[j] = sh ? __funnelshift_r(a[j], a[j + 1], sh) : a[j];
}

__global__ __launch_bounds__(LANES) void flac_md5_kernel(Launch L) {
    const int k = blockIdx.x * LANES + threadIdx.x;
    if (k >= L.n_clips) return;
    const nisqa_flac_clip c = L.clips[k];
    if (!c.md5_set) return;
    // (the clip's fields as the other kernels accepted them: a clip they refused is flagged already and is not read here)
    if (c.bits < 4 || c.bits > 24 || c.channels < 1 || c.channels > 2 || c.n_samples < 1 || c.n_samples >= ((int64_t)1 << 31)) return;
    const int64_t len = c.n_samples * c.channels * ((c.bits + 7) / 8);
    const unsigned char* p;
    if (L.out_i16) {
        if (c.bits != 16 || c.channels != 1 || c.dst_off < 0 || c.dst_off > L.out_samples - c.n_samples) return;
        p = reinterpret_cast<const unsigned char*>(L.out) + 2 * c.dst_off;
    } else {
        if (c.md5_off < 0 || (c.md5_off & 3) || c.md5_off > L.md5_bytes - len) return;
        p = L.md5_buf + c.md5_off;
    }
    const int mis = (int)((uintptr_t)p & 3);
    const uint32_t* al = reinterpret_cast<const uint32_t*>(p - mis);
    const int64_t n_al = (mis + len + 3) >> 2;
    uint32_t s[4] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u};
    uint32_t m[16], nx[16];
    const int64_t full = len >> 6;
    md5_words(al, mis * 8, n_al, 0, m);
    for (int64_t b = 0; b < full; ++b) {                               // the next block's loads fly under this block's 64 steps
        md5_words(al, mis * 8, n_al, b + 1, nx);
        md5_block(s, m);
#pragma unroll
        for (int j = 0; j < 16; ++j) m[j] = nx[j];
    }
    const int r = (int)(len & 63);                                     // (m: the words of the last, partial block)
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int have = r - 4 * j;                                    // bytes of word j that belong to the stream
        if (have <= 0) m[j] = 0;
        else if (have < 4) m[j] &= (1u << (8 * have)) - 1;
        if (j == (r >> 2)) m[j] |= 0x80u << (8 * (r & 3));
    }
    const uint64_t nbits = (uint64_t)len * 8;
    if (r >= 56) {
        md5_block(s, m);
#pragma unroll
        for (int j = 0; j < 16; ++j) m[j] = 0;
    }
    m[14] = (uint32_t)nbits;
    m[15] = (uint32_t)(nbits >> 32);
    md5_block(s, m);
    bool same = true;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t want = (uint32_t)c.md5[4 * j] | ((uint32_t)c.md5[4 * j + 1] << 8) | ((uint32_t)c.md5[4 * j + 2] << 16) | ((uint32_t)c.md5[4 * j + 3] << 24);
        same = same && want == s[j];
    }
    if (!same) atomicOr(&L.status[k], NISQA_FLAC_BAD_MD5);
}

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

extern "C" size_t nisqa_flac_workspace_bytes(int32_t n_frames, int32_t max_block, int32_t max_channels, int64_t md5_bytes) {
    if (n_frames <= 0 || max_block <= 0 || max_block > 65535 || max_channels < 1 || max_channels > 2 || md5_bytes < 0) return 0;
    const size_t groups = ((size_t)n_frames + LANES - 1) / LANES;
    return align256(groups * (size_t)max_channels * (size_t)max_block * LANES * 4) + align256(groups * LANES * 4) + align256((size_t)md5_bytes);
}

extern "C" int nisqa_flac_decode(const void* raw, int64_t raw_bytes, const nisqa_flac_clip* clips, int32_t n_clips,
                                 const nisqa_flac_frame* frames, int32_t n_frames, int32_t max_block, int32_t max_channels,
                                 int32_t out_i16, void* out, int64_t out_samples, int64_t md5_bytes, void* ws, size_t ws_bytes,
                                 int32_t* status, void* stream) {
    if (!raw || !clips || !frames || !out || !ws || !status || ((uintptr_t)raw & 15) || ((uintptr_t)frames & 3) || ((uintptr_t)out & 3) ||
        ((uintptr_t)ws & 255) || raw_bytes <= 0 || n_clips <= 0 || n_frames <= 0 || out_samples <= 0)
        return NISQA_ERR_ARG;
    const size_t need = nisqa_flac_workspace_bytes(n_frames, max_block, max_channels, md5_bytes);
    if (need == 0) return NISQA_ERR_ARG;
    if (ws_bytes < need) return NISQA_ERR_WORKSPACE;
    const size_t groups = ((size_t)n_frames + LANES - 1) / LANES;
    const int tiles = (max_block + TILE - 1) / TILE;
    if (groups > 0x7FFFFFFF || tiles > 65535) return NISQA_ERR_ARG;
    Launch L;
    L.raw = (const unsigned char*)raw;
    L.raw_bytes = raw_bytes;
    L.clips = clips;
    L.n_clips = n_clips;
    L.frames = frames;
    L.n_rows = n_frames;
    L.max_block = max_block;
    L.max_ch = max_channels;
    L.out_i16 = out_i16 ? 1 : 0;
    L.out = out;
    L.out_samples = out_samples;
    L.ws = (int32_t*)ws;
    L.row_ca = (int32_t*)((char*)ws + align256(groups * (size_t)max_channels * (size_t)max_block * LANES * 4));
    L.md5_buf = (unsigned char*)L.row_ca + align256(groups * LANES * 4);
    L.md5_bytes = md5_bytes;
    L.status = status;
    NQ_LAUNCH_BEGIN();
    hipLaunchKernelGGL(flac_frames_kernel, dim3((unsigned)groups), dim3(LANES), 0, (hipStream_t)stream, L);
    hipLaunchKernelGGL(flac_finish_kernel, dim3((unsigned)groups, (unsigned)tiles), dim3(FINISH_THREADS), 0, (hipStream_t)stream, L);
    hipLaunchKernelGGL(flac_md5_kernel, dim3((unsigned)((n_clips + LANES - 1) / LANES)), dim3(LANES), 0, (hipStream_t)stream, L);
    return NQ_LAUNCH_STATUS();
}
