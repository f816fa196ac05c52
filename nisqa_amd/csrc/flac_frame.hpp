// One FLAC frame decoder for host and device: the frame-level half of flac.hpp (nqflac::detail), restated so that ONE source serves
// the HIP kernel (flac_dev.hip: one lane per frame), the host indexer of libnisqa_ingest.so (ingest.cpp: header parse + CRC-8 only)
// and a CPU-compiled test program.  Same published format description as flac.hpp (xiph.org "FLAC format"); the arithmetic mirrors
// nqflac::detail operation for operation, wrap-arounds included, so a valid stream gives the same integers -- what differs is the
// shape: a frame is decoded from a bounded span [p, p + n) it cannot read outside of, samples leave through a sink (`Out`: put(i, v)
// for sample i of the channel chosen with channel(c)) the moment they are restored, and the predictor's history and coefficients
// live in statically indexed arrays (registers on the GPU; a runtime-indexed array would go to scratch memory there).
//
// Memory rules (a damaged stream must never become a GPU fault): Reader loads only bytes below `n`, reads past the end deliver zeros
// and set `over`; every loop bound is a range-checked header field; the unary scan ends with the span; a sink sees only indices in
// [0, block size).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define NQFF_HD __host__ __device__ inline
#else
#define NQFF_HD inline
#endif
#if defined(__clang__)
#define NQFF_UNROLL _Pragma("unroll")
#else
#define NQFF_UNROLL
#endif

namespace nqff {

// ---- CRC-8 (x^8 + x^2 + x + 1) of a frame header and CRC-16 (x^16 + x^15 + x^2 + 1) of a frame; MSB first, initial value 0 ----
struct Tables {
    uint8_t c8[256];
    uint16_t c16[256];
};
NQFF_HD void table_entry(Tables& t, int i) {             // (a kernel fills the tables in LDS, one entry per thread)
    uint8_t a = (uint8_t)i;
    uint16_t b = (uint16_t)(i << 8);
    for (int k = 0; k < 8; ++k) {
        a = (uint8_t)((a & 0x80) ? (a << 1) ^ 0x07 : a << 1);
        b = (uint16_t)((b & 0x8000) ? (b << 1) ^ 0x8005 : b << 1);
    }
    t.c8[i] = a;
    t.c16[i] = b;
}
NQFF_HD void fill_tables(Tables& t) {
    for (int i = 0; i < 256; ++i) table_entry(t, i);
}
NQFF_HD uint8_t crc8(const Tables& t, const uint8_t* p, uint32_t n) {
    uint8_t c = 0;
    for (uint32_t i = 0; i < n; ++i) c = t.c8[c ^ p[i]];
    return c;
}
NQFF_HD uint16_t crc16(const Tables& t, const uint8_t* p, uint32_t n) {
    uint16_t c = 0;
    for (uint32_t i = 0; i < n; ++i) c = (uint16_t)((c << 8) ^ t.c16[(c >> 8) ^ p[i]]);
    return c;
}

// ---- frame header ----
struct Header {
    int len;            // bytes, CRC-8 included
    int bs;             // block size
    int sr_code, ca;    // sample-rate code, channel assignment (0-7 independent channels, 8 left/side, 9 right/side, 10 mid/side)
    int bits;           // 8 / 12 / 16 / 20 / 24; 0 = "as STREAMINFO says"; -1 = reserved code
    int channels;       // -1 = reserved assignment
    int variable;       // blocking-strategy bit: 1 = the number below is the first SAMPLE of the frame
    uint64_t number;    // the UTF-8-coded frame / sample number
};
enum { HDR_OK = 0, HDR_BAD = 1, HDR_SHORT = 2 };

// The header at h (avail bytes readable): HDR_OK, HDR_BAD (no sync, a reserved code, CRC-8 mismatch) or HDR_SHORT (the span ends
// inside it).  Accepts exactly what nqflac::decode accepts.
NQFF_HD int parse_header(const Tables& t, const uint8_t* h, uint32_t avail, Header& o) {
    if (avail < 6) return HDR_SHORT;
    if (h[0] != 0xFF || (h[1] & 0xFE) != 0xF8 || (h[3] & 1)) return HDR_BAD;
    const int bs_code = h[2] >> 4, ss = (h[3] >> 1) & 7;
    o.variable = h[1] & 1;
    o.sr_code = h[2] & 15;
    o.ca = h[3] >> 4;
    uint32_t q = 4;
    {
        const uint8_t f = h[q];
        int extra = 0;
        uint64_t v = f;
        if (f & 0x80) {
            int ones = 0;
            while (ones < 8 && (f & (0x80 >> ones))) ++ones;
            if (ones < 2 || ones > 7) return HDR_BAD;
            extra = ones - 1;
            v = f & (0x7Fu >> ones);
        }
        if (q + 1 + extra + 5 > avail) return HDR_SHORT;
        for (int i = 1; i <= extra; ++i) {
            if ((h[q + i] & 0xC0) != 0x80) return HDR_BAD;
            v = (v << 6) | (h[q + i] & 0x3Fu);
        }
        o.number = v;
        q += 1 + extra;
    }
    if (bs_code == 0) return HDR_BAD;                    // (q + 4 <= avail from here on: block size and sample rate take at most 4)
    else if (bs_code == 1) o.bs = 192;
    else if (bs_code <= 5) o.bs = 576 << (bs_code - 2);
    else if (bs_code == 6) { o.bs = h[q] + 1; q += 1; }
    else if (bs_code == 7) { o.bs = ((h[q] << 8) | h[q + 1]) + 1; q += 2; }
    else o.bs = 256 << (bs_code - 8);
    if (o.sr_code == 12) q += 1;
    else if (o.sr_code == 13 || o.sr_code == 14) q += 2;
    else if (o.sr_code == 15) return HDR_BAD;
    if (q + 1 > avail) return HDR_SHORT;
    if (crc8(t, h, q) != h[q]) return HDR_BAD;
    o.len = (int)q + 1;
    o.bits = ss == 0 ? 0 : ss == 1 ? 8 : ss == 2 ? 12 : ss == 4 ? 16 : ss == 5 ? 20 : ss == 6 ? 24 : -1;
    o.channels = o.ca < 8 ? o.ca + 1 : (o.ca <= 10 ? 2 : -1);
    return HDR_OK;
}

// ---- bit reader over [p, p + n), most-significant bit first; reads past the end deliver zeros and set `over` ----
struct Reader {
    const uint8_t* p;
    uint32_t n, byte;
    uint64_t acc;
    int cnt;
    bool over;
    NQFF_HD void init(const uint8_t* d, uint32_t len) { p = d; n = len; byte = 0; acc = 0; cnt = 0; over = false; }
    NQFF_HD void refill() {
        if (byte + 8 <= n) {                             // away from the end: four bytes at once keep >= 32 bits in the window
            if (cnt <= 32) {
                const uint32_t w = ((uint32_t)p[byte] << 24) | ((uint32_t)p[byte + 1] << 16) | ((uint32_t)p[byte + 2] << 8) | p[byte + 3];
                acc |= (uint64_t)w << (32 - cnt);
                byte += 4;
                cnt += 32;
            }
            return;
        }
        while (cnt <= 56) {
            uint64_t v = 0;
            if (byte < n) v = p[byte];
            else if (byte >= n + 8) over = true;
            ++byte;
            acc |= v << (56 - cnt);
            cnt += 8;
        }
    }
    NQFF_HD uint32_t get(int k) {                        // 0 <= k <= 32
        if (k == 0) return 0;
        refill();
        const uint32_t v = (uint32_t)(acc >> (64 - k));
        acc <<= k;
        cnt -= k;
        return v;
    }
    NQFF_HD int32_t gets(int k) {                        // two's complement field of k bits, 1 <= k <= 32
        const uint32_t v = get(k);
        return k >= 32 ? (int32_t)v : (int32_t)(v << (32 - k)) >> (32 - k);
    }
    NQFF_HD uint32_t unary() {                           // zeros before the next 1 bit; a run that reaches the span's end sets `over`
        uint32_t q = 0;
        for (;;) {
            refill();
            if (acc == 0) {
                q += (uint32_t)cnt;
                cnt = 0;
                if (over || q > (1u << 26)) { over = true; return 0; }
                continue;
            }
            const int z = __builtin_clzll(acc);
            q += (uint32_t)z;
            acc <<= z;                                   // (two steps: z + 1 may be 64)
            acc <<= 1;
            cnt -= z + 1;
            return q;
        }
    }
    NQFF_HD void align() { const int k = cnt & 7; acc <<= k; cnt -= k; }
    NQFF_HD uint32_t byte_pos() const { return byte - (uint32_t)(cnt >> 3); }      // after align()
    NQFF_HD bool bad() const { return over || byte_pos() > n; }
};

// ---- predictors: take the residual of sample i, restore the sample, remember it, hand it (shifted by the wasted bits) to the sink ----
template <class Out>
struct Fixed {
    Out& out;
    int order, wasted;
    int32_t h0, h1, h2, h3;                              // the last four samples, h0 the newest
    NQFF_HD Fixed(Out& o, int ord, int w) : out(o), order(ord), wasted(w), h0(0), h1(0), h2(0), h3(0) {}
    NQFF_HD void keep(int i, int32_t v) {
        h3 = h2; h2 = h1; h1 = h0; h0 = v;
        out.put(i, (int32_t)((uint32_t)v << wasted));
    }
    NQFF_HD void put(int i, int32_t r) {
        int32_t v = r;
        switch (order) {
            case 1: v = (int32_t)(uint32_t)((int64_t)r + h0); break;
            case 2: v = (int32_t)(uint32_t)((int64_t)r + 2 * (int64_t)h0 - h1); break;
            case 3: v = (int32_t)(uint32_t)((int64_t)r + 3 * (int64_t)h0 - 3 * (int64_t)h1 + h2); break;
            case 4: v = (int32_t)(uint32_t)((int64_t)r + 4 * (int64_t)h0 - 6 * (int64_t)h1 + 4 * (int64_t)h2 - h3); break;
            default: break;
        }
        keep(i, v);
    }
};

template <class Out, int N>                              // orders 1..N; coefficients beyond the order are zero
struct Lpc {
    Out& out;
    int wasted, shift;
    bool wide;                                           // the 64-bit restore (a partial sum may not fit 32 bits)
    int32_t coef[N], h[N];                               // h[j] = sample i - 1 - j
    NQFF_HD Lpc(Out& o, int w) : out(o), wasted(w), shift(0), wide(false) {
        NQFF_UNROLL
        for (int j = 0; j < N; ++j) { coef[j] = 0; h[j] = 0; }
    }
    NQFF_HD void set_coef(int j, int32_t c) {            // (a select per slot: no runtime index into the array)
        NQFF_UNROLL
        for (int k = 0; k < N; ++k) coef[k] = k == j ? c : coef[k];
    }
    NQFF_HD void keep(int i, int32_t v) {
        NQFF_UNROLL
        for (int k = N - 1; k > 0; --k) h[k] = h[k - 1];
        h[0] = v;
        out.put(i, (int32_t)((uint32_t)v << wasted));
    }
    NQFF_HD void put(int i, int32_t r) {
        int32_t v;
        if (wide) {
            int64_t acc = 0;
            NQFF_UNROLL
            for (int j = 0; j < N; ++j) acc += (int64_t)coef[j] * h[j];
            v = (int32_t)(uint32_t)((int64_t)r + (acc >> shift));
        } else {
            uint32_t acc = 0;                            // (unsigned: a damaged stream may wrap, a valid one cannot)
            NQFF_UNROLL
            for (int j = 0; j < N; ++j) acc += (uint32_t)coef[j] * (uint32_t)h[j];
            v = (int32_t)((uint32_t)r + (uint32_t)((int32_t)acc >> shift));
        }
        keep(i, v);
    }
};

// ---- partitioned Rice residual of samples [order, bs) -> pr.put(i, residual) ----
template <class Pred>
NQFF_HD bool residual(Reader& br, int bs, int order, Pred& pr) {
    const uint32_t method = br.get(2);
    if (method > 1) return false;
    const int pbits = method ? 5 : 4;
    const uint32_t esc = (1u << pbits) - 1;
    const int porder = (int)br.get(4);
    const int parts = 1 << porder;
    if (porder > 0 && (bs & (parts - 1))) return false;
    const int per = bs >> porder;
    if (per < order && porder > 0) return false;
    if (bs < order) return false;
    int i = order;
    for (int p = 0; p < parts; ++p) {
        const int cnt = per - (p == 0 ? order : 0);
        if (cnt < 0) return false;
        const uint32_t k = br.get(pbits);
        if (k == esc) {
            const int nb = (int)br.get(5);
            for (int j = 0; j < cnt; ++j) pr.put(i++, nb ? br.gets(nb) : 0);
        } else {
            for (int j = 0; j < cnt; ++j) {
                br.refill();
                uint32_t u;
                const int z = br.acc ? __builtin_clzll(br.acc) : 64;
                if (z + 1 + (int)k <= br.cnt && z + 1 + (int)k < 64) {      // quotient, stop bit and remainder are all in the window
                    const uint64_t rest = br.acc << (z + 1);
                    u = ((uint32_t)z << k) | (k ? (uint32_t)(rest >> (64 - k)) : 0u);
                    br.acc = rest << k;
                    br.cnt -= z + 1 + (int)k;
                } else {
                    const uint32_t q = br.unary();
                    u = (q << k) | br.get((int)k);
                }
                pr.put(i++, (int32_t)(u >> 1) ^ -(int32_t)(u & 1));
            }
        }
        if (br.over) return false;
    }
    return i == bs;
}

template <class Out, int N>
NQFF_HD bool lpc_subframe(Reader& br, Out& out, int bs, int b, int order, int wasted) {
    Lpc<Out, N> pr(out, wasted);
    for (int i = 0; i < order; ++i) pr.keep(i, br.gets(b));
    const int prec = (int)br.get(4) + 1;
    if (prec == 16) return false;
    const int shift = br.gets(5);
    if (shift < 0) return false;
    for (int j = 0; j < order; ++j) pr.set_coef(j, br.gets(prec));
    int lg = 0;
    while ((1 << lg) < order) ++lg;
    pr.shift = shift;
    pr.wide = !(b + prec + lg <= 32);                    // (what libFLAC's 32-bit restore assumes too)
    return residual(br, bs, order, pr);
}

// One subframe of `bs` samples, `bits` wide (a side channel: one more than the stream's) -> out.put(i, sample), i in [0, bs).
template <class Out>
NQFF_HD bool subframe(Reader& br, Out& out, int bs, int bits) {
    if (br.get(1)) return false;
    const int type = (int)br.get(6);
    int wasted = 0;
    if (br.get(1)) wasted = (int)br.unary() + 1;
    const int b = bits - wasted;
    if (b < 1 || b > 32) return false;
    if (type == 0) {
        const int32_t v = (int32_t)((uint32_t)br.gets(b) << wasted);
        for (int i = 0; i < bs; ++i) out.put(i, v);
    } else if (type == 1) {
        for (int i = 0; i < bs; ++i) out.put(i, (int32_t)((uint32_t)br.gets(b) << wasted));
    } else if (type >= 8 && type <= 12) {
        const int order = type - 8;
        if (order > bs) return false;
        Fixed<Out> pr(out, order, wasted);
        for (int i = 0; i < order; ++i) pr.keep(i, br.gets(b));
        if (!residual(br, bs, order, pr)) return false;
    } else if (type >= 32) {
        const int order = (type & 31) + 1;
        if (order > bs) return false;
        const bool ok = order <= 8 ? lpc_subframe<Out, 8>(br, out, bs, b, order, wasted)
                      : order <= 12 ? lpc_subframe<Out, 12>(br, out, bs, b, order, wasted)
                                    : lpc_subframe<Out, 32>(br, out, bs, b, order, wasted);
        if (!ok) return false;
    } else {
        return false;                                    // reserved subframe types
    }
    return !br.over;
}

enum { FRAME_OK = 0, FRAME_HEADER = 1, FRAME_FORMAT = 2, FRAME_SUBFRAME = 3, FRAME_OVERRUN = 4, FRAME_CRC16 = 5, FRAME_END = 6 };

// The frame in the span [p, p + n): header, every channel's subframe into `out`, padding, CRC-16.  The frame must carry `bs`
// samples of `ch` channels, `bits` wide, and end at the span's end (exact_end) or not behind it.  *ca = its channel assignment
// (the caller undoes left/side, right/side, mid/side).  FRAME_OK or the first check that failed.
template <class Out>
NQFF_HD int frame(const Tables& t, const uint8_t* p, uint32_t n, bool exact_end, int bs, int bits, int ch, Out& out, int* ca) {
    Header h;
    if (parse_header(t, p, n, h) != HDR_OK) return FRAME_HEADER;
    const int fbits = h.bits == 0 ? bits : h.bits;
    if (fbits != bits || h.channels != ch || h.bs != bs) return FRAME_FORMAT;
    *ca = h.ca;
    Reader br;
    br.init(p + h.len, n - (uint32_t)h.len);
    for (int c = 0; c < ch; ++c) {
        const bool side = (h.ca == 8 && c == 1) || (h.ca == 9 && c == 0) || (h.ca == 10 && c == 1);
        out.channel(c);
        if (!subframe(br, out, bs, fbits + (side ? 1 : 0))) return br.over ? FRAME_OVERRUN : FRAME_SUBFRAME;
    }
    br.align();
    if (br.bad()) return FRAME_OVERRUN;
    const uint32_t body = (uint32_t)h.len + br.byte_pos();
    if (body + 2 > n) return FRAME_OVERRUN;
    if (crc16(t, p, body) != (uint16_t)((p[body] << 8) | p[body + 1])) return FRAME_CRC16;
    if (exact_end ? body + 2 != n : body + 2 > n) return FRAME_END;
    return FRAME_OK;
}

// Undo the stereo decorrelation of one sample pair (a = channel 0, b = channel 1 as decoded), as nqflac::decode does.
NQFF_HD void undo_stereo(int ca, int32_t& a, int32_t& b) {
    if (ca == 8) b = (int32_t)((uint32_t)a - (uint32_t)b);
    else if (ca == 9) a = (int32_t)((uint32_t)a + (uint32_t)b);
    else if (ca == 10) {
        const int32_t sd = b;
        const int32_t m = (int32_t)(((uint32_t)a << 1) | (uint32_t)(sd & 1));
        a = (int32_t)((uint32_t)m + (uint32_t)sd) >> 1;
        b = (int32_t)((uint32_t)m - (uint32_t)sd) >> 1;
    }
}

// ---- host: the frame table of a region (first audio frame to end of file) ----
enum { INDEX_OK = 0, INDEX_FORMAT = 1, INDEX_MISSING = 2 };
// Walk from the first frame: parse the header, then scan forward for the next sync whose header parses, whose CRC-8 holds, whose
// sample format is the stream's and whose frame number is the previous + 1 (the number only filters false syncs: the first may be
// anything).  Positions are the running sum of the block sizes.  rows[k] = {offset, first sample, block size, clip} for n_frames
// frames; INDEX_FORMAT: a block size other than the stream's before the last frame, more frames than planned, a sum other than the
// stream length, a variable-block-size header; INDEX_MISSING: no successor.
template <class Row>
inline int index_region(const Tables& t, const uint8_t* d, uint32_t n, int bits, int channels, int block_size, int32_t n_frames,
                        int64_t n_samples, int32_t clip, Row* rows) {
    Header h;
    if (parse_header(t, d, n, h) != HDR_OK || h.variable) return INDEX_FORMAT;
    uint32_t pos = 0;
    int64_t first = 0;
    for (int32_t k = 0;; ++k) {
        if (k >= n_frames || (h.bits == 0 ? bits : h.bits) != bits || h.channels != channels) return INDEX_FORMAT;
        if (k < n_frames - 1 ? h.bs != block_size : h.bs > block_size) return INDEX_FORMAT;
        rows[k].offset = (int32_t)pos;
        rows[k].first_sample = (int32_t)first;
        rows[k].block_size = h.bs;
        rows[k].clip = clip;
        first += h.bs;
        if (k == n_frames - 1) return first == n_samples ? INDEX_OK : INDEX_FORMAT;
        const uint64_t want = h.number + 1;
        uint32_t at = pos + (uint32_t)h.len;
        for (;;) {
            const void* hit = at < n ? memchr(d + at, 0xFF, n - at) : nullptr;
            if (!hit) return INDEX_MISSING;
            at = (uint32_t)((const uint8_t*)hit - d);
            Header c;
            if (parse_header(t, d + at, n - at, c) == HDR_OK && !c.variable && c.number == want &&
                (c.bits == 0 ? bits : c.bits) == bits && c.channels == channels) {
                h = c;
                pos = at;
                break;
            }
            ++at;
        }
    }
}

}  // namespace nqff
