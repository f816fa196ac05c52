// The device FLAC decoder (nisqa_amd/csrc/flac_frame.hpp) compiled as HOST code, driven the way the GPU path drives it: plan from
// STREAMINFO, frame table from the sync scan, every frame decoded from its bounded span into a workspace, stereo undone, MD5 checked.
// Twin of tools/flac_fuzz.cpp: bit flips, byte runs, truncations and scattered bytes in valid streams (written by tests/flac_enc.py)
// under AddressSanitizer + UBSan; a mutated stream must be refused or decode to what flac.hpp decodes it to, and nothing may be read
// or written out of bounds.  CPU only.
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -o flac_frame_fuzz tools/flac_frame_fuzz.cpp
//   ./flac_frame_fuzz a.flac b.flac ...       (3 000 mutations per file; prints accepted / refused / host-path / differing)
// tests/test_flac_frame_host.py builds the same file as a shared object (no sanitizer) and calls the nqff_* entries.
#include "../nisqa_amd/csrc/flac.hpp"
#include "../nisqa_amd/csrc/flac_frame.hpp"
#include <cstdio>
#include <cstdlib>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

struct nqff_row { int32_t offset, first_sample, block_size, clip; };
struct nqff_info {
    int64_t region_off, region_bytes, n_samples;
    int32_t n_frames, block_size, bits, channels, md5_set, eligible;
    uint8_t md5[16];
};

static const nqff::Tables& tables() {
    static nqff::Tables t;
    static bool done = false;
    if (!done) { nqff::fill_tables(t); done = true; }
    return t;
}

// STREAMINFO + metadata walk + first frame header -> what nisqa_ingest_flac_plan reports.  0 = a FLAC stream (eligible or not), 1 = not.
extern "C" int nqff_plan(const uint8_t* d, size_t n, nqff_info* o) {
    std::memset(o, 0, sizeof(*o));
    nqflac::Stream s;
    if (nqflac::stream_info(d, n, s) != 0 || !nqflac::walk_metadata(d, n, s)) return 1;
    o->region_off = (int64_t)s.first_frame;
    o->region_bytes = (int64_t)n - (int64_t)s.first_frame;
    o->n_samples = s.total;
    o->block_size = s.max_block;
    o->bits = s.bits;
    o->channels = s.channels;
    o->md5_set = s.have_md5;
    std::memcpy(o->md5, s.md5, 16);
    o->n_frames = (int32_t)((s.total + s.max_block - 1) / s.max_block);
    nqff::Header h;
    o->eligible = o->region_bytes >= 16 && o->region_bytes < ((int64_t)1 << 31) &&
                  nqff::parse_header(tables(), d + s.first_frame, (uint32_t)o->region_bytes, h) == nqff::HDR_OK && !h.variable &&
                  s.min_block == s.max_block && s.total >= s.max_block && s.total < ((int64_t)1 << 31) && s.channels <= 2;
    return 0;
}

extern "C" int nqff_index(const uint8_t* d, size_t n, const nqff_info* o, nqff_row* rows) {
    (void)n;
    return nqff::index_region(tables(), d + o->region_off, (uint32_t)o->region_bytes, o->bits, o->channels, o->block_size, o->n_frames,
                              o->n_samples, 0, rows);
}

struct RowOut {                                          // one frame's workspace: [channel][block size]
    int32_t* base;
    int32_t* cur;
    int bs, stride;
    void channel(int c) { cur = base + (size_t)c * stride; }
    void put(int i, int32_t v) {
        if ((unsigned)i >= (unsigned)bs) abort();        // (the decoder itself keeps to [0, bs): the kernel's guard never fires)
        cur[i] = v;
    }
};

// Every row's frame from its span -> out[sample * channels + channel].  0, or the kernel's status bits (1 << frame check, 0x80 MD5,
// 0x100 a row outside its clip).
extern "C" int nqff_decode(const uint8_t* d, size_t n, const nqff_info* o, const nqff_row* rows, int32_t* out) {
    (void)n;
    const uint8_t* reg = d + o->region_off;
    const int ch = o->channels;
    std::vector<int32_t> ws((size_t)ch * o->block_size);
    int status = 0;
    for (int32_t g = 0; g < o->n_frames; ++g) {
        const nqff_row& r = rows[g];
        const bool last = g == o->n_frames - 1;
        const int64_t first = (int64_t)g * o->block_size, left = o->n_samples - first;
        const int64_t end = last ? o->region_bytes : rows[g + 1].offset;
        if (r.first_sample != first || r.block_size != (left < o->block_size ? left : o->block_size) || r.offset < 0 ||
            r.offset >= o->region_bytes || end <= r.offset || end > o->region_bytes) { status |= 0x100; continue; }
        // the span is copied to a heap block of exactly its size: a sanitizer sees any read outside it
        std::vector<uint8_t> span(reg + r.offset, reg + end);
        RowOut w{ws.data(), ws.data(), r.block_size, o->block_size};
        int ca = 0;
        const int rc = nqff::frame(tables(), span.data(), (uint32_t)span.size(), !last, r.block_size, o->bits, ch, w, &ca);
        if (rc != nqff::FRAME_OK) { status |= 1 << rc; continue; }
        for (int i = 0; i < r.block_size; ++i) {
            int32_t a = ws[i], b = ch == 2 ? ws[(size_t)o->block_size + i] : 0;
            if (ch == 2) nqff::undo_stereo(ca, a, b);
            out[(first + i) * ch] = a;
            if (ch == 2) out[(first + i) * ch + 1] = b;
        }
    }
    if (!status && o->md5_set) {
        nqflac::Md5 md5;
        const int bytes = (o->bits + 7) / 8;
        std::vector<uint8_t> raw((size_t)o->n_samples * ch * bytes);
        uint8_t* w = raw.data();
        for (int64_t i = 0; i < o->n_samples * ch; ++i)
            for (int k = 0; k < bytes; ++k) *w++ = (uint8_t)((uint32_t)out[i] >> (8 * k));
        md5.add(raw.data(), raw.size());
        uint8_t got[16];
        md5.finish(got);
        if (std::memcmp(got, o->md5, 16)) status |= 0x80;
    }
    return status;
}

struct Keep : nqflac::Sink {
    std::vector<int32_t> v;
    void block(const int32_t* const* c, int ch, int count) override {
        for (int i = 0; i < count; ++i)
            for (int k = 0; k < ch; ++k) v.push_back(c[k][i]);
    }
};

// One file image through both decoders.  0 = both accept and agree, 1 = the device path refuses, 2 = the stream takes the host path,
// 3 = THEY DIFFER (the device path accepts what the host decoder refuses, or other samples).
extern "C" int nqff_compare(const uint8_t* d, size_t n) {
    nqff_info o;
    if (nqff_plan(d, n, &o) != 0 || !o.eligible) return 2;
    std::vector<nqff_row> rows((size_t)o.n_frames);
    if (nqff_index(d, n, &o, rows.data()) != 0) return 2;            // (the read fails: the file is restaged on the host path)
    std::vector<int32_t> out((size_t)o.n_samples * o.channels);
    if (nqff_decode(d, n, &o, rows.data(), out.data()) != 0) return 1;
    nqflac::Stream s;
    Keep sink;
    int64_t done = 0;
    if (nqflac::stream_info(d, n, s) != 0 || nqflac::decode(d, n, s, &sink, &done) != 0) return 3;
    return sink.v == out ? 0 : 3;
}

int main(int argc, char** argv) {
    long count[4] = {0, 0, 0, 0};
    for (int f = 1; f < argc; ++f) {
        const int fd = open(argv[f], O_RDONLY);
        struct stat sb;
        if (fd < 0 || fstat(fd, &sb) != 0) return 1;
        std::vector<uint8_t> orig((size_t)sb.st_size);
        if (read(fd, orig.data(), orig.size()) != (ssize_t)orig.size()) return 1;
        close(fd);
        if (nqff_compare(orig.data(), orig.size()) != 0) { printf("%s: the unmutated stream is not accepted\n", argv[f]); return 1; }
        srand(f);
        for (int it = 0; it < 3000; ++it) {
            std::vector<uint8_t> buf = orig;
            const size_t pos = 4 + rand() % (buf.size() - 4);
            switch (it % 4) {
                case 0: buf[pos] ^= 1 << (rand() % 8); break;
                case 1: for (int k = 0, m = 1 + rand() % 16; k < m && pos + k < buf.size(); ++k) buf[pos + k] = (uint8_t)rand(); break;
                case 2: buf.resize(pos); break;
                default: for (int k = 0; k < 8; ++k) buf[4 + rand() % (buf.size() - 4)] = (uint8_t)rand();
            }
            std::vector<uint8_t> exact(buf);                          // (capacity == size: reads past the image are seen)
            exact.shrink_to_fit();
            ++count[nqff_compare(exact.data(), exact.size())];
        }
    }
    printf("accepted %ld refused %ld host-path %ld differing %ld\n", count[0], count[1], count[2], count[3]);
    return count[3] ? 2 : 0;
}
