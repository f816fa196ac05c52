// nisqa_mel_gather (include/nisqa_train.h): one training or validation batch out of the resident spectrogram store
// (nisqa_amd/melstore.py) -- the dB spectrograms of the clips `ids`, back to back in step order, and their top_db floors.
//
// A spectrogram row is 48 floats = 192 B = twelve 16-byte units, and every row of the store and of the output starts on a 16-byte
// boundary, so the copy is a flat stream of units: one thread moves one unit per trip of a grid-stride loop over out_frames * 12
// of them (a wave instruction: 1 KiB contiguous on the output side, contiguous on the store side except across a clip boundary).
// A unit's clip is found by binary search in out_frame_off, which is staged in LDS when the batch has at most
// NISQA_MEL_GATHER_LDS_CLIPS clips (every batch of the training loop) and read from global memory above that.
//
// The tables are the caller's (checked on the host before the launch), but nothing here trusts them: an entry whose id is out of
// range or whose output span is not the stored length is skipped -- its rows stay as they were, its floor becomes NaN -- and a unit
// that no valid entry covers is skipped too.  Store-side row arithmetic is 64-bit.  Vector loads and stores only.
#include "common.hpp"
#include "../../include/nisqa_hip.h"
#include "../../include/nisqa_train.h"

namespace {

constexpr int THREADS = 256;
constexpr int UNITS = 12;                                  // 16-byte units per spectrogram row
constexpr int LDS_CLIPS = NISQA_MEL_GATHER_LDS_CLIPS;
constexpr int MAX_BLOCKS = 2048;                           // 8 per CU; the rest is the grid-stride loop

// the stored rows [r0, r0 + span) of entry c, or false: id out of range / a span that is not the stored length / rows outside the store
NQ_DEV bool entry_rows(const int64_t* __restrict__ clip_row, int64_t store_rows, int n_store, const int32_t* __restrict__ ids, int c,
                       int span, int64_t& r0) {
    const int id = ids[c];
    if (id < 0 || id >= n_store || span <= 0) return false;
    r0 = clip_row[id];
    const int64_t r1 = clip_row[id + 1];
    return r0 >= 0 && r1 <= store_rows && r1 - r0 == (int64_t)span;
}

template <bool LDS>
__global__ __launch_bounds__(THREADS) void mel_gather_kernel(const uint4* __restrict__ store, int64_t store_rows,
                                                             const int64_t* __restrict__ clip_row, const float* __restrict__ store_floor,
                                                             int n_store, const int32_t* __restrict__ ids,
                                                             const int32_t* __restrict__ out_frame_off, int n, int out_frames,
                                                             uint4* __restrict__ out_mel, float* __restrict__ out_floor) {
    __shared__ int32_t s_off[LDS ? LDS_CLIPS + 1 : 1];
    if (LDS) {
        for (int i = threadIdx.x; i <= n; i += THREADS) s_off[i] = out_frame_off[i];
        __syncthreads();
    }
    const int32_t* off = LDS ? s_off : out_frame_off;
    const int64_t tid = (int64_t)blockIdx.x * THREADS + threadIdx.x, stride = (int64_t)gridDim.x * THREADS;

    for (int64_t c = tid; c < n; c += stride) {            // the floors: one entry per thread
        int64_t r0;
        const bool ok = entry_rows(clip_row, store_rows, n_store, ids, (int)c, off[c + 1] - off[c], r0);
        out_floor[c] = ok ? store_floor[ids[c]] : __uint_as_float(0x7fc00000u);
    }

    const int64_t total = (int64_t)out_frames * UNITS;
    for (int64_t u = tid; u < total; u += stride) {
        const int row = (int)(u / UNITS), k = (int)(u % UNITS);
        int lo = 0, hi = n;                                // the last entry whose first row is <= row (whatever the table holds: lo stays in [0, n))
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (off[mid] <= row) lo = mid; else hi = mid;
        }
        const int first = off[lo], span = off[lo + 1] - first, local = row - first;
        int64_t r0;
        if (local < 0 || local >= span || !entry_rows(clip_row, store_rows, n_store, ids, lo, span, r0)) continue;
        out_mel[u] = store[(r0 + local) * UNITS + k];
    }
}

}  // namespace

extern "C" int nisqa_mel_gather(const float* store, int64_t store_rows, const int64_t* clip_row, const float* store_floor,
                                int32_t n_store, const int32_t* ids, const int32_t* out_frame_off, int32_t n, int32_t out_frames,
                                float* out_mel, float* out_floor, void* stream) {
    if (!store || !clip_row || !store_floor || !ids || !out_frame_off || !out_mel || !out_floor) return NISQA_ERR_ARG;
    if (n <= 0 || n_store <= 0 || out_frames <= 0 || store_rows <= 0) return NISQA_ERR_ARG;
    if (((uintptr_t)store & 15) || ((uintptr_t)out_mel & 15)) return NISQA_ERR_ARG;
    const int64_t total = (int64_t)out_frames * UNITS;
    const int64_t want = (total + THREADS - 1) / THREADS;
    const unsigned blocks = (unsigned)(want < MAX_BLOCKS ? want : MAX_BLOCKS);
    NQ_LAUNCH_BEGIN();
    if (n <= LDS_CLIPS)
        hipLaunchKernelGGL(mel_gather_kernel<true>, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, (const uint4*)store, store_rows,
                           clip_row, store_floor, n_store, ids, out_frame_off, n, out_frames, (uint4*)out_mel, out_floor);
    else
        hipLaunchKernelGGL(mel_gather_kernel<false>, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, (const uint4*)store, store_rows,
                           clip_row, store_floor, n_store, ids, out_frame_off, n, out_frames, (uint4*)out_mel, out_floor);
    return NQ_LAUNCH_STATUS();
}
