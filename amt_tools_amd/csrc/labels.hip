// Label clips cut from the run-length encoded label maps of resident tracks (include/amtx_labels.h, amt_tools_amd/tracks.py LabelBank).
//
// One wave per (clip, row), LABEL_WAVES rows per block.  The wave finds the runs that cover its clip's frames with two wave-uniform binary
// searches over the row's runs (the run of first_frame, the run of the last frame), stages the first frames of that window in its own
// slice of LDS where they fit, and then every lane resolves its own frame by a binary search inside the window: 64 consecutive frames of
// a row leave as one coalesced store.  Trip counts: ceil(log2(runs)) per search, ceil(T / 64) for the frame and staging loops -- a row
// that alternates every frame costs what a constant row costs, apart from the search depth.  Every output element is written once, by one
// lane; nothing is read from `out`; no workspace.
//
// The launch writes batch * rows * T elements (the piano recipe: 8 x 264 x 625 x 4 B = 5.3 MB) and reads a few KiB of runs: it is bound
// by launch latency, not by the store width, so the stores stay one element per lane (rows are only 4-byte aligned when T is odd).
#include "amtx_common.h"
#include "../../include/amtx_labels.h"

#define LABEL_WAVES 4                    // rows per block
#define LABEL_LDS_RUNS 1024              // first frames a wave stages (4 KiB per wave); a longer window is searched in memory

struct LabelKeys {
    int num_keys;
    int rows[AMTX_LABEL_MAX_KEYS + 1];   // ascending; rows[0] = row_lo, rows[num_keys] = row_hi
};

// Index of the last of `first[0 .. n)` (ascending, first[0] <= f) that is <= f.  ceil(log2(n)) iterations whatever the data.
template <class P>
static __device__ __forceinline__ int64_t last_not_after(P first, int64_t n, int f) {
    int64_t base = 0;
    while (n > 1) {
        const int64_t half = n >> 1;
        if (first[base + half] <= f) base += half;
        n -= half;
    }
    return base;
}

template <class OutT>
__global__ __launch_bounds__(LABEL_WAVES * 64) void label_clips_kernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ run_first,
                                                                      const int32_t* __restrict__ run_bits, int num_tracks, int rows_total,
                                                                      LabelKeys keys, const int64_t* __restrict__ desc, int batch, int T,
                                                                      OutT* __restrict__ out) {
    __shared__ int32_t staged[LABEL_WAVES][LABEL_LDS_RUNS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row_lo = keys.rows[0], nrows = keys.rows[keys.num_keys] - row_lo;
    const int64_t item = (int64_t)blockIdx.x * LABEL_WAVES + wave;
    const bool active = item < (int64_t)batch * nrows;             // wave-uniform; an idle wave still meets the barrier below
    const int b = active ? (int)(item / nrows) : 0;
    const int row = row_lo + (active ? (int)(item % nrows) : 0);

    int64_t track = desc[(int64_t)b * 3];
    track = track < 0 ? 0 : (track >= num_tracks ? num_tracks - 1 : track);           // no read leaves the run tables (amtx_labels.h)
    const int64_t f0_64 = desc[(int64_t)b * 3 + 1];
    const int f0 = f0_64 < 0 ? 0 : (f0_64 > 0x7fffffff - T ? 0x7fffffff - T : (int)f0_64);   // f0 + T - 1 stays an int32 frame

    const int64_t g = track * rows_total + row;
    const int64_t lo = row_ptr[g], n = row_ptr[g + 1] - lo;        // n >= 1 runs, the first at frame 0
    const int32_t* first = run_first + lo;
    const int64_t j0 = last_not_after(first, n, f0);                // the run of the clip's first frame
    const int64_t j1 = j0 + last_not_after(first + j0, n - j0, f0 + T - 1);       // ... and of its last
    const int64_t w = j1 - j0 + 1;                                  // runs of the window: <= min(n, T)
    const bool in_lds = w <= LABEL_LDS_RUNS;
    if (active && in_lds)
        for (int i = lane; i < w; i += 64) staged[wave][i] = first[j0 + i];           // <= ceil(T / 64) iterations
    __syncthreads();
    if (!active) return;

    // map k of this launch: rows [keys.rows[k], keys.rows[k + 1]); key-major output (amtx_labels.h)
    int k = 0;
    for (int i = 1; i < keys.num_keys; ++i) k += row >= keys.rows[i];
    const int key_lo = keys.rows[k], key_rows = keys.rows[k + 1] - key_lo;
    OutT* dst = out + ((int64_t)(key_lo - row_lo) * batch + (int64_t)b * key_rows + (row - key_lo)) * T;
    const int32_t* bits = run_bits + lo + j0;
    if (in_lds) {
        for (int t = lane; t < T; t += 64) dst[t] = (OutT)bits[last_not_after(&staged[wave][0], w, f0 + t)];
    } else {
        for (int t = lane; t < T; t += 64) dst[t] = (OutT)bits[last_not_after(first + j0, w, f0 + t)];
    }
}

extern "C" int amtx_label_clips(const int64_t* row_ptr, const int32_t* run_first, const int32_t* run_bits, int num_tracks, int rows_total,
                                int row_lo, int row_hi, const int64_t* key_rows, int num_keys, const int64_t* desc, int batch,
                                int64_t num_frames, void* out, int out_kind, void* stream) {
    AMTX_REQUIRE(row_ptr && run_first && run_bits && key_rows && desc && out, "amtx_label_clips: null argument");
    AMTX_REQUIRE(num_tracks >= 1 && rows_total >= 1, "amtx_label_clips: num_tracks=%d, rows_total=%d: at least one each", num_tracks, rows_total);
    AMTX_REQUIRE(batch >= 1, "amtx_label_clips: batch=%d: at least one clip", batch);
    AMTX_REQUIRE(num_frames >= 1 && num_frames < 0x7fffffff, "amtx_label_clips: num_frames=%lld: at least one frame, fewer than 2^31 - 1",
                 (long long)num_frames);
    AMTX_REQUIRE(0 <= row_lo && row_lo < row_hi && row_hi <= rows_total, "amtx_label_clips: row_lo=%d, row_hi=%d: an empty row range, or one outside "
                 "the %d rows of a track", row_lo, row_hi, rows_total);
    AMTX_REQUIRE(num_keys >= 1 && num_keys <= AMTX_LABEL_MAX_KEYS, "amtx_label_clips: num_keys=%d: between 1 and %d", num_keys, AMTX_LABEL_MAX_KEYS);
    AMTX_REQUIRE(out_kind == 0 || out_kind == 1, "amtx_label_clips: out_kind=%d: 0 (32-bit patterns) or 1 (int64)", out_kind);
    LabelKeys keys;
    keys.num_keys = num_keys;
    for (int k = 0; k <= num_keys; ++k) {
        AMTX_REQUIRE(key_rows[k] >= row_lo && key_rows[k] <= row_hi && (k == 0 || key_rows[k] > key_rows[k - 1]),
                     "amtx_label_clips: key_rows[%d]=%lld: ascending rows from row_lo=%d to row_hi=%d", k, (long long)key_rows[k], row_lo, row_hi);
        keys.rows[k] = (int)key_rows[k];
    }
    AMTX_REQUIRE(keys.rows[0] == row_lo && keys.rows[num_keys] == row_hi, "amtx_label_clips: key_rows must start at row_lo=%d and end at row_hi=%d",
                 row_lo, row_hi);
    const int64_t items = (int64_t)batch * (row_hi - row_lo);
    const int64_t blocks = (items + LABEL_WAVES - 1) / LABEL_WAVES;
    AMTX_REQUIRE(blocks < 0x7fffffff, "amtx_label_clips: batch=%d x %d rows: too many for one launch", batch, row_hi - row_lo);
    const dim3 grid((unsigned)blocks), block(LABEL_WAVES * 64);
    hipStream_t s = (hipStream_t)stream;
    if (out_kind == 0)
        hipLaunchKernelGGL(label_clips_kernel<int32_t>, grid, block, 0, s, row_ptr, run_first, run_bits, num_tracks, rows_total, keys, desc, batch,
                           (int)num_frames, (int32_t*)out);
    else
        hipLaunchKernelGGL(label_clips_kernel<int64_t>, grid, block, 0, s, row_ptr, run_first, run_bits, num_tracks, rows_total, keys, desc, batch,
                           (int)num_frames, (int64_t*)out);
    AMTX_CHECK_LAUNCH();
    return AMTX_OK;
}
