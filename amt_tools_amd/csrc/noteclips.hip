// The note ground truth of clips cut from resident tracks (include/amtx_noteclips.h, amt_tools_amd/tracks.py NoteBank): the reference's
// tools.slice_batched_notes (amt_tools/tools/utils.py:322-361) for every (clip, slice) group of a batch, as one dense row array plus
// offsets -- what amtx_eval_notes_match takes as its reference.
//
// Three launches, no atomics:
//   1. note_clips_count_kernel   one wave per group walks its track's rows in chunks of 64, ballots the keep predicate and adds the
//                                popcounts: counts[g] in the workspace.
//   2. note_clips_scan_kernel    one block: exclusive scan of the counts into offsets[0 .. G], the total (64-bit sum, clamped at INT32_MAX)
//                                in offsets[G].
//   3. note_clips_write_kernel   the same walk with the same predicate (note_window: ONE function, so the two passes cannot disagree);
//                                a kept row goes to offsets[g] + kept so far + the number of kept lanes below its own, which keeps the
//                                bank's order.  Rows at and past rows_capacity are not written.
// Trip counts are ceil(group rows / 64) in both walks, whatever the values.  Every count, offset and row below min(total, capacity) is
// written exactly once before it is read; nothing else is written.  The arithmetic is comparisons, selections and one float64
// subtraction, so the rows equal NumPy's bit for bit.  A batch moves a few hundred KB: the call is bound by its three launches.
#include "amtx_common.h"
#include "../../include/amtx_noteclips.h"

#define NOTE_CLIP_WAVES 4                // groups per block

namespace {

struct NoteGroup {
    const double* rows;                  // the group's first row
    int64_t n;                           // its rows
    double start, stop;                  // the clip's window
};

// Group g = clip * slices + slice of the batch: the rows of its (clamped) track's slice and the clip's window.
static __device__ __forceinline__ NoteGroup note_group(const double* __restrict__ rows, const int64_t* __restrict__ group_ptr, int num_tracks,
                                                       int slices, const int64_t* __restrict__ clip_tracks, const double* __restrict__ windows, int g) {
    const int clip = g / slices, slice = g - clip * slices;
    int64_t track = clip_tracks[clip];
    track = track < 0 ? 0 : (track >= num_tracks ? num_tracks - 1 : track);           // no read leaves the bank (amtx_noteclips.h)
    const int64_t gg = track * slices + slice;
    const int64_t lo = group_ptr[gg], n = group_ptr[gg + 1] - lo;
    NoteGroup grp;
    grp.rows = rows + lo * 3;
    grp.n = n < 0 ? 0 : n;
    grp.start = windows[(int64_t)clip * 2];
    grp.stop = windows[(int64_t)clip * 2 + 1];
    return grp;
}

// Row i of the group under slice_batched_notes: whether it is kept (offset > start, then onset <= stop) and, if so, its clipped times.
static __device__ __forceinline__ bool note_window(const NoteGroup& grp, int64_t i, double& on, double& off, double& pitch) {
    if (i >= grp.n) return false;
    on = grp.rows[i * 3];
    off = grp.rows[i * 3 + 1];
    pitch = grp.rows[i * 3 + 2];
    return off > grp.start && on <= grp.stop;
}

__global__ __launch_bounds__(NOTE_CLIP_WAVES * 64) void note_clips_count_kernel(const double* __restrict__ rows, const int64_t* __restrict__ group_ptr,
                                                                               int num_tracks, int slices, const int64_t* __restrict__ clip_tracks,
                                                                               const double* __restrict__ windows, int groups, int* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * NOTE_CLIP_WAVES + (threadIdx.x >> 6);
    if (g >= groups) return;                                                          // wave-uniform; no barrier below
    const NoteGroup grp = note_group(rows, group_ptr, num_tracks, slices, clip_tracks, windows, g);
    long long kept = 0;
    for (int64_t c = 0; c < grp.n; c += 64) {
        double on, off, pitch;
        kept += __builtin_popcountll(__ballot(note_window(grp, c + lane, on, off, pitch)));
    }
    if (lane == 0) counts[g] = (int)(kept < 0x7fffffffll ? kept : 0x7fffffffll);
}

// exclusive scan of counts[0 .. groups) into offsets[0 .. groups] (one block; 64-bit running sum, offsets clamp at INT32_MAX)
__global__ __launch_bounds__(1024) void note_clips_scan_kernel(const int* __restrict__ counts, int groups, int* __restrict__ offsets) {
    __shared__ long long part[1024];
    __shared__ long long carry;
    const int tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < groups; base += 1024) {
        const int i = base + tid;
        const long long v = i < groups ? counts[i] : 0;
        part[tid] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const long long add = tid >= o ? part[tid - o] : 0;
            __syncthreads();
            part[tid] += add;
            __syncthreads();
        }
        const long long excl = carry + part[tid] - v;
        if (i < groups) offsets[i] = (int)(excl < 0x7fffffffll ? excl : 0x7fffffffll);
        __syncthreads();
        if (tid == 1023) carry += part[1023];
        __syncthreads();
    }
    if (tid == 0) offsets[groups] = (int)(carry < 0x7fffffffll ? carry : 0x7fffffffll);
}

__global__ __launch_bounds__(NOTE_CLIP_WAVES * 64) void note_clips_write_kernel(const double* __restrict__ rows, const int64_t* __restrict__ group_ptr,
                                                                               int num_tracks, int slices, const int64_t* __restrict__ clip_tracks,
                                                                               const double* __restrict__ windows, int groups, int relative_times,
                                                                               const int* __restrict__ offsets, double* __restrict__ rows_out,
                                                                               int64_t rows_capacity) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * NOTE_CLIP_WAVES + (threadIdx.x >> 6);
    if (g >= groups) return;
    const NoteGroup grp = note_group(rows, group_ptr, num_tracks, slices, clip_tracks, windows, g);
    const unsigned long long below = (1ull << lane) - 1ull;                           // the lanes under this one
    int64_t base = offsets[g];
    for (int64_t c = 0; c < grp.n; c += 64) {
        double on, off, pitch;
        const bool keep = note_window(grp, c + lane, on, off, pitch);
        const unsigned long long mask = __ballot(keep);
        const int64_t dst = base + __builtin_popcountll(mask & below);
        if (keep && dst < rows_capacity) {
            on = on >= grp.start ? on : grp.start;                                    // np.maximum / np.minimum of finite times
            off = off <= grp.stop ? off : grp.stop;
            if (relative_times) {
                on -= grp.start;
                off -= grp.start;
            }
            rows_out[dst * 3] = on;
            rows_out[dst * 3 + 1] = off;
            rows_out[dst * 3 + 2] = pitch;
        }
        base += __builtin_popcountll(mask);
    }
}

}  // namespace

static bool note_clips_sizes_ok(int batch, int slices) {
    return batch >= 1 && slices >= 1 && (int64_t)batch * slices < 0x7fffffffll - NOTE_CLIP_WAVES;
}

extern "C" size_t amtx_note_clips_workspace_bytes(int batch, int slices) {
    if (!note_clips_sizes_ok(batch, slices)) return 0;
    return (size_t)batch * slices * sizeof(int);
}

extern "C" int amtx_note_clips(const double* rows, const int64_t* group_ptr, int num_tracks, int slices, const int64_t* clip_tracks,
                               const double* windows, int batch, int relative_times, double* rows_out, int64_t rows_capacity, int32_t* offsets,
                               void* workspace, size_t workspace_bytes, void* stream) {
    AMTX_REQUIRE(rows && group_ptr && clip_tracks && windows && rows_out && offsets && workspace, "amtx_note_clips: null argument");
    AMTX_REQUIRE(num_tracks >= 1, "amtx_note_clips: num_tracks=%d: at least one", num_tracks);
    AMTX_REQUIRE(note_clips_sizes_ok(batch, slices), "amtx_note_clips: batch=%d, slices=%d: at least one each, fewer than 2^31 groups", batch, slices);
    AMTX_REQUIRE(rows_capacity >= 1 && rows_capacity < 0x7fffffffll, "amtx_note_clips: rows_capacity=%lld: at least one row, fewer than 2^31 - 1",
                 (long long)rows_capacity);
    AMTX_REQUIRE(relative_times == 0 || relative_times == 1, "amtx_note_clips: relative_times=%d: 0 or 1", relative_times);
    AMTX_REQUIRE(workspace_bytes >= amtx_note_clips_workspace_bytes(batch, slices), "amtx_note_clips: workspace of %zu bytes, %zu needed",
                 workspace_bytes, amtx_note_clips_workspace_bytes(batch, slices));
    AMTX_REQUIRE(((uintptr_t)workspace & 3) == 0, "amtx_note_clips: the workspace must be 4-byte aligned");
    const int groups = batch * slices;
    const dim3 grid((unsigned)((groups + NOTE_CLIP_WAVES - 1) / NOTE_CLIP_WAVES)), block(NOTE_CLIP_WAVES * 64);
    int* counts = (int*)workspace;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(note_clips_count_kernel, grid, block, 0, s, rows, group_ptr, num_tracks, slices, clip_tracks, windows, groups, counts);
    AMTX_CHECK_LAUNCH();
    hipLaunchKernelGGL(note_clips_scan_kernel, dim3(1), dim3(1024), 0, s, (const int*)counts, groups, (int*)offsets);
    AMTX_CHECK_LAUNCH();
    hipLaunchKernelGGL(note_clips_write_kernel, grid, block, 0, s, rows, group_ptr, num_tracks, slices, clip_tracks, windows, groups, relative_times,
                       (const int*)offsets, rows_out, rows_capacity);
    AMTX_CHECK_LAUNCH();
    return AMTX_OK;
}
