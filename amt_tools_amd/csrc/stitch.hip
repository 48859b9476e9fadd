// Whole-track maps stitched from the outputs of overlapped clips (include/amtx_stitch.h, amt_tools_amd/tracks.py TrackMaps): of every
// clip of a [batch][rows][num_frames] output tensor, the kept columns go into the clip's track, a contiguous [rows][L] map inside one
// flat destination.
//
// One launch, one kernel.  A wave owns one row of one clip and walks its kept columns 64 at a time: the frame axis is contiguous on both
// sides, so one wave instruction reads and one writes up to 256 (float32) or 512 (int64) contiguous bytes.  Source and destination are
// in general not co-aligned to 16 bytes -- src_first and dst_first differ by the clip's first frame -- so the copy is one element per
// lane.  No LDS, no atomics, no workspace.  The descriptor row of a wave's clip is wave-uniform; the trip count is ceil(count / 64).
// Elements are moved as unsigned integers of their size: bit patterns, never values.
#include "amtx_common.h"
#include "../../include/amtx_stitch.h"

#define STITCH_WAVES 4                   // rows of clips per block

namespace {

template <typename T>
__global__ __launch_bounds__(STITCH_WAVES * 64) void stitch_clips_kernel(const T* __restrict__ src, int64_t clip_rows, int rows, int64_t num_frames,
                                                                        const int64_t* __restrict__ desc, T* __restrict__ dst) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * STITCH_WAVES + (threadIdx.x >> 6);         // row g of the batch: clip g / rows, row g % rows
    if (g >= clip_rows) return;                                                        // wave-uniform; no barrier below
    const int64_t b = g / rows, r = g - b * rows;
    const int64_t* d = desc + b * 5;                                                   // {base, L, dst_first, src_first, count}
    const int64_t count = d[4];
    const T* from = src + g * num_frames + d[3];
    T* to = dst + d[0] + r * d[1] + d[2];
    for (int64_t i = lane; i < count; i += 64) to[i] = from[i];
}

}  // namespace

extern "C" int amtx_stitch_clips(const void* src, int elem_bytes, int batch, int rows, int64_t num_frames, const int64_t* desc_host,
                                 const int64_t* desc, void* dst, int64_t dst_elems, void* stream) {
    AMTX_REQUIRE(src && desc_host && desc && dst, "amtx_stitch_clips: null argument");
    AMTX_REQUIRE(elem_bytes == 4 || elem_bytes == 8, "amtx_stitch_clips: elem_bytes=%d: 4 (float32 maps) or 8 (int64 tablature)", elem_bytes);
    AMTX_REQUIRE(((uintptr_t)src % elem_bytes) == 0 && ((uintptr_t)dst % elem_bytes) == 0, "amtx_stitch_clips: src and dst must be aligned to %d bytes",
                 elem_bytes);
    AMTX_REQUIRE(batch >= 1 && rows >= 1 && num_frames >= 1 && dst_elems >= 1, "amtx_stitch_clips: batch=%d, rows=%d, num_frames=%lld, dst_elems=%lld: at least one each",
                 batch, rows, (long long)num_frames, (long long)dst_elems);
    const int64_t clip_rows = (int64_t)batch * rows;
    AMTX_REQUIRE(clip_rows < 0x7fffffffll - STITCH_WAVES, "amtx_stitch_clips: batch=%d x rows=%d: fewer than 2^31 rows in all", batch, rows);
    AMTX_REQUIRE(num_frames <= INT64_MAX / clip_rows, "amtx_stitch_clips: batch x rows x num_frames does not fit 63 bits");
    for (int b = 0; b < batch; b++) {
        const int64_t* d = desc_host + (int64_t)b * 5;
        AMTX_REQUIRE(d[0] >= 0 && d[1] >= 0 && d[2] >= 0 && d[3] >= 0 && d[4] >= 0, "amtx_stitch_clips: clip %d: a negative entry", b);
        AMTX_REQUIRE(d[4] <= num_frames && d[3] <= num_frames - d[4], "amtx_stitch_clips: clip %d: columns [%lld, %lld + %lld) leave the clip's %lld frames", b,
                     (long long)d[3], (long long)d[3], (long long)d[4], (long long)num_frames);
        AMTX_REQUIRE(d[4] <= d[1] && d[2] <= d[1] - d[4], "amtx_stitch_clips: clip %d: frames [%lld, %lld + %lld) leave the track's %lld frames", b,
                     (long long)d[2], (long long)d[2], (long long)d[4], (long long)d[1]);
        AMTX_REQUIRE(d[0] <= dst_elems && d[1] <= (dst_elems - d[0]) / rows, "amtx_stitch_clips: clip %d: the track map [%lld, %lld + %d x %lld) leaves the %lld elements of dst",
                     b, (long long)d[0], (long long)d[0], rows, (long long)d[1], (long long)dst_elems);
    }
    const dim3 grid((unsigned)((clip_rows + STITCH_WAVES - 1) / STITCH_WAVES)), block(STITCH_WAVES * 64);
    hipStream_t s = (hipStream_t)stream;
    if (elem_bytes == 4)
        hipLaunchKernelGGL(stitch_clips_kernel<uint32_t>, grid, block, 0, s, (const uint32_t*)src, clip_rows, rows, num_frames, desc, (uint32_t*)dst);
    else
        hipLaunchKernelGGL(stitch_clips_kernel<uint64_t>, grid, block, 0, s, (const uint64_t*)src, clip_rows, rows, num_frames, desc, (uint64_t*)dst);
    AMTX_CHECK_LAUNCH();
    return AMTX_OK;
}
