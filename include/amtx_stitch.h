/*
 * amtx -- C ABI, seventh header: whole-track maps stitched from the outputs of overlapped clips.
 *
 * Same conventions as include/amtx.h (extern "C", caller-owned DEVICE pointers unless a parameter says host, explicit stream as void*,
 * int return, message via amtx_last_error()), same library (libamtx.so), same binding (amt_tools_amd/_lib.py, HEADERS).  The tables
 * pinned for the earlier headers stay as they are; this header's function is pinned in tests/golden/abi_signatures_stitch.json.
 *
 * A batch tensor `src` of shape [batch][rows][num_frames] holds one output map of `batch` equally long clips (a piano roll, offset
 * probabilities, a tablature).  Every clip keeps `count` of its columns, from column src_first on; they become the columns
 * [dst_first, dst_first + count) of the clip's TRACK, whose whole map is a contiguous [rows][L] inside one flat destination, `base`
 * elements in.  amt_tools_amd.tracks.seam_clips names clips and kept columns so that every frame of a track is kept exactly once;
 * amt_tools_amd.tracks.TrackMaps owns the destination.
 *
 * DESCRIPTORS: int64 [batch][5] = {base, L, dst_first, src_first, count}, once on the host and once on the device (the convention of
 * amtx_cqt_pyramid_build): the entry point checks every row of the HOST copy before anything is launched, the kernel reads the DEVICE
 * copy, and the caller keeps the two equal.
 */
#ifndef AMTX_STITCH_H
#define AMTX_STITCH_H

#include "amtx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* dst[base_b + r * L_b + dst_first_b + i] = src[b][r][src_first_b + i] for every clip b < batch, r < rows, i < count_b.
 *   src        [batch][rows][num_frames] elements of elem_bytes bytes (4: float32 maps; 8: int64 tablature), contiguous
 *   desc_host  HOST int64 [batch][5], desc its device copy
 *   dst        dst_elems elements of elem_bytes bytes
 * Bit patterns are copied: NaN payloads, -0.0 and -1 arrive as they left.  AMTX_ERR_ARG, with nothing launched and nothing written, for
 * a null pointer, an element size other than 4 or 8, a pointer that is not aligned to it, sizes below 1, batch * rows of 2^31 or more,
 * and for a row with a negative entry, src_first + count > num_frames, dst_first + count > L or base + rows * L > dst_elems.
 * The named elements of dst are written exactly once each, nothing else is written, dst is never read; no workspace, no atomics.
 * Ranges of two clips that overlap in dst are the caller's to avoid. */
int amtx_stitch_clips(const void* src, int elem_bytes, int batch, int rows, int64_t num_frames, const int64_t* desc_host,
                      const int64_t* desc, void* dst, int64_t dst_elems, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* AMTX_STITCH_H */
