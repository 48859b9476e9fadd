/*
 * amtx -- C ABI, fourth header: label clips cut from the run-length encoded label maps of resident tracks.
 *
 * Same conventions as include/amtx.h (extern "C", caller-owned DEVICE pointers unless a parameter says host, explicit stream as void*,
 * int return, message via amtx_last_error()), same library (libamtx.so), same binding (amt_tools_amd/_lib.py, MORE_HEADERS).  The tables
 * pinned for the three earlier headers stay as they are; this header's functions are pinned in tests/golden/abi_signatures_labels.json.
 *
 * A LABEL BANK holds, for every track, `rows_total` rows of frame-aligned ground truth (the rows of all its label maps, one map after the
 * other).  A row is piecewise constant and stored as RUNS: run j holds one 32-bit pattern from frame run_first[j] up to the next run's
 * first frame of the same row, or to the track's end.  The global row of (track, row) is track * rows_total + row; its runs are
 * [row_ptr[g], row_ptr[g + 1]) of run_first / run_bits, at least one, the first at frame 0, first frames strictly ascending.
 * The device never sees a time or a note: amt_tools_amd.tracks.encode_rows makes the runs from the host maps.
 *
 * CLIP DESCRIPTORS: int64 [batch][3] = {track, first_frame, frames}, the rows of a PyramidClips' table; every clip has num_frames frames.
 * Device tables cannot be checked by the entry point: amt_tools_amd.tracks validates the descriptors where it builds them.  The kernel
 * clamps a track index into the bank, so that no read leaves the three run tables whatever a descriptor holds.
 */
#ifndef AMTX_LABELS_H
#define AMTX_LABELS_H

#include "amtx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Most label maps one launch serves (key_rows has one entry more). */
#define AMTX_LABEL_MAX_KEYS 16

/* Columns [first_frame, first_frame + num_frames) of the rows [row_lo, row_hi) of every clip's track, decoded into `out`.
 * key_rows: HOST array of num_keys + 1 ascending row numbers, key_rows[0] = row_lo, key_rows[num_keys] = row_hi: map k is the rows
 * [key_rows[k], key_rows[k + 1]).  out is key-major: map k starts (key_rows[k] - row_lo) * batch * num_frames elements in and is a
 * contiguous [batch][rows of k][num_frames] there.  out_kind 0: the 32-bit patterns as they are (float32 maps); out_kind 1: the
 * patterns sign-extended to int64.  Every element of out is written exactly once; out is never read; no workspace. */
int amtx_label_clips(const int64_t* row_ptr, const int32_t* run_first, const int32_t* run_bits, int num_tracks, int rows_total, int row_lo,
                     int row_hi, const int64_t* key_rows, int num_keys, const int64_t* desc, int batch, int64_t num_frames, void* out,
                     int out_kind, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* AMTX_LABELS_H */
