/*
 * amtx -- C ABI, sixth header: the note ground truth of clips cut from resident tracks.
 *
 * Same conventions as include/amtx.h (extern "C", caller-owned DEVICE pointers unless a parameter says host, explicit stream as void*,
 * int return, message via amtx_last_error()), same library (libamtx.so), same binding (amt_tools_amd/_lib.py, HEADERS).  The tables
 * pinned for the earlier headers stay as they are; this header's functions are pinned in tests/golden/abi_signatures_noteclips.json.
 *
 * A NOTE BANK holds the notes of every track as rows {onset_s, offset_s, pitch} (float64) in GROUPS: a track has `slices` groups (1 for
 * batched notes, one per string for the stacked notes of a tablature track), group (track, slice) owns the rows
 * [group_ptr[track * slices + slice], group_ptr[track * slices + slice + 1]) of `rows`, in (pitch, onset) order -- the order
 * amtx_eval_notes_match reads.  amt_tools_amd.tracks.NoteBank builds both tables on the host.
 *
 * A CLIP is (track, [start_time, stop_time]); its notes are the reference's tools.slice_batched_notes(group, start_time, stop_time,
 * relative_times) (amt_tools/tools/utils.py:322-361) of every group of its track: rows with offset > start_time and onset <= stop_time,
 * onset = max(onset, start_time), offset = min(offset, stop_time), both minus start_time when relative_times is set.  Comparisons,
 * selections and one float64 subtraction: the result equals NumPy's bit for bit.  The times come from the host (the device never
 * divides); NaN times are the caller's to refuse.
 *
 * Device tables cannot be checked by the entry point: amt_tools_amd.tracks validates them where it builds them.  The kernels clamp a
 * track index into the bank, so that no read leaves the two bank tables whatever clip_tracks holds.
 */
#ifndef AMTX_NOTECLIPS_H
#define AMTX_NOTECLIPS_H

#include "amtx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the workspace amtx_note_clips needs for `batch` clips of a bank with `slices` groups per track (host only; 0 for sizes the
 * call refuses). */
size_t amtx_note_clips_workspace_bytes(int batch, int slices);

/* The notes of `batch` clips: group g = clip * slices + slice owns the rows [offsets[g], offsets[g + 1]) of rows_out, in the bank's order
 * (the compaction is stable) -- the (rows, offsets) pair amtx_eval_notes_match takes as its reference.
 *   rows        float64 [N][3], group_ptr int64 [num_tracks * slices + 1]: the bank
 *   clip_tracks int64 [batch]; windows float64 [batch][2] = {start_time, stop_time}
 *   rows_out    float64 [rows_capacity][3]; offsets int32 [batch * slices + 1]
 * offsets[batch * slices] is the true total (clamped at INT32_MAX) and may exceed rows_capacity: rows at and past rows_capacity are not
 * written, and the caller retries with a larger buffer (the convention of amtx_notes_rows and amtx_tab_notes).  Every element of offsets
 * is written, every row below min(total, rows_capacity) exactly once, nothing else; neither they nor the workspace are read before they
 * are written, and there are no atomics.  Trip counts depend on the group sizes only. */
int amtx_note_clips(const double* rows, const int64_t* group_ptr, int num_tracks, int slices, const int64_t* clip_tracks,
                    const double* windows, int batch, int relative_times, double* rows_out, int64_t rows_capacity, int32_t* offsets,
                    void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* AMTX_NOTECLIPS_H */
