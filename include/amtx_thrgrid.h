/*
 * amtx -- C ABI, tenth header: a GRID of decision thresholds applied to probability maps, without building a roll per threshold.
 *
 * Same conventions as include/amtx.h (extern "C", caller-owned DEVICE pointers, explicit stream as void*, int return, message via
 * amtx_last_error()), same library (libamtx.so), same binding (amt_tools_amd/_lib.py, HEADERS).  The tables pinned for the earlier
 * headers stay as they are; this header's functions are pinned in tests/golden/abi_signatures_thrgrid.json.
 *
 * Both functions take PROBABILITY maps in the decoder's layout, [batch][keys][num_frames] fp32 -- what amtx_pianoroll_fwd writes with
 * threshold < 0 -- and cut them on the fly with amtx_pianoroll_fwd's own expression on the same float,
 *     cell = s < thr ? 0 : 1          (s == thr is active, a NaN is active),
 * so every result is bit-equal to thresholding first and calling the function named beside it.  Thresholds and pair tables are small
 * DEVICE arrays.  Neither function allocates; every output element is written by the call, and nothing depends on what the outputs
 * held before.  Sums are integers added in a fixed order, no atomics.
 */
#ifndef AMTX_THRGRID_H
#define AMTX_THRGRID_H

#include "amtx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* For every clip b and threshold g: counts[b][g] = {cells active in both maps, in the estimate cut at thresholds[g], in the reference}
 * -- the three integers amtx_eval_multipitch_counts (slices = 1) answers for the roll cut at thresholds[g] (a reference cell counts
 * when it is non-zero).  One pass over prob and ref, whatever G.
 *   prob, ref    [batch][keys][num_frames] fp32, 4-byte aligned; keys * num_frames need not be a multiple of 4
 *   thresholds   [G] fp32 on the device
 *   counts       [batch][G][3] int64, 8-byte aligned
 * AMTX_ERR_ARG: a null or misaligned pointer, batch, keys or num_frames below 1, keys * num_frames or batch of 2^31 or more, G outside
 * [1, 32]. */
int amtx_eval_multipitch_grid_counts(const float* prob, const float* ref, int batch, int keys, int num_frames, const float* thresholds, int G,
                                     int64_t* counts, void* stream);

/* amtx_notes_decode for P threshold pairs at once: pairs_thr[p] = {onset_thr, frame_thr}.  Row (p * batch + b) * keys + k of `pairs`
 * ([rows][capacity][2] int32) and `counts` ([rows] int32) holds what amtx_notes_decode writes for row (b, k) given on_prob cut at
 * onset_thr and mp_prob cut at frame_thr: events {onset frame, offset frame} in descending frame order, counts[row] = the number of
 * events found, of which the first min(counts[row], capacity) are stored.  on_prob may be NULL: onsets are then derived from the frame
 * roll and a pair's first entry is not read.  The output is what amtx_notes_rows takes with batch = P * batch.
 *   on_prob, mp_prob   [batch][keys][num_frames] fp32
 *   pairs_thr          [P][2] fp32 on the device
 * AMTX_ERR_ARG: a null mp_prob / pairs_thr / pairs / counts, a size below 1, P * batch * keys of 2^31 or more. */
int amtx_notes_decode_grid(const float* on_prob, const float* mp_prob, int batch, int keys, int num_frames, const float* pairs_thr, int P,
                           int capacity, int32_t* pairs, int32_t* counts, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* AMTX_THRGRID_H */
