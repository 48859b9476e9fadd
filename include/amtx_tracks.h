/*
 * amtx -- C ABI, second header: entry points that work on clips cut from device-resident tracks.
 *
 * Same conventions as include/amtx.h (extern "C", caller-owned DEVICE pointers, explicit stream as void*, int return, message via
 * amtx_last_error()), same library (libamtx.so), same binding (amt_tools_amd/_lib.py reads both headers).  The table pinned for amtx.h,
 * tests/golden/abi_signatures.json, stays as it is; this header's functions are pinned in tests/golden/abi_signatures_tracks.json.
 */
#ifndef AMTX_TRACKS_H
#define AMTX_TRACKS_H

#include "amtx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct amtx_spec_plan amtx_spec_plan;   /* include/amtx.h; repeated for readers of this header alone */

/* Clips cut from longer tracks.  desc: device int64 [batch][4] = {track_start (element offset into audio), track_len (samples),
 * first_frame, frames}, 1 <= frames <= num_frames, first_frame + frames <= amtx_spec_num_frames(plan, track_len).
 * power: [batch][num_frames][n_bins], rows t >= frames[b] written as zeros; or NULL: maxima only.
 * clip_max[b]: maximum over the clip's `frames` rows.
 * Row t of clip b is frame first_frame + t of its track: the window starts at sample (first_frame + t) * hop - n_fft/2 of the track
 * (no - n_fft/2 when the plan is not centred), the plan's padding appears only where the TRACK ends, and no sample outside
 * [track_start, track_start + track_len) is read.  Same kernels, arithmetic and summation order as amtx_spec_power: rows and maxima are
 * the bits of amtx_spec_power run on the whole track.  The table's contents are not checked here (device memory); build it with
 * amt_tools_amd.tracks.clip_descriptors, which is where they are validated. */
int amtx_spec_power_clips(const amtx_spec_plan* plan, const float* audio, const int64_t* desc, int batch, int64_t num_frames,
                          float* power, float* clip_max, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* AMTX_TRACKS_H */
