/*
 * amtx -- C ABI, third header: CQT-family clips cut from the resident decimation pyramids of whole tracks.
 *
 * Same conventions as include/amtx.h (extern "C", caller-owned DEVICE pointers unless a parameter says host, explicit stream as void*,
 * int return, message via amtx_last_error()), same library (libamtx.so), same binding (amt_tools_amd/_lib.py, LATER_HEADERS).  The tables
 * pinned for amtx.h and amtx_tracks.h stay as they are; this header's functions are pinned in tests/golden/abi_signatures_pyramid.json.
 *
 * A BANK is a set of tracks whose audio lies in one float32 buffer and whose pyramid levels lie in a second one.  Per track and level
 * the pyramid holds the level signal exactly as amtx_cqt_forward lays it out for one clip: `pad` samples (zeros for librosa >= 0.10,
 * the reflected samples for librosa 0.9), level_len samples, a tail up to level_stride.  For zero-padded plans level 0 is the audio
 * itself, read in place (level_stride[0] = 0: no storage).  The levels are produced by the kernels of amtx_cqt_forward run on the
 * whole track, so a clip's power map is, bit for bit, the columns [first_frame, first_frame + frames) of the track's own.
 *
 * TRACK TABLE: int64 [num_tracks][cols], cols = 4 + 3 * levels + harmonics (amtx_cqt_track_cols), one row per track:
 *   [0] element offset of the track in `audio`, a multiple of 4      [1] its samples
 *   [2] max over h of rows_h                                          [3] frames of its feature map (amtx_cqt_num_frames)
 *   [4 + 3 l ..] level l: element offset in `pyramid` (a multiple of 4: 16-byte aligned), level_len, level_stride
 *   [4 + 3 levels + h] rows_h: frames of harmonic h's own map (the dB reference is its maximum over these)
 * CLIP DESCRIPTORS: int64 [batch][3] = {track, first_frame, frames}, 1 <= frames <= num_frames, first_frame + frames <= [3] of the track.
 * Device tables cannot be checked by the entry points: amtx_cqt_pyramid_build checks the host copy of the track table against the plan
 * and the buffers' sizes, amt_tools_amd.tracks validates the descriptors where it builds them.
 */
#ifndef AMTX_PYRAMID_H
#define AMTX_PYRAMID_H

#include "amtx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct amtx_cqt_plan amtx_cqt_plan;   /* include/amtx.h; repeated for readers of this header alone */

/* Host only.  Columns of a track-table row for this plan (> 0), or a negative error code. */
int amtx_cqt_track_cols(const amtx_cqt_plan* plan);

/* Host only.  The layout of one track of num_samples: level_len / level_stride (arrays of 16; entries past the returned count untouched),
 * rows_h (array of 16) and *frames.  Returns the number of pyramid levels.  AMTX_ERR_UNSUPPORTED for a plan (or a track length under it)
 * whose basis products the windowed kernel does not cover: such a plan has no clip form. */
int amtx_cqt_track_layout(const amtx_cqt_plan* plan, int64_t num_samples, int64_t* level_len, int64_t* level_stride, int64_t* rows_h,
                          int64_t* frames);

/* Decimations, pads and the track maxima of a whole bank.  tracks_host / tracks: the track table on the host (checked here against
 * amtx_cqt_track_layout, audio_elems and pyramid_elems; rows in ascending, non-overlapping order) and its device copy.
 * maxima: [num_tracks][harmonics], the maximum of harmonic h's power map over its rows_h frames -- no map is written. */
int amtx_cqt_pyramid_build(const amtx_cqt_plan* plan, const float* audio, int64_t audio_elems, const int64_t* tracks_host,
                           const int64_t* tracks, int num_tracks, float* pyramid, int64_t pyramid_elems, float* maxima, void* stream);

/* power: [batch][harmonics][n_bins][num_frames], column t of clip b = frame first_frame + t of its track; columns t >= frames zero.
 * Reads nothing outside the clip's own track: [level offset, level offset + level_stride) of each level, the track's samples of `audio`. */
int amtx_cqt_power_clips(const amtx_cqt_plan* plan, const float* audio, const float* pyramid, const int64_t* tracks, const int64_t* desc,
                         int batch, int64_t num_frames, float* power, void* stream);

/* Bytes of the power map the scaled forms below compute first. */
size_t amtx_cqt_clips_workspace_bytes(const amtx_cqt_plan* plan, int batch, int64_t num_frames);

/* The scaled forms of amtx_cqt_forward / _forward16 / _forward16_split for clips: refs [batch][harmonics] are the dB references (the
 * maxima of the clips' tracks, gathered by the caller); out [batch][harmonics][n_bins][num_frames] fp32, out16 [batch][num_frames][n_bins][8]
 * bf16 (and its second plane plane_elems 16-bit elements behind it).  workspace: 256-byte aligned. */
int amtx_cqt_clips(const amtx_cqt_plan* plan, const float* audio, const float* pyramid, const int64_t* tracks, const int64_t* desc, int batch,
                   int64_t num_frames, const float* refs, int decibels, void* workspace, size_t workspace_bytes, float* out, void* stream);
int amtx_cqt_clips16(const amtx_cqt_plan* plan, const float* audio, const float* pyramid, const int64_t* tracks, const int64_t* desc, int batch,
                     int64_t num_frames, const float* refs, int decibels, void* workspace, size_t workspace_bytes, void* out16, void* stream);
int amtx_cqt_clips16_split(const amtx_cqt_plan* plan, const float* audio, const float* pyramid, const int64_t* tracks, const int64_t* desc,
                           int batch, int64_t num_frames, const float* refs, int decibels, void* workspace, size_t workspace_bytes, void* out16,
                           int64_t plane_elems, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* AMTX_PYRAMID_H */
