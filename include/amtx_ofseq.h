/*
 * amtx -- C ABI, ninth header: exact whole-track Onsets & Frames.  The acoustic half of the engine runs on overlapped clips, both BiLSTM
 * recurrences run once over whole tracks -- many tracks of different lengths per launch.
 *
 * Same conventions as include/amtx.h (extern "C", caller-owned DEVICE pointers unless a parameter says host, explicit stream as void*,
 * int return, message via amtx_last_error()), same library (libamtx.so), same binding (amt_tools_amd/_lib.py, HEADERS).  The tables
 * pinned for the earlier headers stay as they are; this header's functions are pinned in tests/golden/abi_signatures_ofseq.json.
 *
 * PACKED ROWS: R = sum of L_t rows hold S sequences (tracks) back to back.  SEQUENCE TABLE: int64 [S][2] = {row0, len}.  GATHER TABLE:
 * int64 [batch][3] = {src_first, count, dst_row}.  Every table travels twice, once on the host and once on the device (the convention
 * of amtx_stitch_clips): the entry point checks every row of the HOST copy before anything is launched, the kernels read the DEVICE
 * copy, and the caller keeps the two equal.  A sequence table is good when every row has len >= 1, row0 >= 0 and row0 + len <=
 * total_rows and no two sequences overlap; a bad row is AMTX_ERR_ARG naming the row, with nothing launched and nothing written.
 * The kernels take a block's slots in table order, so a caller lists the sequences longest first: a block's slots finish together.
 */
#ifndef AMTX_OFSEQ_H
#define AMTX_OFSEQ_H

#include "amtx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct amtx_of_model amtx_of_model;

/* amtx_bilstm_h_fwd over packed sequences: xproj [groups][total_rows][2][4 hidden], out [groups][total_rows][2 hidden], whh_packed
 * `groups` fragment sets of amtx_bilstm_h_pack one after the other.  Forward direction: rows row0 .. row0 + len - 1 of a sequence, backward
 * direction from row0 + len - 1 down.  Every sequence comes out with the bits amtx_bilstm_h_fwd gives it alone (batch 1, num_frames len).
 * Built: hidden 128 / 256 / 384 / 512 with planes = 1 and elem_type AMTX_T_BF16, or planes = 2 and AMTX_T_F32; anything else is
 * AMTX_ERR_UNSUPPORTED.  Rows of [0, total_rows) that no sequence names are not written. */
int amtx_bilstm_seq_fwd(const void* xproj, const uint16_t* whh_packed, int hidden, int planes, int elem_type, void* out,
                        const int64_t* seqs_host, const int64_t* seqs_dev, int num_seqs, int64_t total_rows, int groups, void* stream);

/* For every clip b < batch: rows [src_first_b, src_first_b + count_b) of the row-major src [batch][num_frames][width_bytes] become rows
 * dst_row_b ... of dst [total_rows][width_bytes]; with planes = 2 the same for a second plane src_plane_bytes / dst_plane_bytes further on.
 * Bit patterns are copied, 16 bytes at a time: AMTX_ERR_ARG for a width or plane stride that is no multiple of 16 bytes, a pointer that is
 * not aligned to 16, and for a table row with a negative entry, src_first + count > num_frames or dst_row + count > total_rows.  Every
 * named destination row is written once, nothing else is written; no atomics.  Destination ranges that overlap are the caller's to avoid. */
int amtx_rows_gather(const void* src, int batch, int64_t num_frames, int64_t width_bytes, int planes, int64_t src_plane_bytes,
                     const int64_t* table_host, const int64_t* table_dev, void* dst, int64_t total_rows, int64_t dst_plane_bytes, void* stream);

/* amtx_pianoroll_fwd over packed rows: sequence s gets its own contiguous [keys][len_s] map at element keys * row0_s of `out` (the layout
 * of amt_tools_amd.tracks.TrackMaps): out[keys * row0 + k * len + t] = f(logits[(row0 + t) * ld + col0 + k]), f as for amtx_pianoroll_fwd
 * (threshold < 0: the sigmoid itself). */
int amtx_pianoroll_seq(const float* logits, int64_t ld, int col0, const int64_t* seqs_host, const int64_t* seqs_dev, int num_seqs,
                       int64_t total_rows, int keys, float threshold, float* out, void* stream);

/* ---- the engine in two phases ------------------------------------------------------------------------------------------------------
 * ACOUSTIC PHASE, on `batch` clips of `num_frames` frames: the convolution stack, the fc1 GEMM of the recurrent heads and the pitch
 * head's folded GEMM -- the launches of amtx_of_forward on the workspace of amtx_of_workspace_bytes(model, batch, num_frames) -- then the
 * kept rows of every clip (gather table) into two caller-owned packed buffers:
 *   rows_e      amtx_of_rows_e_bytes(model, total_rows) bytes: the recurrent heads' fc1 output in the engine's activation format,
 *               [heads][total_rows][dim_am] (a two-plane model: [2 planes][heads][total_rows][dim_am] 16-bit)
 *   rows_pitch  [total_rows][n_out] float32: the pitch head's logits
 * The three entry points take the three input forms of amtx_of_forward / _power / _feats16. */
size_t amtx_of_rows_e_bytes(const amtx_of_model* model, int64_t total_rows);
int amtx_of_acoustic_rows(const amtx_of_model* model, const float* feats, int64_t stride_b, int64_t stride_c, int64_t stride_t, int64_t stride_f,
                          int batch, int num_frames, void* workspace, size_t workspace_bytes, const int64_t* table_host, const int64_t* table_dev,
                          int64_t total_rows, void* rows_e, float* rows_pitch, void* stream);
int amtx_of_acoustic_rows_power(const amtx_of_model* model, const float* power, int64_t stride_b, int64_t stride_t, int64_t stride_f,
                                const float* clip_max, const float* ref, int batch, int num_frames, void* workspace, size_t workspace_bytes,
                                const int64_t* table_host, const int64_t* table_dev, int64_t total_rows, void* rows_e, float* rows_pitch,
                                void* stream);
int amtx_of_acoustic_rows_feats16(const amtx_of_model* model, const void* feats16, int batch, int num_frames, void* workspace,
                                  size_t workspace_bytes, const int64_t* table_host, const int64_t* table_dev, int64_t total_rows, void* rows_e,
                                  float* rows_pitch, void* stream);

/* LANGUAGE PHASE, on total_rows packed rows that hold num_seqs whole tracks: the recurrent heads' input projection, their packed
 * recurrence, their LogisticBanks, the refinement stage's input projection, recurrence and LogisticBank.  Piano rolls in the packed
 * layout of amtx_pianoroll_seq: out_onsets / out_multi_pitch thresholded at 0.5, out_offsets (a model with an offset head) as
 * probabilities; each may be null.  logits_*: optional raw logits, packed [total_rows][n_out] float32.  The workspace
 * (amtx_of_language_workspace_bytes(model, total_rows) bytes, 256-byte aligned) is the phase's own. */
size_t amtx_of_language_workspace_bytes(const amtx_of_model* model, int64_t total_rows);
int amtx_of_language_rows(const amtx_of_model* model, const void* rows_e, const float* rows_pitch, const int64_t* seqs_host,
                          const int64_t* seqs_dev, int num_seqs, int64_t total_rows, void* workspace, size_t workspace_bytes, float* out_onsets,
                          float* out_multi_pitch, float* out_offsets, float* logits_onsets, float* logits_multi_pitch, float* logits_offsets,
                          void* stream);

#ifdef __cplusplus
}
#endif

#endif /* AMTX_OFSEQ_H */
