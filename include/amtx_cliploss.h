/*
 * amtx -- C ABI, eighth header: validation losses summed PER CLIP, over a frame window of each clip.
 *
 * Same conventions as include/amtx.h (extern "C", caller-owned DEVICE pointers unless a parameter says host, explicit stream as void*,
 * int return, message via amtx_last_error()), same library (libamtx.so), same binding (amt_tools_amd/_lib.py, HEADERS).  The tables
 * pinned for the earlier headers stay as they are; this header's functions are pinned in tests/golden/abi_signatures_cliploss.json.
 *
 * amtx_bce_logits_loss and amtx_softmax_groups_loss (include/amtx.h) answer ONE number, the mean over a batch: the training loss.
 * A validation loop wants one number per clip -- the reference's loss of that clip as a batch of one is sum_k mean_t, that is
 * sums[b] / count_b -- and, for a track stitched from overlapped clips, the sum over the kept frames of every clip:
 *     loss(track) = (1 / L) * sum over the track's clips of sums[clip]          (windows that cover every frame of the track once)
 * The functions here produce those sums in float64.  No gradient, no mean: the caller divides.
 *
 * WINDOWS: int32 [batch][2] = {first, count}, once on the host and once on the device (the convention of amtx_stitch_clips): the entry
 * point checks every row of the HOST copy before anything is launched, the kernel reads the DEVICE copy, and the caller keeps the two
 * equal.  Both pointers NULL: every clip's window is {0, num_frames}.  One of the two NULL: AMTX_ERR_ARG.
 *
 * REDUCTION ORDER (fixed: the same arguments give the same bits): every term is evaluated in float32 in the form of the batch-mean
 * kernels; a thread adds its terms in float64, a wave adds its lanes with a fixed shuffle butterfly, a block adds its four waves as
 * (w0 + w1) + (w2 + w3) and writes one float64 partial into the workspace; one wave per clip then adds the clip's partials, lane l
 * taking partials l, l + 64, ... in order, and its lanes with the same butterfly.  No atomics.  Every element of sums and every partial
 * the second level reads is written by the call: neither sums nor the workspace needs to be cleared, and their old contents are never
 * read.  A block whose frames all lie outside its clip's window writes 0.0 and reads neither logits nor labels.
 */
#ifndef AMTX_CLIPLOSS_H
#define AMTX_CLIPLOSS_H

#include "amtx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* LogisticBank.get_loss (amt_tools/models/common.py:541-584) without its means:
 *     sums[b] = sum_k weight[k] * sum_{first_b <= t < first_b + count_b} BCEWithLogits(logits[b][t][k], labels[b][k][t])
 * with the stable form max(x, 0) - x * y + log1p(exp(-|x|)) of amtx_bce_logits_loss and torch.
 *   logits       [batch][num_frames][keys] fp32, rows ld >= keys elements apart
 *   labels       [batch][keys][num_frames] fp32, contiguous
 *   weight       [keys] fp32 or NULL (all ones)
 *   frames_host  HOST int32 [batch][2], frames_dev its device copy; both NULL = whole clips
 *   sums         [batch] float64, 8-byte aligned; count_b == 0 writes 0.0
 *   workspace    amtx_bce_clip_sums_workspace_bytes(batch, num_frames, keys) bytes, 8-byte aligned
 * AMTX_ERR_ARG, with nothing launched and nothing written: a null logits / labels / sums / workspace, one window table of the two,
 * batch, num_frames or keys below 1, batch above 65535, ld < keys, a misaligned sums or workspace, a workspace that is too small, and a
 * window row with a negative entry or first + count > num_frames (the message names the clip). */
size_t amtx_bce_clip_sums_workspace_bytes(int batch, int num_frames, int keys);
int amtx_bce_clip_sums(const float* logits, int64_t ld, const float* labels, const float* weight, const int32_t* frames_host,
                       const int32_t* frames_dev, int batch, int num_frames, int keys, double* sums, void* workspace, size_t workspace_bytes,
                       void* stream);

/* SoftmaxGroups.get_loss (amt_tools/models/common.py:369-440) without its means:
 *     sums[b] = sum_{first_b <= t < first_b + count_b} sum_g w[g][y] * (logsumexp_c logits[b][t][g*C + c] - logits[b][t][g*C + y]),
 *     y = targets[b][g][t], with -1 standing for the last class C - 1; w = 1 without weight.
 *   logits   [batch][num_frames][num_groups * num_classes] fp32, rows ld >= num_groups * num_classes elements apart
 *   targets  [batch][num_groups][num_frames] int64, contiguous
 *   weight   [num_groups * num_classes] fp32 or NULL
 * A target outside [-1, C) is handled as amtx_softmax_groups_loss handles it: its term is NaN (the reference raises on it), so sums[b]
 * of a clip that has one INSIDE its window is NaN; outside the window it is never read.  The other clips are not affected.
 * frames_host, frames_dev, sums, workspace and the refusals as above (workspace: amtx_softmax_groups_clip_sums_workspace_bytes);
 * AMTX_ERR_UNSUPPORTED for num_groups * num_classes above 8192 (a frame's logits are staged in LDS). */
size_t amtx_softmax_groups_clip_sums_workspace_bytes(int batch, int num_frames, int num_groups, int num_classes);
int amtx_softmax_groups_clip_sums(const float* logits, int64_t ld, const int64_t* targets, const float* weight, const int32_t* frames_host,
                                  const int32_t* frames_dev, int batch, int num_frames, int num_groups, int num_classes, double* sums,
                                  void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* AMTX_CLIPLOSS_H */
