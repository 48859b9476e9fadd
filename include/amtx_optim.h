/*
 * amtx -- C ABI, fifth header: the parameter update of a training step, Adam and Adadelta over a table of tensors in one launch.
 *
 * Same conventions as include/amtx.h (extern "C", caller-owned DEVICE pointers unless a parameter says host, explicit stream as void*,
 * int return, message via amtx_last_error()), same library (libamtx.so), same binding (amt_tools_amd/_lib.py, HEADERS).  The tables
 * pinned for the earlier headers stay as they are; this header's functions are pinned in tests/golden/abi_signatures_optim.json.
 *
 * TENSOR TABLE: a HOST array int64 [num_tensors][5] = {param, grad, state_a, state_b, numel}, the four addresses as integers.  Every
 * tensor is float32 and dense: `numel` consecutive elements from each address, the same element order in all four.  An address need
 * only be 4-byte aligned; a tensor whose four addresses are all 16-byte aligned is updated with 16-byte loads and stores.  numel 0 is
 * legal: the tensor is skipped and its addresses are not looked at.  The table travels to the kernel as a kernel argument, so the
 * entry points read it on the calling thread and neither copy it to the device nor wait for the device.
 *
 * Adam: state_a = exp_avg, state_b = exp_avg_sq.  Adadelta: state_a = square_avg, state_b = acc_delta.  The gradient sum of squares
 * reads column 1 and column 4 alone.
 *
 * One launch serves at most AMTX_OPTIM_MAX_TENSORS tensors; a longer table is dealt to several launches by the entry point itself.
 * Every element of param and of the two state maps is read and written by exactly one lane; gradients are only read.  No atomics.
 */
#ifndef AMTX_OPTIM_H
#define AMTX_OPTIM_H

#include "amtx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Most tensors one launch serves. */
#define AMTX_OPTIM_MAX_TENSORS 72
/* Elements of one tensor a block owns. */
#define AMTX_OPTIM_CHUNK 4096

/* Launches a table with these numels (HOST array) takes: consecutive tensors, at most AMTX_OPTIM_MAX_TENSORS per launch; a run of
 * tensors that holds no element is no launch.  Negative: an argument error. */
int amtx_optim_num_launches(const int64_t* numels, int64_t num_tensors);

/* Blocks of all those launches together = the floats of `partials` amtx_optim_grad_sumsq needs.  Negative: an argument error. */
int64_t amtx_optim_num_blocks(const int64_t* numels, int64_t num_tensors);

/* out[0] = the sum of g * g over every gradient of the table, out[1] = its square root (the global gradient norm).  Each block writes
 * the sum of its chunk to `partials` (partials_elems floats, at least amtx_optim_num_blocks), then one block adds the partials in a
 * fixed order: the same bits on every run, whatever partials held before.  An empty table writes two zeros. */
int amtx_optim_grad_sumsq(const int64_t* table, int64_t num_tensors, float* partials, int64_t partials_elems, float* out, void* stream);

/* torch.optim.Adam (amsgrad off, maximize off), in place:
 *     g += weight_decay * p;  m = lerp(m, g, 1 - beta1);  v = beta2 * v + (1 - beta2) * g * g;
 *     p -= step_size * m / (sqrt(v) / bias_correction2_sqrt + eps)
 * step_size = lr / (1 - beta1^step) and bias_correction2_sqrt = sqrt(1 - beta2^step) are the caller's, in double precision.
 * sumsq: null, or a DEVICE float holding the sum of squares of all gradients (amtx_optim_grad_sumsq's out): every gradient read is
 * then scaled by min(1, max_norm / (sqrt(*sumsq) + 1e-6)), torch.nn.utils.clip_grad_norm_'s coefficient; the gradient tensors are
 * not written.  Returns the number of launches. */
int amtx_optim_adam_step(const int64_t* table, int64_t num_tensors, double step_size, double bias_correction2_sqrt, double beta1,
                         double beta2, double eps, double weight_decay, const float* sumsq, double max_norm, void* stream);

/* torch.optim.Adadelta (maximize off), in place:
 *     g += weight_decay * p;  sq = rho * sq + (1 - rho) * g * g;  delta = sqrt(acc + eps) / sqrt(sq + eps) * g;
 *     acc = rho * acc + (1 - rho) * delta * delta;  p -= lr * delta
 * sumsq / max_norm as above.  Returns the number of launches. */
int amtx_optim_adadelta_step(const int64_t* table, int64_t num_tensors, double lr, double rho, double eps, double weight_decay,
                             const float* sumsq, double max_norm, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* AMTX_OPTIM_H */
