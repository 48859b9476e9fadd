// Validation losses summed per clip over a frame window of each clip (include/amtx_cliploss.h; amt_tools_amd/cliploss.py).
//   amtx_bce_clip_sums             LogisticBank.get_loss without its means:  sums[b] = sum_k w_k sum_{t in window_b} BCEWithLogits
//   amtx_softmax_groups_clip_sums  SoftmaxGroups.get_loss without its means: sums[b] = sum_{t in window_b} sum_g w[g][y] NLL
// Two launches each.  First level: a block owns a tile of ONE clip, evaluates its terms in float32 (the expressions of bce_loss_kernel,
// head.hip, and sm_loss_kernel, tabtrain.hip), adds them in float64 -- thread, wave butterfly, (w0 + w1) + (w2 + w3) -- and writes one
// float64 partial; a block whose frames all lie outside the clip's window writes 0.0 and reads nothing else.  Second level: one wave per
// clip adds the clip's partials in a fixed order.  Deterministic, no atomics, nothing cleared beforehand.
//   BCE: the labels arrive key-major, the logits frame-major: a 32 x 32 LDS transpose keeps both streams coalesced.
//   softmax: a tile's logit rows are staged in LDS by coalesced row reads (odd row stride: the per-(frame, group) threads of a wave, frame
//   fastest, read different banks); the targets are read with the frame fastest, 8 contiguous bytes per lane.
#include "amtx_common.h"
#include "../../include/amtx_cliploss.h"

#define CLIPLOSS_SM_LDS 8224             // floats of LDS for a softmax tile: 32 frames of 256 (+1) logits; fewer frames for wider heads
#define CLIPLOSS_SM_MAX_GC 8192

namespace {

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// the block's sum, valid in thread 0: fixed order
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
    v = wave_sum_f64(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// grid (frame tiles, key tiles, clips); partial[(b * gridDim.y + ky) * gridDim.x + kt]
__global__ __launch_bounds__(256) void bce_clip_partials_kernel(const float* __restrict__ logits, int64_t ld, const float* __restrict__ labels,
                                                                const float* __restrict__ weight, const int32_t* __restrict__ frames, int T,
                                                                int keys, double* __restrict__ partial) {
    __shared__ float tile[32][33];
    __shared__ double red[4];
    const int b = blockIdx.z;
    const int t0 = blockIdx.x * 32, k0 = blockIdx.y * 32;
    const int lo = frames ? frames[2 * b] : 0;                                   // block-uniform
    const int hi = frames ? min(lo + frames[2 * b + 1], T) : T;                  // (the host copy was checked; no read past the clip either way)
    double* out = partial + ((int64_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    if (t0 >= hi || t0 + 32 <= lo) {                                             // (count 0: hi == lo, every block leaves here)
        if (threadIdx.x == 0) *out = 0.0;
        return;
    }
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = k0 + ty + 8 * i, t = t0 + tx;
        tile[ty + 8 * i][tx] = (t >= lo && t < hi && k < keys) ? labels[((int64_t)b * keys + k) * T + t] : 0.f;
    }
    __syncthreads();
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int t = t0 + ty + 8 * i, k = k0 + tx;
        if (t >= lo && t < hi && k < keys) {
            const float x = logits[((int64_t)b * T + t) * ld + k];
            const float y = tile[tx][ty + 8 * i];
            const float w = weight ? weight[k] : 1.0f;
            acc += (double)(w * (fmaxf(x, 0.f) - x * y + log1pf(expf(-fabsf(x)))));
        }
    }
    acc = block_sum_f64(acc, red);
    if (threadIdx.x == 0) *out = acc;
}

// grid (frame tiles, clips); a tile is `tt` frames; partial[b * gridDim.x + kt].  stride: floats between two staged rows (odd, >= GC)
__global__ __launch_bounds__(256) void sm_clip_partials_kernel(const float* __restrict__ logits, int64_t ld, const int64_t* __restrict__ targets,
                                                               const float* __restrict__ weight, const int32_t* __restrict__ frames, int T, int G,
                                                               int C, int tt, int stride, double* __restrict__ partial) {
    __shared__ float rows[CLIPLOSS_SM_LDS];
    __shared__ double red[4];
    const int b = blockIdx.y;
    const int t0 = blockIdx.x * tt;
    const int lo = frames ? frames[2 * b] : 0;
    const int hi = frames ? lo + frames[2 * b + 1] : T;
    double* out = partial + (int64_t)b * gridDim.x + blockIdx.x;
    if (t0 >= hi || t0 + tt <= lo) {
        if (threadIdx.x == 0) *out = 0.0;
        return;
    }
    const int first = max(t0, lo), last = min(min(t0 + tt, hi), T);              // the tile's frames inside the window: [first, last)
    const int GC = G * C, n = last - first;
    for (int i = threadIdx.x; i < n * GC; i += 256) {
        const int r = i / GC, c = i - r * GC;
        rows[r * stride + c] = logits[((int64_t)b * T + first + r) * ld + c];
    }
    __syncthreads();
    double acc = 0.0;
    for (int i = threadIdx.x; i < n * G; i += 256) {
        const int g = i / n, r = i - g * n;                                       // the frame runs fastest
        const float* x = rows + r * stride + g * C;
        int64_t tg = targets[((int64_t)b * G + g) * T + first + r];
        if (tg == -1) tg = C - 1;
        const bool bad = tg < 0 || tg >= C;
        const int tgt = bad ? 0 : (int)tg;
        float m = x[0];
        for (int c = 1; c < C; ++c) m = fmaxf(m, x[c]);
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += expf(x[c] - m);
        const float w = bad ? __builtin_nanf("") : (weight ? weight[g * C + tgt] : 1.0f);
        acc += (double)(w * (m + logf(s) - x[tgt]));
    }
    acc = block_sum_f64(acc, red);
    if (threadIdx.x == 0) *out = acc;
}

// sums[b] = partial[b * n .. b * n + n) added up: lane l takes l, l + 64, ... in order, then the butterfly
__global__ __launch_bounds__(64) void clip_sums_kernel(const double* __restrict__ partial, int64_t n, double* __restrict__ sums) {
    const double* p = partial + (int64_t)blockIdx.x * n;
    double a = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 64) a += p[i];
    a = wave_sum_f64(a);
    if (threadIdx.x == 0) sums[blockIdx.x] = a;
}

// frames per softmax tile and the staged row stride for a head of gc logits
void sm_tile(int gc, int* tt, int* stride) {
    *stride = gc | 1;
    const int fit = CLIPLOSS_SM_LDS / *stride;
    *tt = fit > 32 ? 32 : fit;
}

int64_t bce_partials_per_clip(int num_frames, int keys) { return (int64_t)((num_frames + 31) / 32) * ((keys + 31) / 32); }

// what the two entry points share: pointers, alignment, the window tables
int check_common(const char* who, const void* logits, const void* labels, const int32_t* frames_host, const int32_t* frames_dev, int batch,
                 int num_frames, const double* sums, const void* workspace) {
    AMTX_REQUIRE(logits && labels && sums && workspace, "%s: null pointer", who);
    AMTX_REQUIRE((frames_host == nullptr) == (frames_dev == nullptr), "%s: the window table is passed twice, on the host and on the device, or not at all", who);
    AMTX_REQUIRE(batch >= 1 && batch <= 65535 && num_frames >= 1, "%s: batch=%d (1 .. 65535), num_frames=%d (at least 1)", who, batch, num_frames);
    AMTX_REQUIRE(((uintptr_t)sums % 8) == 0 && ((uintptr_t)workspace % 8) == 0, "%s: sums and workspace must be aligned to 8 bytes", who);
    if (frames_host)
        for (int b = 0; b < batch; b++) {
            const int64_t first = frames_host[2 * b], count = frames_host[2 * b + 1];
            AMTX_REQUIRE(first >= 0 && count >= 0, "%s: clip %d: a negative entry in the window {%lld, %lld}", who, b, (long long)first, (long long)count);
            AMTX_REQUIRE(first + count <= num_frames, "%s: clip %d: frames [%lld, %lld + %lld) leave the clip's %d frames", who, b, (long long)first,
                         (long long)first, (long long)count, num_frames);
        }
    return AMTX_OK;
}

}  // namespace

extern "C" size_t amtx_bce_clip_sums_workspace_bytes(int batch, int num_frames, int keys) {
    if (batch <= 0 || num_frames <= 0 || keys <= 0) return 0;
    return (size_t)batch * (size_t)bce_partials_per_clip(num_frames, keys) * sizeof(double);
}

extern "C" int amtx_bce_clip_sums(const float* logits, int64_t ld, const float* labels, const float* weight, const int32_t* frames_host,
                                  const int32_t* frames_dev, int batch, int num_frames, int keys, double* sums, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    const int rc = check_common("amtx_bce_clip_sums", logits, labels, frames_host, frames_dev, batch, num_frames, sums, workspace);
    if (rc != AMTX_OK) return rc;
    AMTX_REQUIRE(keys >= 1 && ld >= keys, "amtx_bce_clip_sums: keys=%d (at least 1), ld=%lld (at least keys)", keys, (long long)ld);
    AMTX_REQUIRE((keys + 31) / 32 <= 65535, "amtx_bce_clip_sums: keys=%d: at most 65535 tiles of 32", keys);
    AMTX_REQUIRE(workspace_bytes >= amtx_bce_clip_sums_workspace_bytes(batch, num_frames, keys), "amtx_bce_clip_sums: workspace too small (%zu of %zu bytes)",
                 workspace_bytes, amtx_bce_clip_sums_workspace_bytes(batch, num_frames, keys));
    hipStream_t s = (hipStream_t)stream;
    double* partial = static_cast<double*>(workspace);
    const dim3 grid((unsigned)((num_frames + 31) / 32), (unsigned)((keys + 31) / 32), (unsigned)batch);
    hipLaunchKernelGGL(bce_clip_partials_kernel, grid, dim3(256), 0, s, logits, ld, labels, weight, frames_dev, num_frames, keys, partial);
    AMTX_CHECK_LAUNCH();
    hipLaunchKernelGGL(clip_sums_kernel, dim3((unsigned)batch), dim3(64), 0, s, (const double*)partial, bce_partials_per_clip(num_frames, keys), sums);
    AMTX_CHECK_LAUNCH();
    return AMTX_OK;
}

extern "C" size_t amtx_softmax_groups_clip_sums_workspace_bytes(int batch, int num_frames, int num_groups, int num_classes) {
    if (batch <= 0 || num_frames <= 0 || num_groups <= 0 || num_classes <= 0 || (int64_t)num_groups * num_classes > CLIPLOSS_SM_MAX_GC) return 0;
    int tt, stride;
    sm_tile(num_groups * num_classes, &tt, &stride);
    return (size_t)batch * (size_t)((num_frames + tt - 1) / tt) * sizeof(double);
}

extern "C" int amtx_softmax_groups_clip_sums(const float* logits, int64_t ld, const int64_t* targets, const float* weight, const int32_t* frames_host,
                                             const int32_t* frames_dev, int batch, int num_frames, int num_groups, int num_classes, double* sums,
                                             void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = check_common("amtx_softmax_groups_clip_sums", logits, targets, frames_host, frames_dev, batch, num_frames, sums, workspace);
    if (rc != AMTX_OK) return rc;
    AMTX_REQUIRE(num_groups >= 1 && num_classes >= 1, "amtx_softmax_groups_clip_sums: num_groups=%d, num_classes=%d: at least one each", num_groups, num_classes);
    const int64_t gc = (int64_t)num_groups * num_classes;
    AMTX_REQUIRE(ld >= gc, "amtx_softmax_groups_clip_sums: ld=%lld (at least num_groups x num_classes = %lld)", (long long)ld, (long long)gc);
    if (gc > CLIPLOSS_SM_MAX_GC) {
        amtx_set_error("amtx_softmax_groups_clip_sums: num_groups x num_classes = %lld (at most %d are built)", (long long)gc, CLIPLOSS_SM_MAX_GC);
        return AMTX_ERR_UNSUPPORTED;
    }
    const size_t need = amtx_softmax_groups_clip_sums_workspace_bytes(batch, num_frames, num_groups, num_classes);
    AMTX_REQUIRE(workspace_bytes >= need, "amtx_softmax_groups_clip_sums: workspace too small (%zu of %zu bytes)", workspace_bytes, need);
    int tt, stride;
    sm_tile((int)gc, &tt, &stride);
    const int tiles = (num_frames + tt - 1) / tt;
    hipStream_t s = (hipStream_t)stream;
    double* partial = static_cast<double*>(workspace);
    hipLaunchKernelGGL(sm_clip_partials_kernel, dim3((unsigned)tiles, (unsigned)batch), dim3(256), 0, s, logits, ld, targets, weight, frames_dev,
                       num_frames, num_groups, num_classes, tt, stride, partial);
    AMTX_CHECK_LAUNCH();
    hipLaunchKernelGGL(clip_sums_kernel, dim3((unsigned)batch), dim3(64), 0, s, (const double*)partial, (int64_t)tiles, sums);
    AMTX_CHECK_LAUNCH();
    return AMTX_OK;
}
