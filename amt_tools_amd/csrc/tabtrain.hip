// TabCNN training on shared-window sequences (amt_tools/models/tabcnn.py:140-180 and SoftmaxGroups.get_loss,
// amt_tools/models/common.py:369-440, in train mode): the amtx_tab_pool_train_* and amtx_softmax_groups_loss ABI of include/amtx.h.
//
// The three 3x3 convolutions run once per zero-padded sequence as padded ("same") convolutions on train.hip's implicit GEMMs
// (amt_tools_amd/models.py, TabCNN._forward_hip_train): valid conv k at (row r, column v) is "same" conv k at (r + k, v + k), so
// window t's 2x2 pool reads conv3's "same" map at rows {2h+3, 2h+4} and columns {t+3, t+4}.  The kernels here are that pool, forward
// and backward, and the grouped softmax loss.  Everything is deterministic: no atomics, fixed summation orders.
//
//   tab_pool_fwd   conv3 map (any strides) -> ReLU + 2x2 max -> fc's input rows x[b*T + t][c*H + h] (the reference's channel-major
//                  flatten, tabcnn.py:172-175) + one uint8 record per output: winner (0..3, row-major in the window, first on ties as
//                  max_pool2d picks) | 4 when the max was > 0
//   tab_pool_bwd   dx -> d(conv3 map) as a gather: each map position collects from the at most two windows (t = col-3, col-4) whose
//                  recorded winner it is, ReLU's mask applied; every element is written (no memset)
//   sm_loss        log-softmax per (frame, group) -> weighted NLL of the labelled class -> one partial per block, d loss / d logits
#include "amtx_kernels.h"

namespace {

constexpr int POOL_HT = 16;   // pooled rows (h) per tile = 32 map rows
constexpr int POOL_CT = 64;   // channels per tile

// grid (B*T, ceil(H / POOL_HT), ceil(C / POOL_CT)).  Reads: channel-fastest (coalesced on a channels-last map); writes: h-fastest
// runs of fc's input rows, through an LDS transpose.
__global__ __launch_bounds__(256) void tab_pool_fwd_kernel(const float* __restrict__ map, int64_t sb, int64_t sc, int64_t scol, int64_t sf,
                                                           int T, int C, int H, float* __restrict__ x, uint8_t* __restrict__ rec) {
    __shared__ float val[POOL_CT][POOL_HT + 1];
    __shared__ uint8_t win[POOL_CT][POOL_HT + 1];
    const int64_t row = blockIdx.x;
    const int b = (int)(row / T), t = (int)(row - (int64_t)b * T);
    const int h0 = blockIdx.y * POOL_HT, c0 = blockIdx.z * POOL_CT;
    const float* base = map + (int64_t)b * sb + (int64_t)(t + 3) * scol;
    for (int j = threadIdx.x; j < POOL_HT * POOL_CT; j += 256) {
        const int c = j % POOL_CT, hh = j / POOL_CT;
        const int h = h0 + hh, cc = c0 + c;
        float v = 0.f;
        uint8_t code = 0;
        if (h < H && cc < C) {
            const float* p = base + (int64_t)cc * sc + (int64_t)(2 * h + 3) * sf;
            const float q[4] = {p[0], p[scol], p[sf], p[sf + scol]};   // row-major window order: (2h+3, t+3) (2h+3, t+4) (2h+4, t+3) (2h+4, t+4)
            float best = q[0];
            int k = 0;
#pragma unroll
            for (int i = 1; i < 4; ++i)
                if (q[i] > best || __builtin_isnan(q[i])) {   // strict: ties keep the first; NaN propagates as in max_pool2d
                    best = q[i];
                    k = i;
                }
            v = best > 0.f ? best : (__builtin_isnan(best) ? best : 0.f);
            code = (uint8_t)(k | (best > 0.f ? 4 : 0));
        }
        val[c][hh] = v;
        win[c][hh] = code;
    }
    __syncthreads();
    const int64_t ld = (int64_t)C * H;
    for (int j = threadIdx.x; j < POOL_HT * POOL_CT; j += 256) {
        const int hh = j % POOL_HT, c = j / POOL_HT;
        const int h = h0 + hh, cc = c0 + c;
        if (h < H && cc < C) {
            const int64_t o = row * ld + (int64_t)cc * H + h;
            x[o] = val[c][hh];
            rec[o] = win[c][hh];
        }
    }
}

// grid (B*cols, ceil((F-3) / (2*POOL_HT)), ceil(C / POOL_CT)).  Block (b, col, k) owns map rows f = 3 + 32k .. 3 + 32k + 31 of column
// col (pooled rows h = 16k .. 16k + 15) and, for k == 0, the border rows f = 0, 1, 2.  dmap is channels-last [b][col][f][c].
__global__ __launch_bounds__(256) void tab_pool_bwd_kernel(const float* __restrict__ dx, const uint8_t* __restrict__ rec, int T, int cols, int F,
                                                           int C, int H, float* __restrict__ dmap) {
    __shared__ float g[2][POOL_CT][POOL_HT + 1];
    __shared__ uint8_t r[2][POOL_CT][POOL_HT + 1];
    const int64_t bc = blockIdx.x;
    const int b = (int)(bc / cols), col = (int)(bc - (int64_t)b * cols);
    const int k = blockIdx.y, h0 = k * POOL_HT, c0 = blockIdx.z * POOL_CT;
    const int64_t ld = (int64_t)C * H;
    // s = 0: window t = col - 3 reads this column as its first pooled column; s = 1: window t = col - 4, second pooled column
    for (int j = threadIdx.x; j < 2 * POOL_CT * POOL_HT; j += 256) {
        const int hh = j % POOL_HT, c = (j / POOL_HT) % POOL_CT, s = j / (POOL_HT * POOL_CT);
        const int t = col - 3 - s, h = h0 + hh, cc = c0 + c;
        float gv = 0.f;
        uint8_t rv = 0;
        if (t >= 0 && t < T && h < H && cc < C) {
            const int64_t o = ((int64_t)b * T + t) * ld + (int64_t)cc * H + h;
            gv = dx[o];
            rv = rec[o];
        }
        g[s][c][hh] = gv;
        r[s][c][hh] = rv;
    }
    __syncthreads();
    float* out = dmap + bc * F * C;
    for (int j = threadIdx.x; j < 2 * POOL_HT * POOL_CT; j += 256) {
        const int c = j % POOL_CT, ui = j / POOL_CT;
        const int f = 3 + 2 * h0 + ui, cc = c0 + c;
        if (f < F && cc < C) {
            const int hh = ui >> 1, dr = ui & 1;
            float acc = 0.f;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int rv = r[s][c][hh];
                if ((rv & 4) && (rv & 3) == 2 * dr + s) acc += g[s][c][hh];
            }
            out[(int64_t)f * C + cc] = acc;
        }
    }
    if (k == 0)
        for (int j = threadIdx.x; j < 3 * POOL_CT; j += 256) {
            const int c = j % POOL_CT, f = j / POOL_CT, cc = c0 + c;
            if (f < F && cc < C) out[(int64_t)f * C + cc] = 0.f;
        }
}

// One thread per (frame row, group): logits[row*ld + g*C .. + C-1], target = targets[(b*G + g)*T + t] (-1 -> C-1).
//   term = w[g][tgt] * (logsumexp - x[tgt]);   grad[row][g*C + c] = w[g][tgt] * (softmax_c - [c == tgt]) / (B*T)
// A target outside [-1, C) makes its term and gradient NaN (the reference raises on it).
__global__ __launch_bounds__(256) void sm_loss_kernel(const float* __restrict__ logits, int64_t ld, const int64_t* __restrict__ targets,
                                                      const float* __restrict__ weight, int T, int G, int C, int64_t pairs, float inv_bt,
                                                      float* __restrict__ grad, float* __restrict__ partial) {
    __shared__ float red[4];
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float term = 0.f;
    if (p < pairs) {
        const int64_t row = p / G;
        const int g = (int)(p - row * G);
        const int b = (int)(row / T), t = (int)(row - (int64_t)b * T);
        const float* x = logits + row * ld + (int64_t)g * C;
        int64_t tg = targets[((int64_t)b * G + g) * T + t];
        if (tg == -1) tg = C - 1;
        const bool bad = tg < 0 || tg >= C;
        const int tgt = bad ? 0 : (int)tg;
        float m = x[0];
        for (int c = 1; c < C; ++c) m = fmaxf(m, x[c]);
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += expf(x[c] - m);
        const float w = bad ? __builtin_nanf("") : (weight ? weight[g * C + tgt] : 1.0f);
        term = w * (m + logf(s) - x[tgt]);
        if (grad) {
            float* d = grad + row * ((int64_t)G * C) + (int64_t)g * C;
            const float scale = w * inv_bt, inv_s = 1.0f / s;
            for (int c = 0; c < C; ++c) d[c] = scale * (expf(x[c] - m) * inv_s - (c == tgt ? 1.0f : 0.0f));
        }
    }
    term = wave_sum_f32(term);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = term;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

int64_t sm_loss_blocks(int batch, int num_frames, int num_groups) { return ((int64_t)batch * num_frames * num_groups + 255) / 256; }

}  // namespace

// ---- TabCNN.conv's last ReLU + MaxPool2d((2, 2)) + flatten (tabcnn.py:172-175) over a shared-window conv3 map, train mode
extern "C" int amtx_tab_pool_train_fwd(const float* map, int64_t stride_b, int64_t stride_c, int64_t stride_col, int64_t stride_f, int batch,
                                       int channels, int num_bins, int num_windows, float* x, uint8_t* record, void* stream) {
    AMTX_REQUIRE(map && x && record, "amtx_tab_pool_train_fwd: null pointer");
    AMTX_REQUIRE(batch > 0 && channels > 0 && num_windows > 0 && num_bins >= 8, "amtx_tab_pool_train_fwd: bad sizes (batch %d, channels %d, "
                 "num_bins %d >= 8, num_windows %d)", batch, channels, num_bins, num_windows);
    AMTX_REQUIRE(stride_b >= 0 && stride_c >= 0 && stride_col >= 0 && stride_f >= 0, "amtx_tab_pool_train_fwd: negative stride");
    const int H = (num_bins - 6) / 2;
    AMTX_REQUIRE((int64_t)batch * num_windows < (1ll << 31) && (int64_t)channels * H < (1ll << 31) && channels <= 65535 * POOL_CT,
                 "amtx_tab_pool_train_fwd: too large");
    dim3 grid((unsigned)((int64_t)batch * num_windows), (unsigned)((H + POOL_HT - 1) / POOL_HT), (unsigned)((channels + POOL_CT - 1) / POOL_CT));
    hipLaunchKernelGGL(tab_pool_fwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, map, stride_b, stride_c, stride_col, stride_f, num_windows,
                       channels, H, x, record);
    AMTX_CHECK_LAUNCH();
    return AMTX_OK;
}

extern "C" int amtx_tab_pool_train_bwd(const float* dx, const uint8_t* record, int batch, int channels, int num_bins, int num_windows, float* dmap,
                                       void* stream) {
    AMTX_REQUIRE(dx && record && dmap, "amtx_tab_pool_train_bwd: null pointer");
    AMTX_REQUIRE(batch > 0 && channels > 0 && num_windows > 0 && num_bins >= 8, "amtx_tab_pool_train_bwd: bad sizes (batch %d, channels %d, "
                 "num_bins %d >= 8, num_windows %d)", batch, channels, num_bins, num_windows);
    const int H = (num_bins - 6) / 2, cols = num_windows + 8;
    AMTX_REQUIRE((int64_t)batch * cols < (1ll << 31) && (int64_t)channels * H < (1ll << 31) && channels <= 65535 * POOL_CT,
                 "amtx_tab_pool_train_bwd: too large");
    dim3 grid((unsigned)((int64_t)batch * cols), (unsigned)((num_bins - 3 + 2 * POOL_HT - 1) / (2 * POOL_HT)),
              (unsigned)((channels + POOL_CT - 1) / POOL_CT));
    hipLaunchKernelGGL(tab_pool_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, dx, record, num_windows, cols, num_bins, channels, H, dmap);
    AMTX_CHECK_LAUNCH();
    return AMTX_OK;
}

// ---- SoftmaxGroups.get_loss (models/common.py:369-440) forward and backward, modelled on amtx_bce_logits_loss (head.hip)
extern "C" size_t amtx_softmax_groups_loss_workspace_bytes(int batch, int num_frames, int num_groups, int num_classes) {
    if (batch <= 0 || num_frames <= 0 || num_groups <= 0 || num_classes <= 0) return 0;
    return (size_t)sm_loss_blocks(batch, num_frames, num_groups) * sizeof(float);
}

extern "C" int amtx_softmax_groups_loss(const float* logits, int64_t ld, const int64_t* targets, const float* weight, int batch, int num_frames,
                                        int num_groups, int num_classes, float* loss, float* grad, void* workspace, size_t workspace_bytes,
                                        void* stream) {
    AMTX_REQUIRE(logits && targets && loss, "amtx_softmax_groups_loss: null pointer");
    AMTX_REQUIRE(batch > 0 && num_frames > 0 && num_groups > 0 && num_classes > 0 && ld >= (int64_t)num_groups * num_classes,
                 "amtx_softmax_groups_loss: bad sizes");
    const int64_t pairs = (int64_t)batch * num_frames * num_groups;
    AMTX_REQUIRE(pairs < (1ll << 31), "amtx_softmax_groups_loss: too many frames");
    AMTX_REQUIRE(workspace && workspace_bytes >= amtx_softmax_groups_loss_workspace_bytes(batch, num_frames, num_groups, num_classes),
                 "amtx_softmax_groups_loss: workspace too small");
    const int64_t blocks = sm_loss_blocks(batch, num_frames, num_groups);
    const float inv_bt = 1.0f / ((float)batch * (float)num_frames);
    float* partial = static_cast<float*>(workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(sm_loss_kernel, dim3((unsigned)blocks), dim3(256), 0, s, logits, ld, targets, weight, num_frames, num_groups, num_classes,
                       pairs, inv_bt, grad, partial);
    AMTX_CHECK_LAUNCH();
    return amtx_launch_loss_reduce(partial, blocks, inv_bt, loss, s);
}
