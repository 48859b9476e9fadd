// Device-side weight packing for a weight RE-SYNC of the Onsets & Frames engine (amtx_of_model_finalize_device), and the Linear packer
// of both sides.  The layouts, the BatchNorm fold and the hi / lo split are those of amtx_pack_layouts.h, which the host packers call as
// well: a kernel here is a grid-stride loop over the same function a host packer loops over, so a model synced on the device holds the
// SAME BITS as one synced through the host (tests/test_gpu_model.py::test_device_side_weight_sync_equals_the_host_path).  Why:
// validate() inside train() (amt_tools/train.py:183-189) re-syncs the engine at every checkpoint; through the host that is a
// device-to-host copy of every tensor, ~164 M double multiply-adds and the packing loops on one core, and the upload -- 30 - 60 ms; here
// it is a handful of small kernels.
// Compiled twice like the kernels that read the packed weights (namespace AMTX_FMT_NS): the 16-bit format is the build's.

#include "amtx_kernels.h"
#include "amtx_pack_layouts.h"

#include <algorithm>

namespace {

#define PACK_ITEMS(T, item, n) for (T item = (T)blockIdx.x * blockDim.x + threadIdx.x; item < (n); item += (T)gridDim.x * blockDim.x)

__global__ void bn_fold_kernel(const float* cb, const float* g, const float* be, const float* mu, const float* var, int c_out, float* scale, float* shift) {
    PACK_ITEMS(int, c, c_out) amtx_bn_fold(cb, g, be, mu, var, c, scale, shift);
}

__global__ void conv3x3_pack_kernel(const float* w, const float* scale, int c_out, int n, AmtxFragPut put) {
    PACK_ITEMS(int, item, n) amtx_layout_conv3x3(item, w, scale, c_out, put);
}

__global__ void conv1_pack_kernel(const float* w, const float* scale, AmtxFragPut put) {
    PACK_ITEMS(int, item, AMTX_LAYOUT_CONV1_ITEMS) amtx_layout_conv1(item, w, scale, put);
}

__global__ void linear_pack_kernel(const float* W, int64_t ldw, int N, int K, int k_pad, int row0, int perm_c, int perm_f, int64_t n, AmtxPlanePut put) {
    PACK_ITEMS(int64_t, item, n) amtx_layout_linear(item, W, ldw, N, K, k_pad, row0, perm_c, perm_f, put);
}

// ofmodel.hip: (W_out . W_fc1) and W_out . b_fc1 + b_out in double, j ascending -- the host's summation order.  Output column k is in the
// engine's (freq, channel) order (amtx_fc1_col); columns kfc .. kfc_pad are zero.  One thread per element, where the host blocks by rows.
__global__ void head_fold_kernel(const float* w_out, const float* w_fc1, const float* b_fc1, const float* b_out, int n_out, int dim_am, int kfc,
                                 int kfc_pad, int nf3, int fq, float* wfold, float* bfold) {
#pragma clang fp contract(off)
    PACK_ITEMS(int64_t, idx, (int64_t)n_out * kfc_pad) {
        const int o = (int)(idx / kfc_pad), k = (int)(idx - (int64_t)o * kfc_pad);
        double acc = 0.0;
        if (k < kfc) {
            const int ks = amtx_fc1_col(k, nf3, fq);
            for (int j = 0; j < dim_am; ++j) acc += (double)w_out[(size_t)o * dim_am + j] * (double)w_fc1[(size_t)j * kfc + ks];
        }
        wfold[idx] = (float)acc;
    }
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o < n_out) {
        double acc = b_out[o];
        for (int j = 0; j < dim_am; ++j) acc += (double)w_out[(size_t)o * dim_am + j] * (double)b_fc1[j];
        bfold[o] = (float)acc;
    }
}

__global__ void conv_gen_pack_kernel(const float* w, const float* scale, int c_in, int ntc, int n, AmtxFragPut put) {
    PACK_ITEMS(int, item, n) amtx_layout_conv_gen(item, w, scale, c_in, ntc, put);
}

__global__ void conv1g_pack_kernel(const float* w, const float* scale, int c_in, bool tapk, int n, AmtxFragPut put) {
    PACK_ITEMS(int, item, n) amtx_layout_conv1g(item, w, scale, c_in, tapk, put);
}

__global__ void scale_rows_kernel(const float* w, const float* scale, int rows, int cols, float* out) {
    PACK_ITEMS(int, item, rows * cols) amtx_layout_scale_rows(item, w, scale, cols, out);
}

__global__ void vec_add_kernel(const float* a, const float* b, int n, float* out) {
    PACK_ITEMS(int, i, n) out[i] = a[i] + b[i];
}

}  // namespace

namespace AMTX_FMT_NS {

int amtx_pack_bn_fold_dev(const float* conv_bias, const float* gamma, const float* beta, const float* mean, const float* var, int c_out, float* scale,
                          float* shift, hipStream_t s) {
    hipLaunchKernelGGL(bn_fold_kernel, dim3((c_out + 63) / 64), dim3(64), 0, s, conv_bias, gamma, beta, mean, var, c_out, scale, shift);
    AMTX_CHECK_LAUNCH();
    return AMTX_OK;
}

int amtx_pack_conv3x3_dev(const float* w, const float* scale, int c_out, int planes, bf16_t* out, hipStream_t s) {
    hipLaunchKernelGGL(conv3x3_pack_kernel, dim3(64), dim3(256), 0, s, w, scale, c_out, amtx_layout_conv3x3_items(c_out), AmtxFragPut{out, planes});
    AMTX_CHECK_LAUNCH();
    return AMTX_OK;
}

int amtx_pack_conv_gen_dev(const float* w, const float* scale, int c_in, int c_out, int ntc, int planes, bf16_t* out, hipStream_t s) {
    AMTX_REQUIRE(ntc > 0 && c_in % 16 == 0 && c_out % (16 * ntc) == 0, "conv pack (general): bad channel counts %d -> %d", c_in, c_out);
    hipLaunchKernelGGL(conv_gen_pack_kernel, dim3(32), dim3(256), 0, s, w, scale, c_in, ntc, amtx_layout_conv_gen_items(c_out), AmtxFragPut{out, planes});
    AMTX_CHECK_LAUNCH();
    return AMTX_OK;
}

int amtx_pack_conv1g_dev(const float* w, const float* scale, int c_in, int c_mid, int planes, bf16_t* out, hipStream_t s) {
    const bool tapk = amtx_conv1g_tapk(c_in, planes);
    hipLaunchKernelGGL(conv1g_pack_kernel, dim3(16), dim3(256), 0, s, w, scale, c_in, tapk, amtx_layout_conv1g_items(c_in, c_mid, tapk), AmtxFragPut{out, planes});
    AMTX_CHECK_LAUNCH();
    return AMTX_OK;
}

int amtx_pack_scale_rows_dev(const float* w, const float* scale, int rows, int cols, float* out, hipStream_t s) {
    hipLaunchKernelGGL(scale_rows_kernel, dim3((rows * cols + 255) / 256), dim3(256), 0, s, w, scale, rows, cols, out);
    AMTX_CHECK_LAUNCH();
    return AMTX_OK;
}

int amtx_pack_conv1_dev(const float* w, const float* scale, int planes, bf16_t* out, hipStream_t s) {
    hipLaunchKernelGGL(conv1_pack_kernel, dim3(16), dim3(256), 0, s, w, scale, AmtxFragPut{out, planes});
    AMTX_CHECK_LAUNCH();
    return AMTX_OK;
}

int amtx_pack_linear_dev(const float* W, int64_t ldw, int N, int K, int planes, int n_pad, int k_pad, int row0, int rows_owned, int perm_c, int perm_f,
                         bf16_t* out, hipStream_t s) {
    AMTX_REQUIRE(k_pad % 8 == 0 && perm_c % 8 == 0, "linear pack: k_pad and the permuted channel count must be multiples of 8");
    const int64_t n = amtx_layout_linear_items(rows_owned, k_pad);
    const unsigned blocks = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(linear_pack_kernel, dim3(blocks), dim3(256), 0, s, W, ldw, N, K, k_pad, row0, perm_c, perm_f, n, AmtxPlanePut{out, planes, (size_t)n_pad * k_pad});
    AMTX_CHECK_LAUNCH();
    return AMTX_OK;
}

void amtx_pack_linear_host(const float* W, int64_t ldw, int N, int K, int planes, int n_pad, int k_pad, int row0, int rows_owned, int perm_c, int perm_f,
                           bf16_t* out) {
    const AmtxPlanePut put{out, planes, (size_t)n_pad * k_pad};
    for (int64_t item = 0, n = amtx_layout_linear_items(rows_owned, k_pad); item < n; ++item) amtx_layout_linear(item, W, ldw, N, K, k_pad, row0, perm_c, perm_f, put);
}

int amtx_pack_head_fold_dev(const float* w_out, const float* w_fc1, const float* b_fc1, const float* b_out, int n_out, int dim_am, int kfc, int kfc_pad,
                            int nf3, int fq, float* wfold, float* bfold, hipStream_t s) {
    const int64_t total = (int64_t)n_out * kfc_pad;
    hipLaunchKernelGGL(head_fold_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, w_out, w_fc1, b_fc1, b_out, n_out, dim_am, kfc, kfc_pad,
                       nf3, fq, wfold, bfold);
    AMTX_CHECK_LAUNCH();
    return AMTX_OK;
}

int amtx_pack_vec_add_dev(const float* a, const float* b, int n, float* out, hipStream_t s) {
    hipLaunchKernelGGL(vec_add_kernel, dim3((n + 255) / 256), dim3(256), 0, s, a, b, n, out);
    AMTX_CHECK_LAUNCH();
    return AMTX_OK;
}

}  // namespace AMTX_FMT_NS
