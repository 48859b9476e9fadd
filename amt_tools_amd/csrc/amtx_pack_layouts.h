// The packed weight layouts of the engine, each defined ONCE for the host packers (conv.hip, convg.hip, gemm.hip, lstm.hip, pack.hip:
// `for (item = 0; item < n_items; ++item) layout(item, ..., put)`) and the device packers (pack.hip, lstm.hip: a grid-stride loop over
// the same call), plus the BatchNorm fold and the hi / lo split they share.  A layout maps a work item to values and to positions
// (fragment, element) or (matrix index); the writer `put` turns a position into memory and splits the value into the planes.
// Everything here is `static inline`: six files are compiled twice with a different 16-bit format (amtx_common.h: AMTX_FMT_NS), so a name with
// external linkage would be one name with two meanings.
#pragma once
#include "amtx_common.h"

#include <cmath>

constexpr int AMTX_FRAG = 64 * 8;          // elements of one MFMA operand fragment and plane: 64 lanes x 8 values
constexpr int AMTX_CONV_CIN = 32;          // input channels of conv.hip's 3x3 layers (convf.hip and convx.hip read the same fragments)
constexpr int AMTX_LSTM_BWD_WAVES = 8;     // waves of a backward-recurrence block: each owns hidden / 8 units of the transposed fragments

// fragments per 16-channel output tile of convg.hip: nine taps x the full 32-deep steps, five paired fragments for a 16-channel tail
static constexpr __host__ __device__ int g_wfrags_per_tile(int ci16) { return 9 * (ci16 / 2) + 5 * (ci16 % 2); }

// ---------------------------------------------------------------- the hi / lo split and the two writers
// planes == 1: out[i] = 16-bit(v).  planes == 2: hi = 16-bit(v) at i, lo = 16-bit(v - hi) plane_stride elements behind it.
static inline __host__ __device__ void amtx_split_store(bf16_t* out, size_t i, size_t plane_stride, int planes, float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    // v is often a product (weight x BatchNorm scale).  In the half-precision build hipcc would fuse multiply and conversion into one
    // v_fma_mixlo_f16, i.e. round the exact product ONCE to half, where the host rounds it to fp32 first: rare last-bit
    // differences between a device-synced and a host-synced model (seen as 3e-5 ... 4e-4 on f16 logits).  Keep the fp32 product.
    asm volatile("" : "+v"(v));
#endif
    const bf16_t hi = f32_to_bf16_rn(v);
    out[i] = hi;
    if (planes == 2) out[i + plane_stride] = f32_to_bf16_rn(v - bf16_to_f32(hi));
}

// The writers' member functions call the split of THIS build's 16-bit format: internal linkage like everything else here (an inline
// member of a named struct would be one symbol for the bf16 and the f16 objects, and the linker keeps only one of the two).
namespace {
// element e of fragment `frag` of [fragment][plane][frag_elems]
struct AmtxFragPut {
    bf16_t* out; int planes; int frag_elems = AMTX_FRAG;
    __host__ __device__ void operator()(size_t frag, int e, float v) const { amtx_split_store(out, frag * planes * frag_elems + e, frag_elems, planes, v); }
};
// element i of a [plane][plane_elems] matrix
struct AmtxPlanePut {
    bf16_t* out; int planes; size_t plane_elems;
    __host__ __device__ void operator()(size_t i, float v) const { amtx_split_store(out, i, plane_elems, planes, v); }
};
}  // namespace

// ---------------------------------------------------------------- BatchNorm fold
// eval-mode BatchNorm2d behind a conv: scale = gamma / sqrt(var + 1e-5), shift = beta + (conv_bias - mean) * scale, in double, rounded once
static inline __host__ __device__ void amtx_bn_fold(const float* cb, const float* g, const float* be, const float* mu, const float* var, int c, float* scale,
                                                    float* shift) {
#pragma clang fp contract(off)      // neither compiler may fuse these: the same bits on both sides
    const double s = (double)g[c] / sqrt((double)var[c] + 1e-5);
    scale[c] = (float)s;
    shift[c] = (float)((double)be[c] + ((double)cb[c] - (double)mu[c]) * s);
}

// the fp32 weights of the unfused first convolution: out[row][i] = w[row][i] * scale[row]; item = one element
static inline __host__ __device__ void amtx_layout_scale_rows(int item, const float* w, const float* scale, int cols, float* out) {
    out[item] = w[item] * scale[item / cols];
}

// ---------------------------------------------------------------- conv.hip: 3x3 layer, 32 input channels
// [tap][nt][plane][lane][8]: lane l = (row, k-group), row -> channel co = (row >> 2) 4 NT + 4 nt + (row & 3), k = 8 (l >> 4) + j -> input channel.
// item = one element.
static inline __host__ __device__ int amtx_layout_conv3x3_items(int c_out) { return 9 * (c_out / 16) * AMTX_FRAG; }
template <class Put>
static inline __host__ __device__ void amtx_layout_conv3x3(int item, const float* w, const float* scale, int c_out, const Put& put) {
    const int NT = c_out / 16;
    int r = item;
    const int j = r & 7; r >>= 3;
    const int l = r & 63; r >>= 6;
    const int nt = r % NT, tap = r / NT;
    const int row = l & 15;
    const int co = (row >> 2) * (4 * NT) + 4 * nt + (row & 3);
    const int ci = (l >> 4) * 8 + j;
    put(tap * NT + nt, l * 8 + j, w[((size_t)co * AMTX_CONV_CIN + ci) * 9 + tap] * (scale ? scale[co] : 1.0f));
}

// conv.hip: Toeplitz A fragments of the fused first conv with ONE input channel (conv3x3_kernel, KS == 1), [q][nt][plane][lane][8]:
// fragment (q, nt), lane l = (row, k-group g): row -> channel co = 8 (row >> 2) + 4 nt + (row & 3) (a lane of the D tile then holds 8
// consecutive channels over nt = 0, 1), k = 8 g + e -> tap (dy = g, kw = e - q) of output column q within a 4-column unit; everything
// else is zero.  item = one element.
constexpr int AMTX_LAYOUT_CONV1_ITEMS = 4 * 2 * AMTX_FRAG;
template <class Put>
static inline __host__ __device__ void amtx_layout_conv1(int item, const float* w, const float* scale, const Put& put) {
    int r = item;
    const int e = r & 7; r >>= 3;
    const int l = r & 63; r >>= 6;
    const int nt = r & 1, q = r >> 1;
    const int row = l & 15, g = l >> 4;
    const int co = (row >> 2) * 8 + 4 * nt + (row & 3);
    const int kw = e - q;
    put(q * 2 + nt, l * 8 + e, (g < 3 && kw >= 0 && kw <= 2) ? w[(size_t)co * 9 + g * 3 + kw] * (scale ? scale[co] : 1.0f) : 0.0f);
}

// conv.hip: the fused first conv with SEVERAL input channels, legacy 16-deep steps: [ks][nt][plane][lane][4], k = 16 ks + 4 (l >> 4) + j over
// (ci, kh, kw) in the weight tensor's own order, zero past 9 c_in.  Host only (no device packer: ConvPlan::device_resync).
static inline void amtx_layout_conv1_multi(const float* w, const float* scale, int c_in, int planes, bf16_t* out) {
    const int kvalid = 9 * c_in, ksteps = (kvalid + 15) / 16;
    const AmtxFragPut put{out, planes, 64 * 4};
    for (int ks = 0; ks < ksteps; ++ks)
        for (int nt = 0; nt < 2; ++nt)
            for (int l = 0; l < 64; ++l) {
                const int row = l & 15;
                const int co = (row >> 2) * 8 + 4 * nt + (row & 3);
                for (int j = 0; j < 4; ++j) {
                    const int k = 16 * ks + 4 * (l >> 4) + j;
                    put(ks * 2 + nt, l * 4 + j, k < kvalid ? w[(size_t)co * kvalid + k] * (scale ? scale[co] : 1.0f) : 0.0f);
                }
            }
}

// ---------------------------------------------------------------- convg.hip: 3x3 layer, any multiple of 16 input channels
// [chunk][fragment][plane][lane][8], a chunk = ntc 16-channel tiles; fragments of a chunk: the full 32-deep steps in (tap, tile, step)
// order, then (C_in with a 16-channel tail) the paired tails A (kw, tile): taps (0,kw) | (1,kw); B (tile): (2,0) | (2,1); C (tile): (2,2) | 0.
// item = one (chunk, tile, lane, j): it writes its element of every fragment of the tile.
static inline __host__ __device__ int amtx_layout_conv_gen_items(int c_out) { return (c_out / 16) * AMTX_FRAG; }
template <class Put>
static inline __host__ __device__ void amtx_layout_conv_gen(int item, const float* w, const float* scale, int c_in, int ntc, const Put& put) {
    const int ci16 = c_in / 16, n32 = ci16 / 2, n16 = ci16 % 2;
    const int nmain = 9 * ntc * n32, nfrag = ntc * g_wfrags_per_tile(ci16);
    int r = item;
    const int j = r & 7; r >>= 3;
    const int l = r & 63; r >>= 6;
    const int nt = r % ntc, ch = r / ntc;
    const int row = l & 15, gq = l >> 4;
    const int co = ch * 16 * ntc + (row >> 2) * (4 * ntc) + 4 * nt + (row & 3);
    const float sc = scale ? scale[co] : 1.0f;
    auto wv = [&](int ci, int tap) { return w[((size_t)co * c_in + ci) * 9 + tap] * sc; };
    auto frag = [&](int f, float v) { put((size_t)ch * nfrag + f, l * 8 + j, v); };
    for (int tap = 0; tap < 9; ++tap)
        for (int ks = 0; ks < n32; ++ks) frag((tap * ntc + nt) * n32 + ks, wv(32 * ks + 8 * gq + j, tap));
    if (!n16) return;
    const int ct = 32 * n32 + 8 * (gq & 1) + j;                          // tail channel of this lane group and j
    for (int kw = 0; kw < 3; ++kw) frag(nmain + kw * ntc + nt, wv(ct, (gq < 2 ? 0 : 3) + kw));   // A: tap rows 0 | 1 at column shift kw
    frag(nmain + 3 * ntc + nt, wv(ct, gq < 2 ? 6 : 7));                 // B: (2,0) | (2,1)
    frag(nmain + 4 * ntc + nt, gq < 2 ? wv(ct, 8) : 0.0f);              // C: (2,2) | zero
}

// convg.hip: fused first conv (c_in -> c_mid channels), [tile of 16 channels][k-step][plane][lane][8].  Two K orders (amtx_conv1g_tapk):
// the weight tensor's own, k = 32 ks + 8 (lane >> 4) + j over (ci, kh, kw), zero past 9 c_in; or tap-major with 8 channel slots per tap,
// k = 8 tap + ci, three steps.  item = one element.
static inline __host__ __device__ int amtx_conv1g_ksteps(int c_in, bool tapk) { return tapk ? 3 : (9 * c_in + 31) / 32; }
static inline __host__ __device__ int amtx_layout_conv1g_items(int c_in, int c_mid, bool tapk) { return (c_mid / 16) * amtx_conv1g_ksteps(c_in, tapk) * AMTX_FRAG; }
template <class Put>
static inline __host__ __device__ void amtx_layout_conv1g(int item, const float* w, const float* scale, int c_in, bool tapk, const Put& put) {
    const int kvalid = 9 * c_in, nks = amtx_conv1g_ksteps(c_in, tapk);
    int r = item;
    const int j = r & 7; r >>= 3;
    const int l = r & 63; r >>= 6;
    const int ks = r % nks, nt = r / nks;
    const int co = 16 * nt + (l & 15);
    const int tap = 4 * ks + (l >> 4), k = 32 * ks + 8 * (l >> 4) + j;
    const bool valid = tapk ? tap < 9 && j < c_in : k < kvalid;
    const size_t src = tapk ? ((size_t)co * c_in + j) * 9 + tap : (size_t)co * kvalid + k;
    put(nt * nks + ks, l * 8 + j, valid ? w[src] * (scale ? scale[co] : 1.0f) : 0.0f);
}

// ---------------------------------------------------------------- gemm.hip: Linear
// fc1's columns: the reference flattens (channel, freq), the conv kernels write (freq, channel): packed column k = f nf3 + c is column
// c fq + f of W.  The fold of the pitch head walks W_fc1 by the same map.
static inline __host__ __device__ int amtx_fc1_col(int k, int nf3, int fq) { return (k % nf3) * fq + k / nf3; }

// Rows [row0, row0 + rows_owned) of a [planes][n_pad][k_pad] matrix from W (N x K, leading dimension ldw), zero padding included for the
// rows it owns (rows_owned >= N: whoever packs the last row block passes the pad rows too).  perm_c > 0 (a multiple of 8): packed column
// k is column amtx_fc1_col(k, perm_c, perm_f) of W.  item = one run of 8 columns of one row (k_pad is a multiple of 8; with perm_c a
// multiple of 8 a run is 8 channels of one frequency: source columns perm_f apart).
static inline __host__ __device__ int64_t amtx_layout_linear_items(int rows_owned, int k_pad) { return (int64_t)rows_owned * (k_pad / 8); }
template <class Put>
static inline __host__ __device__ void amtx_layout_linear(int64_t item, const float* W, int64_t ldw, int N, int K, int k_pad, int row0, int perm_c, int perm_f,
                                                          const Put& put) {
    const int n = (int)(item / (k_pad / 8)), k0 = 8 * (int)(item - (int64_t)n * (k_pad / 8));
    const float* src = W + (int64_t)n * ldw + (perm_c > 0 ? amtx_fc1_col(k0, perm_c, perm_f) : k0);
    const int step = perm_c > 0 ? perm_f : 1;
    for (int j = 0; j < 8; ++j) put((size_t)(row0 + n) * k_pad + k0 + j, n < N && k0 + j < K ? src[(int64_t)j * step] : 0.0f);
}

// ---------------------------------------------------------------- lstm.hip: W_hh (4 hidden x hidden per direction, gate-major rows i, f, g, o)
// Forward fragments [dir][unit tile u][gate q][k-step][plane][lane][8] = W[q hidden + 16 u + (l & 15)][32 ks + 8 (l >> 4) + j].  A wave of
// the hidden-128 kernels owns consecutive unit tiles, so their [dir][wave][unit block] order is this one.  item = one (fragment, lane).
static inline __host__ __device__ int amtx_layout_bilstm_items(int hidden) { return hidden * hidden; }     // 2 x 4 hidden x hidden / 8; the transposed layout has as many
template <class Put>
static inline __host__ __device__ void amtx_layout_bilstm(int item, const float* whh_fwd, const float* whh_bwd, int hidden, const Put& put) {
    const int nu = hidden / 16, ksn = hidden / 32;
    int r = item;
    const int l = r & 63; r >>= 6;
    const int ks = r % ksn; r /= ksn;
    const int q = r & 3; r >>= 2;
    const int u = r % nu, dir = r / nu;
    const float* src = (dir == 0 ? whh_fwd : whh_bwd) + (size_t)(q * hidden + 16 * u + (l & 15)) * hidden + 32 * ks + 8 * (l >> 4);
    for (int j = 0; j < 8; ++j) put(item >> 6, l * 8 + j, src[j]);
}

// Transposed fragments for the backward recurrence (training; device only), [dir][wave][unit tile ut][k-step][plane][lane][8] =
// W[32 ks + 8 (l >> 4) + j][16 (hidden / 128) wave + 16 ut + (l & 15)], k over all 4 hidden rows.  item = one (fragment, lane).
template <class Put>
static inline __host__ __device__ void amtx_layout_bilstm_transposed(int item, const float* whh_fwd, const float* whh_bwd, int hidden, const Put& put) {
    const int ut_n = hidden / (16 * AMTX_LSTM_BWD_WAVES), ksn = 4 * hidden / 32;
    int r = item;
    const int l = r & 63; r >>= 6;
    const int ks = r % ksn; r /= ksn;
    const int ut = r % ut_n; r /= ut_n;
    const int wv = r % AMTX_LSTM_BWD_WAVES, dir = r / AMTX_LSTM_BWD_WAVES;
    const float* src = (dir == 0 ? whh_fwd : whh_bwd) + (size_t)(32 * ks + 8 * (l >> 4)) * hidden + 16 * ut_n * wv + 16 * ut + (l & 15);
    for (int j = 0; j < 8; ++j) put(item >> 6, l * 8 + j, src[(size_t)j * hidden]);
}
