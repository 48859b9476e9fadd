// TabCNN inference engine (amt_tools/models/tabcnn.py:17-221, model_complexity 1): the amtx_tab_* ABI of include/amtx.h.
//
// The reference convolves every frame's 9-frame context window on its own.  Its three 3x3 convolutions are unpadded with stride 1, so
// column w of window t after any number of them is column t + w of the same layers run once over the whole (zero-padded) sequence:
// the engine runs them once per sequence of num_windows + 8 columns and takes the 2x2 max-pool of window t from sequence columns
// {t, t+1} (the window's third conv3 column falls to the pool's floor).  Same dot products, 3.5x less arithmetic at dim_in 192.
//
//   tab_conv12   features (fp32, any strides) -> conv1 + ReLU (fp32, LDS only) -> conv2 + ReLU (MFMA implicit GEMM)
//                -> conv2 map [B][T+4][F-4][64] channels-last in HBM, bf16 or the two split planes (x3)
//   tab_conv3    conv2 map -> conv3 + ReLU (MFMA) -> 2x2 max-pool in the epilogue -> fc's input rows [B*T][64*H] (h-major, channel
//                minor; dense.0.weight's columns are permuted at pack time to match), bf16 or split planes
//   fc           amtx_launch_gemm (gemm.hip): [B*T][128] fp32 = rows . W^T + bias
//   tab_head     ReLU -> output layer (fp32) -> logits [B*T][G*C] and the per-group argmax (first index on ties, last class -> -1) as
//                tablature [B][G][T] int64
#include "amtx_kernels.h"
#include "amtx_model_common.h"

namespace {

constexpr int TAB_THREADS = 256;   // four waves: wave w owns output channels 16w .. 16w+15 of conv2 / conv3
constexpr int TAB_TF = 16;         // output rows (frequency) per tile: one MFMA column block
constexpr int TAB_TT = 16;         // output columns (sequence) per tile
constexpr int TAB_C1 = 32, TAB_C2 = 64;
constexpr int TAB_P1 = TAB_C1 + 8; // LDS elements per conv1 position (80 bytes: spreads the 16-lane column reads over the banks)
constexpr int TAB_P2 = TAB_C2 + 8; // LDS elements per conv2 position (144 bytes)
constexpr int TAB_FC = 128;        // fc width at model_complexity 1
constexpr int TAB_HEAD_ROWS = 8;   // frames per tab_head workgroup
constexpr int TAB_MAX_GC = 256;

// one 16x16x32 product in the precision of the build: bf16 (one plane) or x3 (hi.hi + hi.lo + lo.hi)
template <int PLANES>
__device__ __forceinline__ amtx_f32x4 tab_mfma(const uint4* a, const uint4* b, amtx_f32x4 c) {
    if (PLANES == 2) {
        c = amtx_mfma_16x16x32(a[1], b[0], c);
        c = amtx_mfma_16x16x32(a[0], b[1], c);
    }
    return amtx_mfma_16x16x32(a[0], b[0], c);
}

// four channels of one position to a bf16 row (8 bytes) or to the two planes of a split row
template <int PLANES>
__device__ __forceinline__ void tab_store4(bf16_t* dst, int64_t split, float v0, float v1, float v2, float v3) {
    if (PLANES == 2) {
        uint32_t h0, l0, h1, l1;
        split_bf16x2(v0, v1, h0, l0);
        split_bf16x2(v2, v3, h1, l1);
        *reinterpret_cast<uint2*>(dst) = make_uint2(h0, h1);
        *reinterpret_cast<uint2*>(dst + split) = make_uint2(l0, l1);
    } else {
        *reinterpret_cast<uint2*>(dst) = make_uint2(pack_bf16x2(v0, v1), pack_bf16x2(v2, v3));
    }
}

struct Conv12Args {
    const float* feats; int64_t sb, sc, sf, st;   // element strides of the features; column t of clip b at feats + b*sb + t*st
    int c_in, F, cols;                            // cols = num_windows + 8
    const float* w1; const float* b1;            // [c_in*9][32] fp32, [32]
    const bf16_t* w2frag; const float* b2;       // [planes][4][9][64 lanes][8], [64]
    bf16_t* y2; int64_t y2_split;                // [B][T2][F2][64]
    int T2, F2;                                   // num_windows + 4, F - 4
};

// grid (ceil(T2/16), ceil(F2/16), B).  A tile: conv1 at (16+2) x (16+2) positions from (16+4) x (16+4) feature values per channel, then
// conv2 at 16 x 16 positions; the conv1 map lives in LDS only.
template <int PLANES>
__global__ void __launch_bounds__(TAB_THREADS) tab_conv12_kernel(Conv12Args a) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int XF = TAB_TF + 4, XT = TAB_TT + 4, YF = TAB_TF + 2, YT = TAB_TT + 2;
    const int c_in = a.c_in;
    float* xs = reinterpret_cast<float*>(smem);                    // [c_in][XF][XT]
    float* w1s = xs + c_in * XF * XT;                               // [c_in*9][32]
    float* b1s = w1s + c_in * 9 * TAB_C1;                          // [32]
    bf16_t* y1 = reinterpret_cast<bf16_t*>(b1s + TAB_C1);          // [PLANES][YT][YF][P1]
    constexpr int Y1_PLANE = YT * YF * TAB_P1;

    const int tid = threadIdx.x;
    const int t0 = blockIdx.x * TAB_TT, f0 = blockIdx.y * TAB_TF, b = blockIdx.z;
    for (int i = tid; i < c_in * 9 * TAB_C1; i += TAB_THREADS) w1s[i] = a.w1[i];
    if (tid < TAB_C1) b1s[tid] = a.b1[tid];
    const float* fb = a.feats + (int64_t)b * a.sb;
    for (int i = tid; i < c_in * XF * XT; i += TAB_THREADS) {
        const int c = i / (XF * XT), r = i % (XF * XT), fi = r / XT, ti = r % XT;
        const int f = f0 + fi, t = t0 + ti;
        xs[i] = (f < a.F && t < a.cols) ? fb[c * a.sc + (int64_t)f * a.sf + (int64_t)t * a.st] : 0.0f;
    }
    __syncthreads();

    // conv1 + bias + ReLU in fp32: one position x 8 output channels per task
    for (int task = tid; task < YT * YF * 4; task += TAB_THREADS) {
        const int cg = task & 3, pos = task >> 2, fi = pos % YF, ti = pos / YF;
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = b1s[cg * 8 + j];
        for (int c = 0; c < c_in; ++c) {
#pragma unroll
            for (int kf = 0; kf < 3; ++kf)
#pragma unroll
                for (int kt = 0; kt < 3; ++kt) {
                    const float x = xs[(c * XF + fi + kf) * XT + ti + kt];
                    const float4* w = reinterpret_cast<const float4*>(w1s + (c * 9 + kf * 3 + kt) * TAB_C1 + cg * 8);
                    const float4 wa = w[0], wb = w[1];
                    acc[0] += x * wa.x; acc[1] += x * wa.y; acc[2] += x * wa.z; acc[3] += x * wa.w;
                    acc[4] += x * wb.x; acc[5] += x * wb.y; acc[6] += x * wb.z; acc[7] += x * wb.w;
                }
        }
        uint32_t hi[4], lo[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float u = fmaxf(acc[2 * j], 0.0f), v = fmaxf(acc[2 * j + 1], 0.0f);
            if (PLANES == 2) split_bf16x2(u, v, hi[j], lo[j]);
            else hi[j] = pack_bf16x2(u, v);
        }
        bf16_t* dst = y1 + (ti * YF + fi) * TAB_P1 + cg * 8;
        *reinterpret_cast<uint4*>(dst) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
        if (PLANES == 2) *reinterpret_cast<uint4*>(dst + Y1_PLANE) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
    }

    // conv2 weights of this wave's 16 output channels, register-resident: A operand, rows = output channels
    const int wave = tid >> 6, lane = tid & 63;
    uint4 wa[9][PLANES];
#pragma unroll
    for (int s = 0; s < 9; ++s)
#pragma unroll
        for (int p = 0; p < PLANES; ++p)
            wa[s][p] = reinterpret_cast<const uint4*>(a.w2frag)[((p * 4 + wave) * 9 + s) * 64 + lane];
    float bias[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) bias[i] = a.b2[wave * 16 + 4 * (lane >> 4) + i];
    __syncthreads();

    const int pos = lane & 15, kq = 8 * (lane >> 4);
    const int f2 = f0 + pos;
    for (int tc = 0; tc < TAB_TT; ++tc) {
        const int t2 = t0 + tc;
        if (t2 >= a.T2) break;
        amtx_f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int s = 0; s < 9; ++s) {
            const int kf = s / 3, kt = s % 3;
            const bf16_t* src = y1 + ((tc + kt) * YF + pos + kf) * TAB_P1 + kq;
            uint4 bv[PLANES];
            bv[0] = *reinterpret_cast<const uint4*>(src);
            if (PLANES == 2) bv[PLANES - 1] = *reinterpret_cast<const uint4*>(src + Y1_PLANE);
            acc = tab_mfma<PLANES>(wa[s], bv, acc);
        }
        if (f2 < a.F2) {
            bf16_t* dst = a.y2 + (((int64_t)b * a.T2 + t2) * a.F2 + f2) * TAB_C2 + wave * 16 + 4 * (lane >> 4);
            tab_store4<PLANES>(dst, a.y2_split, fmaxf(acc[0] + bias[0], 0.0f), fmaxf(acc[1] + bias[1], 0.0f), fmaxf(acc[2] + bias[2], 0.0f),
                               fmaxf(acc[3] + bias[3], 0.0f));
        }
    }
}

struct Conv3Args {
    const bf16_t* y2; int64_t y2_split; int T2, F2;
    const bf16_t* w3frag; const float* b3;       // [planes][4][18][64 lanes][8], [64]
    bf16_t* e; int64_t e_split;                  // [B*T][K], K = 64*H
    int T, H, K;
};

// grid (ceil(T/16), ceil((F2-2)/16), B).  A tile: conv3 at 16 rows x 17 sequence columns (pooled window t needs columns t and t+1) from
// 18 x 19 conv2 positions in LDS; rows pooled across lane pairs, columns across consecutive iterations.
template <int PLANES>
__global__ void __launch_bounds__(TAB_THREADS) tab_conv3_kernel(Conv3Args a) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int YF = TAB_TF + 2, YT = TAB_TT + 3;
    constexpr int YS_PLANE = YT * YF * TAB_P2;
    bf16_t* ys = reinterpret_cast<bf16_t*>(smem);                  // [PLANES][YT][YF][P2]

    const int tid = threadIdx.x;
    const int t0 = blockIdx.x * TAB_TT, f0 = blockIdx.y * TAB_TF, b = blockIdx.z;
    for (int i = tid; i < YT * YF * 8; i += TAB_THREADS) {
        const int q = i & 7, p = i >> 3, fi = p % YF, ti = p / YF;
        const int f2 = f0 + fi, t2 = t0 + ti;
        uint4 hi = make_uint4(0, 0, 0, 0), lo = hi;
        if (f2 < a.F2 && t2 < a.T2) {
            const bf16_t* src = a.y2 + (((int64_t)b * a.T2 + t2) * a.F2 + f2) * TAB_C2 + q * 8;
            hi = *reinterpret_cast<const uint4*>(src);
            if (PLANES == 2) lo = *reinterpret_cast<const uint4*>(src + a.y2_split);
        }
        bf16_t* dst = ys + (ti * YF + fi) * TAB_P2 + q * 8;
        *reinterpret_cast<uint4*>(dst) = hi;
        if (PLANES == 2) *reinterpret_cast<uint4*>(dst + YS_PLANE) = lo;
    }
    const int wave = tid >> 6, lane = tid & 63;
    uint4 wa[18][PLANES];
#pragma unroll
    for (int s = 0; s < 18; ++s)
#pragma unroll
        for (int p = 0; p < PLANES; ++p)
            wa[s][p] = reinterpret_cast<const uint4*>(a.w3frag)[((p * 4 + wave) * 18 + s) * 64 + lane];
    float bias[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) bias[i] = a.b3[wave * 16 + 4 * (lane >> 4) + i];
    __syncthreads();

    const int pos = lane & 15, kq = 8 * (lane >> 4);
    const int h = (f0 + pos) >> 1;
    const bool writer = (pos & 1) == 0 && h < a.H;
    float prev[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int c3 = 0; c3 <= TAB_TT; ++c3) {
        const int t3 = t0 + c3;
        if (t3 > a.T) break;                       // the last pooled window, T - 1, reads columns T - 1 and T
        amtx_f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int s = 0; s < 18; ++s) {
            const int tap = s >> 1, kf = tap / 3, kt = tap % 3;
            const bf16_t* src = ys + ((c3 + kt) * YF + pos + kf) * TAB_P2 + 32 * (s & 1) + kq;
            uint4 bv[PLANES];
            bv[0] = *reinterpret_cast<const uint4*>(src);
            if (PLANES == 2) bv[PLANES - 1] = *reinterpret_cast<const uint4*>(src + YS_PLANE);
            acc = tab_mfma<PLANES>(wa[s], bv, acc);
        }
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[i] = fmaxf(acc[i] + bias[i], 0.0f);
            v[i] = fmaxf(v[i], __shfl_xor(v[i], 1, 64));          // rows 2h, 2h+1
        }
        if (c3 > 0 && writer) {
            const int t = t3 - 1;
            bf16_t* dst = a.e + ((int64_t)b * a.T + t) * a.K + h * TAB_C2 + wave * 16 + 4 * (lane >> 4);
            tab_store4<PLANES>(dst, a.e_split, fmaxf(prev[0], v[0]), fmaxf(prev[1], v[1]), fmaxf(prev[2], v[2]), fmaxf(prev[3], v[3]));
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) prev[i] = v[i];
    }
}

// ReLU(fc rows) -> output layer in fp32 -> logits and per-group argmax.  One workgroup per TAB_HEAD_ROWS frames; thread n = logit n.
__global__ void __launch_bounds__(TAB_THREADS) tab_head_kernel(const float* __restrict__ h1, const float* __restrict__ w, const float* __restrict__ bias,
                                                              float* logits, int64_t* tab, int64_t M, int T, int G, int C) {
    __shared__ __align__(16) float hs[TAB_HEAD_ROWS][TAB_FC];
    __shared__ float ls[TAB_HEAD_ROWS][TAB_MAX_GC];
    const int tid = threadIdx.x, GC = G * C;
    const int64_t m0 = (int64_t)blockIdx.x * TAB_HEAD_ROWS;
    for (int i = tid; i < TAB_HEAD_ROWS * TAB_FC; i += TAB_THREADS) {
        const int r = i / TAB_FC, k = i % TAB_FC;
        hs[r][k] = m0 + r < M ? fmaxf(h1[(m0 + r) * TAB_FC + k], 0.0f) : 0.0f;
    }
    __syncthreads();
    if (tid < GC) {
        float acc[TAB_HEAD_ROWS];
        const float b0 = bias[tid];
#pragma unroll
        for (int r = 0; r < TAB_HEAD_ROWS; ++r) acc[r] = b0;
        const float4* wr = reinterpret_cast<const float4*>(w + (int64_t)tid * TAB_FC);
        for (int k4 = 0; k4 < TAB_FC / 4; ++k4) {
            const float4 wv = wr[k4];
#pragma unroll
            for (int r = 0; r < TAB_HEAD_ROWS; ++r) {
                const float4 x = *reinterpret_cast<const float4*>(&hs[r][4 * k4]);
                acc[r] += x.x * wv.x;
                acc[r] += x.y * wv.y;
                acc[r] += x.z * wv.z;
                acc[r] += x.w * wv.w;
            }
        }
#pragma unroll
        for (int r = 0; r < TAB_HEAD_ROWS; ++r) {
            ls[r][tid] = acc[r];
            if (logits && m0 + r < M) logits[(m0 + r) * GC + tid] = acc[r];
        }
    }
    __syncthreads();
    if (!tab) return;
    for (int i = tid; i < TAB_HEAD_ROWS * G; i += TAB_THREADS) {
        const int r = i / G, g = i % G;
        const int64_t m = m0 + r;
        if (m >= M) continue;
        float best = ls[r][g * C];
        int arg = 0;
        for (int c = 1; c < C; ++c) {
            const float v = ls[r][g * C + c];
            if (v > best) { best = v; arg = c; }
        }
        const int64_t bb = m / T, t = m % T;
        tab[(bb * G + g) * T + t] = arg == C - 1 ? -1 : arg;
    }
}

size_t conv12_lds(int c_in, int planes) {
    return (size_t)(c_in * (TAB_TF + 4) * (TAB_TT + 4) + c_in * 9 * TAB_C1 + TAB_C1) * 4 + (size_t)planes * (TAB_TT + 2) * (TAB_TF + 2) * TAB_P1 * 2;
}
size_t conv3_lds(int planes) { return (size_t)planes * (TAB_TT + 3) * (TAB_TF + 2) * TAB_P2 * 2; }

}  // namespace

struct amtx_tab_model {
    int dim_in, in_channels, mc, G, C, precision, planes;
    int H, K;                                    // pooled rows, fc input width 64*H
    TensorStore store{"amtx_tab_model_finalize", "was never set"};
    std::map<std::string, int64_t> expected;     // state_dict key -> numel
    DevBuf w1, b1, w2, b2, w3, b3, fcw, fcb, hw, hb;
    int fc_npad = 0, fc_kpad = 0;
    bool finalized = false;
};

extern "C" int amtx_tab_model_create(amtx_tab_model** out, int dim_in, int in_channels, int model_complexity, int num_groups, int num_classes,
                                     int precision) {
    AMTX_REQUIRE(out, "amtx_tab_model_create: null model pointer");
    *out = nullptr;
    AMTX_REQUIRE(precision == AMTX_PREC_BF16 || precision == AMTX_PREC_X3, "amtx_tab_model_create: precision must be AMTX_PREC_BF16 or AMTX_PREC_X3 (got %d)", precision);
    AMTX_REQUIRE(dim_in >= 9, "amtx_tab_model_create: dim_in must be at least 9 (three unpadded 3x3 convolutions and a 2x2 pool; got %d)", dim_in);
    AMTX_REQUIRE(in_channels >= 1 && num_groups >= 1 && num_classes >= 1, "amtx_tab_model_create: bad dims");
    if (model_complexity != 1) {
        amtx_set_error("amtx_tab_model_create: model_complexity 1 (32/64/64 channels, fc 128) is implemented (got model_complexity=%d)", model_complexity);
        return AMTX_ERR_UNSUPPORTED;
    }
    if (in_channels > 8) {
        amtx_set_error("amtx_tab_model_create: in_channels 1 to 8 are implemented (got in_channels=%d)", in_channels);
        return AMTX_ERR_UNSUPPORTED;
    }
    if (dim_in > 2048) {
        amtx_set_error("amtx_tab_model_create: dim_in up to 2048 is implemented (got dim_in=%d)", dim_in);
        return AMTX_ERR_UNSUPPORTED;
    }
    if (num_classes > 32) {
        amtx_set_error("amtx_tab_model_create: num_classes up to 32 is implemented (got num_classes=%d)", num_classes);
        return AMTX_ERR_UNSUPPORTED;
    }
    if (num_groups * num_classes > TAB_MAX_GC) {
        amtx_set_error("amtx_tab_model_create: num_groups x num_classes up to %d is implemented (got %d x %d)", TAB_MAX_GC, num_groups, num_classes);
        return AMTX_ERR_UNSUPPORTED;
    }
    amtx_tab_model* m = new amtx_tab_model();
    m->dim_in = dim_in; m->in_channels = in_channels; m->mc = model_complexity; m->G = num_groups; m->C = num_classes;
    m->precision = precision; m->planes = precision == AMTX_PREC_X3 ? 2 : 1;
    m->H = (dim_in - 6) / 2; m->K = TAB_C2 * m->H;
    const int gc = num_groups * num_classes;
    m->expected = {{"conv.0.weight", (int64_t)TAB_C1 * in_channels * 9}, {"conv.0.bias", TAB_C1},
                   {"conv.2.weight", (int64_t)TAB_C2 * TAB_C1 * 9}, {"conv.2.bias", TAB_C2},
                   {"conv.4.weight", (int64_t)TAB_C2 * TAB_C2 * 9}, {"conv.4.bias", TAB_C2},
                   {"dense.0.weight", (int64_t)TAB_FC * m->K}, {"dense.0.bias", TAB_FC},
                   {"dense.3.output_layer.weight", (int64_t)gc * TAB_FC}, {"dense.3.output_layer.bias", gc}};
    *out = m;
    return AMTX_OK;
}

extern "C" int amtx_tab_model_destroy(amtx_tab_model* m) {
    if (!m) return AMTX_OK;
    DevBuf* bufs[] = {&m->w1, &m->b1, &m->w2, &m->b2, &m->w3, &m->b3, &m->fcw, &m->fcb, &m->hw, &m->hb};
    for (DevBuf* b : bufs) b->release();
    delete m;
    return AMTX_OK;
}

extern "C" int amtx_tab_model_set_tensor(amtx_tab_model* m, const char* name, const float* host_data, int64_t numel) {
    AMTX_REQUIRE(m && name && host_data, "amtx_tab_model_set_tensor: bad argument");
    auto it = m->expected.find(name);
    AMTX_REQUIRE(it != m->expected.end(), "amtx_tab_model_set_tensor: unknown tensor '%s' (the reference's TabCNN state_dict keys: conv.{0,2,4}.{weight,bias}, "
                                          "dense.0.{weight,bias}, dense.3.output_layer.{weight,bias})", name);
    AMTX_REQUIRE(numel == it->second, "amtx_tab_model_set_tensor: '%s' has %lld elements, this model needs %lld", name, (long long)numel, (long long)it->second);
    m->store.set(name, host_data, numel);
    m->finalized = false;
    return AMTX_OK;
}

extern "C" int amtx_tab_model_finalize(amtx_tab_model* m) {
    AMTX_REQUIRE(m, "amtx_tab_model_finalize: null model");
    int rc;
    for (const auto& kv : m->expected) {
        const float* unused;
        if ((rc = m->store.need(kv.first, (size_t)kv.second, &unused)) != AMTX_OK) return rc;
    }
    if ((rc = amtx_quiesce_before_resync(m->w1.p != nullptr)) != AMTX_OK) return rc;
    std::map<std::string, std::vector<float>>& tensors = m->store.host;
    const int P = m->planes, cin = m->in_channels;
    auto plane_of = [](float x, int p) -> bf16_t {
        const bf16_t hi = f32_to_bf16_rn(x);
        return p == 0 ? hi : f32_to_bf16_rn(x - bf16_to_f32(hi));
    };
    // conv1: [c*9 + kf*3 + kt][32] fp32
    const std::vector<float>& c1 = tensors["conv.0.weight"];
    std::vector<float> w1((size_t)cin * 9 * TAB_C1);
    for (int o = 0; o < TAB_C1; ++o)
        for (int k = 0; k < cin * 9; ++k) w1[(size_t)k * TAB_C1 + o] = c1[(size_t)o * cin * 9 + k];
    // conv2 / conv3: MFMA A fragments [plane][wave][k-step][lane][8]; lane l holds output channel 16*wave + (l & 15) and the 8 input
    // channels 8*(l >> 4) .. +7 of k-step s (conv2: tap s; conv3: tap s/2, channels 32*(s&1) + ...)
    auto pack_conv = [&](const std::vector<float>& wt, int c_in, int steps, std::vector<bf16_t>& out) {
        out.assign((size_t)P * 4 * steps * 64 * 8, 0);
        const int per_tap = c_in / 32;
        for (int p = 0; p < P; ++p)
            for (int wv = 0; wv < 4; ++wv)
                for (int s = 0; s < steps; ++s)
                    for (int l = 0; l < 64; ++l)
                        for (int j = 0; j < 8; ++j) {
                            const int tap = s / per_tap, ci = 32 * (s % per_tap) + 8 * (l >> 4) + j, o = 16 * wv + (l & 15);
                            out[((((size_t)p * 4 + wv) * steps + s) * 64 + l) * 8 + j] = plane_of(wt[((size_t)o * c_in + ci) * 9 + tap], p);
                        }
    };
    std::vector<bf16_t> w2, w3;
    pack_conv(tensors["conv.2.weight"], TAB_C1, 9, w2);
    pack_conv(tensors["conv.4.weight"], TAB_C2, 18, w3);
    // fc: columns permuted from the reference's flatten order (c * H + h) to the engine's (h * 64 + c)
    const std::vector<float>& fw = tensors["dense.0.weight"];
    std::vector<float> wp((size_t)TAB_FC * m->K);
    for (int n = 0; n < TAB_FC; ++n)
        for (int c = 0; c < TAB_C2; ++c)
            for (int h = 0; h < m->H; ++h) wp[(size_t)n * m->K + h * TAB_C2 + c] = fw[(size_t)n * m->K + c * m->H + h];
    amtx_gemm_pack_dims(TAB_FC, m->K, &m->fc_npad, &m->fc_kpad);
    std::vector<bf16_t> fcp((size_t)P * m->fc_npad * m->fc_kpad);
    amtx_gemm_pack_host(wp.data(), m->K, TAB_FC, m->K, P, fcp.data());
#define TAB_UP(buf, vec) if ((rc = m->buf.upload((vec).data(), (vec).size() * sizeof((vec)[0]))) != AMTX_OK) return rc
    TAB_UP(w1, w1);
    TAB_UP(b1, tensors["conv.0.bias"]);
    TAB_UP(w2, w2);
    TAB_UP(b2, tensors["conv.2.bias"]);
    TAB_UP(w3, w3);
    TAB_UP(b3, tensors["conv.4.bias"]);
    TAB_UP(fcw, fcp);
    TAB_UP(fcb, tensors["dense.0.bias"]);
    TAB_UP(hw, tensors["dense.3.output_layer.weight"]);
    TAB_UP(hb, tensors["dense.3.output_layer.bias"]);
#undef TAB_UP
    m->finalized = true;
    return AMTX_OK;
}

namespace {
struct TabLayout { bf16_t *y2, *e; float* h1; size_t total; int64_t y2_elems, e_elems; };
TabLayout tab_layout(const amtx_tab_model* m, int64_t batch, int64_t num_windows, void* base) {
    TabLayout L;
    const size_t es = m->planes == 2 ? 4 : 2;     // bf16, or the two planes of a split element
    L.y2_elems = batch * (num_windows + 4) * (m->dim_in - 4) * TAB_C2;
    L.e_elems = batch * num_windows * m->K;
    WorkspaceCarver ws{static_cast<char*>(base)};
    L.y2 = reinterpret_cast<bf16_t*>(ws.take(L.y2_elems * es));
    L.e = reinterpret_cast<bf16_t*>(ws.take(L.e_elems * es));
    L.h1 = reinterpret_cast<float*>(ws.take(batch * num_windows * TAB_FC * 4));
    L.total = ws.off;
    return L;
}
}  // namespace

extern "C" size_t amtx_tab_workspace_bytes(const amtx_tab_model* m, int batch, int num_windows) {
    if (!m || batch <= 0 || num_windows <= 0) return 0;
    return tab_layout(m, batch, num_windows, nullptr).total;
}

extern "C" int amtx_tab_forward(const amtx_tab_model* m, const float* feats, int64_t stride_b, int64_t stride_c, int64_t stride_f, int64_t stride_t,
                                int batch, int num_windows, void* workspace, size_t workspace_bytes, float* logits, int64_t* tablature, void* stream) {
    AMTX_REQUIRE(m && m->finalized, "amtx_tab_forward: model missing or not finalized");
    AMTX_REQUIRE(feats && workspace, "amtx_tab_forward: null features or workspace");
    AMTX_REQUIRE(logits || tablature, "amtx_tab_forward: no output requested");
    AMTX_REQUIRE(batch > 0 && batch <= 65535 && num_windows > 0, "amtx_tab_forward: bad batch / num_windows (%d, %d)", batch, num_windows);
    AMTX_REQUIRE((int64_t)batch * num_windows < (1ll << 31), "amtx_tab_forward: batch x num_windows must be below 2^31");
    AMTX_REQUIRE(((uintptr_t)workspace % 256) == 0, "amtx_tab_forward: workspace must be 256-byte aligned");
    const TabLayout L = tab_layout(m, batch, num_windows, workspace);
    AMTX_REQUIRE(workspace_bytes >= L.total, "amtx_tab_forward: workspace of %zu bytes, %zu needed", workspace_bytes, L.total);
    hipStream_t st = (hipStream_t)stream;
    bf16_t *y2 = L.y2, *e = L.e;
    float* h1 = L.h1;
    const int F = m->dim_in, F2 = F - 4, T = num_windows, T2 = T + 4;
    const bool x3 = m->planes == 2;

    Conv12Args a;
    a.feats = feats; a.sb = stride_b; a.sc = stride_c; a.sf = stride_f; a.st = stride_t;
    a.c_in = m->in_channels; a.F = F; a.cols = T + 8;
    a.w1 = (const float*)m->w1.p; a.b1 = (const float*)m->b1.p; a.w2frag = (const bf16_t*)m->w2.p; a.b2 = (const float*)m->b2.p;
    a.y2 = y2; a.y2_split = L.y2_elems; a.T2 = T2; a.F2 = F2;
    const size_t lds1 = conv12_lds(m->in_channels, m->planes);
    const dim3 g1((T2 + TAB_TT - 1) / TAB_TT, (F2 + TAB_TF - 1) / TAB_TF, batch);
    if (x3) {
        AMTX_GRANT_LDS(tab_conv12_kernel<2>, lds1);
        hipLaunchKernelGGL(tab_conv12_kernel<2>, g1, dim3(TAB_THREADS), lds1, st, a);
    } else {
        AMTX_GRANT_LDS(tab_conv12_kernel<1>, lds1);
        hipLaunchKernelGGL(tab_conv12_kernel<1>, g1, dim3(TAB_THREADS), lds1, st, a);
    }
    AMTX_CHECK_LAUNCH();

    Conv3Args c;
    c.y2 = y2; c.y2_split = L.y2_elems; c.T2 = T2; c.F2 = F2;
    c.w3frag = (const bf16_t*)m->w3.p; c.b3 = (const float*)m->b3.p;
    c.e = e; c.e_split = L.e_elems; c.T = T; c.H = m->H; c.K = m->K;
    const size_t lds3 = conv3_lds(m->planes);
    const dim3 g3((T + TAB_TT - 1) / TAB_TT, (F2 - 2 + TAB_TF - 1) / TAB_TF, batch);
    if (x3) {
        AMTX_GRANT_LDS(tab_conv3_kernel<2>, lds3);
        hipLaunchKernelGGL(tab_conv3_kernel<2>, g3, dim3(TAB_THREADS), lds3, st, c);
    } else {
        AMTX_GRANT_LDS(tab_conv3_kernel<1>, lds3);
        hipLaunchKernelGGL(tab_conv3_kernel<1>, g3, dim3(TAB_THREADS), lds3, st, c);
    }
    AMTX_CHECK_LAUNCH();

    const int64_t M = (int64_t)batch * T;
    GemmArgs g;
    g.A = e; g.lda = m->K; g.a_type = x3 ? AMTX_T_SPLIT : AMTX_T_BF16; g.a_split = x3 ? L.e_elems : 0;
    g.W = (const bf16_t*)m->fcw.p; g.planes = m->planes; g.n_pad = m->fc_npad; g.k_pad = m->fc_kpad;
    g.bias = (const float*)m->fcb.p; g.C = h1; g.ldc = TAB_FC; g.c_type = AMTX_T_F32; g.M = M; g.N = TAB_FC; g.K = m->K;
    g.groups = 1; g.a_gs = g.w_gs = g.bias_gs = g.c_gs = 0;
    int rc = amtx_launch_gemm(g, st);
    if (rc != AMTX_OK) return rc;

    hipLaunchKernelGGL(tab_head_kernel, dim3((unsigned)((M + TAB_HEAD_ROWS - 1) / TAB_HEAD_ROWS)), dim3(TAB_THREADS), 0, st, h1, (const float*)m->hw.p,
                       (const float*)m->hb.p, logits, tablature, M, T, m->G, m->C);
    AMTX_CHECK_LAUNCH();
    return AMTX_OK;
}
