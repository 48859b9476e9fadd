// The parameter update of a training step: Adam and Adadelta over a table of tensors in one launch, the global gradient norm for
// clipping (include/amtx_optim.h, amt_tools_amd/optim.py).
//
// A block of OPTIM_THREADS lanes owns one chunk of AMTX_OPTIM_CHUNK consecutive elements of ONE tensor.  The table (addresses, numels, the
// first block of every tensor) is a kernel argument: a block finds its tensor with a wave-uniform binary search over the block prefix
// (scalar loads from the kernel-argument segment, ceil(log2(tensors)) of them), then every lane issues all the loads of its 16 elements
// (param, grad and two state maps: 16 x 16 bytes or 64 x 4 bytes in flight per lane, 64 KiB per block), computes, and stores param and the
// state maps back.  A tensor whose four addresses are 16-byte aligned moves as float4; any other (a gradient that is a view at an odd
// offset of DataParallelOptimizer's flat buffer) one element per lane.  A chunk starts a multiple of 16 KiB into its tensor, so the
// tensor's alignment is every chunk's.  Every element is read and written by exactly one lane: no atomics, no workspace, no LDS.
//
// The arithmetic follows torch's multi-tensor updates operation by operation (each _foreach_ call rounds to float32 once; an a + s * b
// of theirs is one fused multiply-add, an addcmul a + s * (b * c) with the product rounded first), so that the result is torch's GPU
// step's, bit for bit where the division and square root round alike.  HBM-bound: Adam and Adadelta read 4 and write 3 floats per element, 28 bytes.
#include "amtx_common.h"
#include "../../include/amtx_optim.h"

#include <math.h>

#include <algorithm>

// torch's operations round one by one: nothing below is fused that is not written as fmaf
#pragma clang fp contract(off)

#define OPTIM_THREADS 256
#define OPTIM_PER_LANE (AMTX_OPTIM_CHUNK / OPTIM_THREADS)      // 16 elements = 4 float4
#define OPTIM_FINAL_THREADS 1024
static_assert(AMTX_OPTIM_CHUNK % (4 * OPTIM_THREADS) == 0, "a chunk is whole float4 rounds of the block");

struct OptimTable {
    float* param[AMTX_OPTIM_MAX_TENSORS];
    const float* grad[AMTX_OPTIM_MAX_TENSORS];
    float* state_a[AMTX_OPTIM_MAX_TENSORS];
    float* state_b[AMTX_OPTIM_MAX_TENSORS];
    int64_t numel[AMTX_OPTIM_MAX_TENSORS];
    int block_first[AMTX_OPTIM_MAX_TENSORS + 1];      // ascending; tensor t owns the blocks [block_first[t], block_first[t + 1])
    int num_tensors;
    unsigned char vec[AMTX_OPTIM_MAX_TENSORS];        // the float4 path
};
static_assert(sizeof(OptimTable) <= 3584, "the table is a kernel argument: it has to fit the 4 KiB of the argument segment with the scalars");

// The last tensor whose first block is <= bid: a tensor without blocks (numel 0) shares its first block with its successor and is never
// the last.  Wave-uniform: bid is blockIdx.x.
static __device__ __forceinline__ int optim_tensor_of(const OptimTable& T, int bid) {
    int lo = 0, n = T.num_tensors;
    while (n > 1) {
        const int half = n >> 1;
        if (T.block_first[lo + half] <= bid) lo += half;
        n -= half;
    }
    return lo;
}

// torch._foreach_* sequence of _multi_tensor_adam (amsgrad off, maximize off); scalars are torch's: doubles rounded to float once.
struct AdamOp {
    float weight, beta2, one_minus_beta2, bc2_sqrt, eps, neg_step, weight_decay;
    __device__ __forceinline__ void operator()(float& p, float g, float& m, float& v) const {
#pragma clang fp contract(off)
        if (weight_decay != 0.0f) g = fmaf(weight_decay, p, g);
        const float diff = g - m;                                            // lerp(m, g, weight)
        m = fabsf(weight) < 0.5f ? fmaf(weight, diff, m) : g - diff * (1.0f - weight);
        v = v * beta2;
        v = fmaf(one_minus_beta2, g * g, v);                              // addcmul: a + value * (t1 * t2)
        const float denom = sqrtf(v) / bc2_sqrt + eps;
        p = fmaf(neg_step, m / denom, p);
    }
};

// _multi_tensor_adadelta (maximize off): a = square_avg, b = acc_delta
struct AdadeltaOp {
    float rho, one_minus_rho, eps, neg_lr, weight_decay;
    __device__ __forceinline__ void operator()(float& p, float g, float& sq, float& acc) const {
#pragma clang fp contract(off)
        if (weight_decay != 0.0f) g = fmaf(weight_decay, p, g);
        sq = sq * rho;
        sq = fmaf(one_minus_rho, g * g, sq);
        const float std_ = sqrtf(sq + eps);
        float delta = sqrtf(acc + eps) / std_;
        delta = delta * g;
        acc = acc * rho;
        acc = fmaf(one_minus_rho, delta * delta, acc);
        p = fmaf(neg_lr, delta, p);
    }
};

template <class Op>
__global__ __launch_bounds__(OPTIM_THREADS) void optim_step_kernel(const OptimTable T, const Op op, const float* __restrict__ sumsq, float max_norm) {
    const int tid = threadIdx.x, bid = blockIdx.x;
    const int t = optim_tensor_of(T, bid);
    const int64_t base = (int64_t)(bid - T.block_first[t]) * AMTX_OPTIM_CHUNK;
    const int64_t left = T.numel[t] - base;
    const int cnt = left < AMTX_OPTIM_CHUNK ? (int)left : AMTX_OPTIM_CHUNK;      // 1 .. CHUNK elements of this block
    float* __restrict__ p = T.param[t] + base;
    const float* __restrict__ g = T.grad[t] + base;
    float* __restrict__ a = T.state_a[t] + base;
    float* __restrict__ b = T.state_b[t] + base;
    // clip_grad_norm_'s coefficient (norm_type 2) from the device scalar; * 1 is exact, so an unclipped step reads the gradient's own bits
    float coef = 1.0f;
    if (sumsq) coef = fminf(1.0f, max_norm / (sqrtf(*sumsq) + 1e-6f));

    if (T.vec[t]) {
        float4 pv[OPTIM_PER_LANE / 4], gv[OPTIM_PER_LANE / 4], av[OPTIM_PER_LANE / 4], bv[OPTIM_PER_LANE / 4];
#pragma unroll
        for (int i = 0; i < OPTIM_PER_LANE / 4; ++i) {
            const int e = (i * OPTIM_THREADS + tid) * 4;
            if (e + 4 <= cnt) {
                pv[i] = *reinterpret_cast<const float4*>(p + e);
                gv[i] = *reinterpret_cast<const float4*>(g + e);
                av[i] = *reinterpret_cast<const float4*>(a + e);
                bv[i] = *reinterpret_cast<const float4*>(b + e);
            }
        }
#pragma unroll
        for (int i = 0; i < OPTIM_PER_LANE / 4; ++i) {
            const int e = (i * OPTIM_THREADS + tid) * 4;
            if (e + 4 <= cnt) {
                op(pv[i].x, gv[i].x * coef, av[i].x, bv[i].x);
                op(pv[i].y, gv[i].y * coef, av[i].y, bv[i].y);
                op(pv[i].z, gv[i].z * coef, av[i].z, bv[i].z);
                op(pv[i].w, gv[i].w * coef, av[i].w, bv[i].w);
                *reinterpret_cast<float4*>(p + e) = pv[i];
                *reinterpret_cast<float4*>(a + e) = av[i];
                *reinterpret_cast<float4*>(b + e) = bv[i];
            }
        }
        const int whole = cnt & ~3;                  // the 1 .. 3 elements behind the tensor's last whole float4
        if (tid < cnt - whole) {
            const int e = whole + tid;
            float pe = p[e], ae = a[e], be = b[e];
            op(pe, g[e] * coef, ae, be);
            p[e] = pe, a[e] = ae, b[e] = be;
        }
    } else {
        float pv[OPTIM_PER_LANE], gv[OPTIM_PER_LANE], av[OPTIM_PER_LANE], bv[OPTIM_PER_LANE];
#pragma unroll
        for (int i = 0; i < OPTIM_PER_LANE; ++i) {
            const int e = i * OPTIM_THREADS + tid;
            if (e < cnt) pv[i] = p[e], gv[i] = g[e], av[i] = a[e], bv[i] = b[e];
        }
#pragma unroll
        for (int i = 0; i < OPTIM_PER_LANE; ++i) {
            const int e = i * OPTIM_THREADS + tid;
            if (e < cnt) {
                op(pv[i], gv[i] * coef, av[i], bv[i]);
                p[e] = pv[i], a[e] = av[i], b[e] = bv[i];
            }
        }
    }
}

// partials[bid] = the sum of g * g over the block's chunk: per lane in element order, then the wave butterfly, then the four waves in order
__global__ __launch_bounds__(OPTIM_THREADS) void optim_sumsq_kernel(const OptimTable T, float* __restrict__ partials) {
    __shared__ float waves[OPTIM_THREADS / 64];
    const int tid = threadIdx.x, bid = blockIdx.x;
    const int t = optim_tensor_of(T, bid);
    const int64_t base = (int64_t)(bid - T.block_first[t]) * AMTX_OPTIM_CHUNK;
    const int64_t left = T.numel[t] - base;
    const int cnt = left < AMTX_OPTIM_CHUNK ? (int)left : AMTX_OPTIM_CHUNK;
    const float* __restrict__ g = T.grad[t] + base;
    float s = 0.0f;
    if (T.vec[t]) {
        float4 gv[OPTIM_PER_LANE / 4];
#pragma unroll
        for (int i = 0; i < OPTIM_PER_LANE / 4; ++i) {
            const int e = (i * OPTIM_THREADS + tid) * 4;
            gv[i] = e + 4 <= cnt ? *reinterpret_cast<const float4*>(g + e) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
#pragma unroll
        for (int i = 0; i < OPTIM_PER_LANE / 4; ++i) s += (gv[i].x * gv[i].x + gv[i].y * gv[i].y) + (gv[i].z * gv[i].z + gv[i].w * gv[i].w);
        const int whole = cnt & ~3;
        if (tid < cnt - whole) s += g[whole + tid] * g[whole + tid];
    } else {
        float gv[OPTIM_PER_LANE];
#pragma unroll
        for (int i = 0; i < OPTIM_PER_LANE; ++i) {
            const int e = i * OPTIM_THREADS + tid;
            gv[i] = e < cnt ? g[e] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < OPTIM_PER_LANE; ++i) s += gv[i] * gv[i];
    }
    s = wave_sum_f32(s);
    if ((tid & 63) == 0) waves[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) partials[bid] = (waves[0] + waves[1]) + (waves[2] + waves[3]);
}

// out[0] = the partials added in a fixed order (lane i takes i, i + 1024, ...; then a tree over the lanes), out[1] = its square root
__global__ __launch_bounds__(OPTIM_FINAL_THREADS) void optim_sumsq_final_kernel(const float* __restrict__ partials, int64_t n, float* __restrict__ out) {
    __shared__ float tree[OPTIM_FINAL_THREADS];
    const int tid = threadIdx.x;
    float s = 0.0f;
    for (int64_t i = tid; i < n; i += OPTIM_FINAL_THREADS) s += partials[i];
    tree[tid] = s;
    __syncthreads();
    for (int width = OPTIM_FINAL_THREADS / 2; width > 0; width >>= 1) {
        if (tid < width) tree[tid] += tree[tid + width];
        __syncthreads();
    }
    if (tid == 0) out[0] = tree[0], out[1] = sqrtf(tree[0]);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Host side: checks -> route -> launch.  The route is a function of the numels and of the addresses' alignment alone: it dereferences
// no tensor, launches nothing and reads no environment.

// One launch: the tensors it takes from the front of the table, their blocks and their path.
struct OptimRoute {
    const char* error = nullptr;      // a refusal: amtx_last_error's text, with AMTX_ERR_ARG
    int count = 0;                    // tensors of this launch: min(remaining, AMTX_OPTIM_MAX_TENSORS), fewer where the blocks would not fit an int
    int64_t blocks = 0;               // grid; 0: nothing to launch (every tensor of the run is empty)
    int block_first[AMTX_OPTIM_MAX_TENSORS + 1] = {0};
    unsigned char vec[AMTX_OPTIM_MAX_TENSORS] = {0};
};
// numels / aligned16: of the remaining tensors (aligned16[t]: every address of tensor t the kernel touches is 16-byte aligned; null: none is)
OptimRoute optim_route(const int64_t* numels, const unsigned char* aligned16, int64_t remaining) {
    OptimRoute r;
    const int64_t max_blocks = 0x7fffffff;
    for (; r.count < remaining && r.count < AMTX_OPTIM_MAX_TENSORS; ++r.count) {
        const int64_t n = numels[r.count];
        if (n < 0) {
            r.error = "optim: a negative numel";
            return r;
        }
        const int64_t chunks = n / AMTX_OPTIM_CHUNK + (n % AMTX_OPTIM_CHUNK != 0);
        if (chunks > max_blocks) {
            r.error = "optim: a tensor with more chunks than one launch has blocks";
            return r;
        }
        if (r.blocks + chunks > max_blocks) break;      // r.count >= 1 here: the next launch starts with this tensor
        r.block_first[r.count] = (int)r.blocks;
        r.vec[r.count] = aligned16 != nullptr && aligned16[r.count] != 0;
        r.blocks += chunks;
    }
    for (int t = r.count; t <= AMTX_OPTIM_MAX_TENSORS; ++t) r.block_first[t] = (int)r.blocks;
    return r;
}

// launches and blocks of a whole table
static int optim_count(const char* who, const int64_t* numels, int64_t num_tensors, int64_t* launches, int64_t* blocks) {
    AMTX_REQUIRE(num_tensors >= 0 && num_tensors <= 0x7fffffff, "%s: num_tensors=%lld: between 0 and 2^31 - 1", who, (long long)num_tensors);
    AMTX_REQUIRE(numels || num_tensors == 0, "%s: null argument", who);
    *launches = *blocks = 0;
    for (int64_t t0 = 0; t0 < num_tensors;) {
        const OptimRoute r = optim_route(numels + t0, nullptr, num_tensors - t0);
        AMTX_REQUIRE(!r.error, "%s: %s (tensor %lld)", who, r.error, (long long)(t0 + r.count));
        *launches += r.blocks > 0;
        *blocks += r.blocks;
        t0 += r.count;
    }
    return AMTX_OK;
}

extern "C" int amtx_optim_num_launches(const int64_t* numels, int64_t num_tensors) {
    int64_t launches, blocks;
    const int rc = optim_count("amtx_optim_num_launches", numels, num_tensors, &launches, &blocks);
    return rc != AMTX_OK ? rc : (int)launches;
}

extern "C" int64_t amtx_optim_num_blocks(const int64_t* numels, int64_t num_tensors) {
    int64_t launches, blocks;
    const int rc = optim_count("amtx_optim_num_blocks", numels, num_tensors, &launches, &blocks);
    return rc != AMTX_OK ? rc : blocks;
}

// The checks every entry point makes before anything is launched.  columns: how many of the four addresses its kernel touches
// (4: the update; the sum of squares reads the gradient alone and passes grad_only).
static int optim_check_table(const char* who, const int64_t* table, int64_t num_tensors, bool grad_only) {
    AMTX_REQUIRE(num_tensors >= 0 && num_tensors <= 0x7fffffff, "%s: num_tensors=%lld: between 0 and 2^31 - 1", who, (long long)num_tensors);
    AMTX_REQUIRE(table || num_tensors == 0, "%s: null table", who);
    for (int64_t t = 0; t < num_tensors; ++t) {
        const int64_t* row = table + t * 5;
        AMTX_REQUIRE(row[4] >= 0, "%s: tensor %lld: numel=%lld", who, (long long)t, (long long)row[4]);
        if (row[4] == 0) continue;
        AMTX_REQUIRE(row[1] != 0 && (grad_only || (row[0] != 0 && row[2] != 0 && row[3] != 0)), "%s: tensor %lld: null pointer", who, (long long)t);
        AMTX_REQUIRE(((row[1] | (grad_only ? 0 : row[0] | row[2] | row[3])) & 3) == 0, "%s: tensor %lld: an address that is not 4-byte aligned", who,
                     (long long)t);
    }
    return AMTX_OK;
}

// Fills the kernel argument of the launch that starts at row t0; returns its route.
static OptimRoute optim_fill(const int64_t* table, int64_t t0, int64_t num_tensors, bool grad_only, OptimTable* T) {
    int64_t numels[AMTX_OPTIM_MAX_TENSORS];
    unsigned char aligned[AMTX_OPTIM_MAX_TENSORS];
    const int64_t take = std::min<int64_t>(num_tensors - t0, AMTX_OPTIM_MAX_TENSORS);
    for (int64_t i = 0; i < take; ++i) {
        const int64_t* row = table + (t0 + i) * 5;
        numels[i] = row[4];
        aligned[i] = ((row[1] | (grad_only ? 0 : row[0] | row[2] | row[3])) & 15) == 0;
    }
    const OptimRoute r = optim_route(numels, aligned, num_tensors - t0);
    memset(T, 0, sizeof(*T));
    for (int i = 0; i < r.count; ++i) {
        const int64_t* row = table + (t0 + i) * 5;
        T->param[i] = reinterpret_cast<float*>(row[0]);
        T->grad[i] = reinterpret_cast<const float*>(row[1]);
        T->state_a[i] = reinterpret_cast<float*>(row[2]);
        T->state_b[i] = reinterpret_cast<float*>(row[3]);
        T->numel[i] = row[4];
        T->vec[i] = r.vec[i];
    }
    memcpy(T->block_first, r.block_first, sizeof(T->block_first));
    T->num_tensors = r.count;
    return r;
}

template <class Op>
static int optim_step(const char* who, const int64_t* table, int64_t num_tensors, const Op& op, const float* sumsq, double max_norm, void* stream) {
    const int rc = optim_check_table(who, table, num_tensors, false);
    if (rc != AMTX_OK) return rc;
    AMTX_REQUIRE(!sumsq || max_norm >= 0.0, "%s: max_norm=%g: not negative (and a number) when the sum of squares is given", who, max_norm);
    int launches = 0;
    OptimTable T;
    for (int64_t t0 = 0; t0 < num_tensors;) {
        const OptimRoute r = optim_fill(table, t0, num_tensors, false, &T);
        AMTX_REQUIRE(!r.error, "%s: %s", who, r.error);
        if (r.blocks > 0) {
            hipLaunchKernelGGL(optim_step_kernel<Op>, dim3((unsigned)r.blocks), dim3(OPTIM_THREADS), 0, (hipStream_t)stream, T, op, sumsq, (float)max_norm);
            AMTX_CHECK_LAUNCH();
            ++launches;
        }
        t0 += r.count;
    }
    return launches;
}

extern "C" int amtx_optim_adam_step(const int64_t* table, int64_t num_tensors, double step_size, double bias_correction2_sqrt, double beta1,
                                    double beta2, double eps, double weight_decay, const float* sumsq, double max_norm, void* stream) {
    AMTX_REQUIRE(bias_correction2_sqrt > 0.0, "amtx_optim_adam_step: bias_correction2_sqrt=%g: positive", bias_correction2_sqrt);
    AdamOp op;
    op.weight = (float)(1.0 - beta1);
    op.beta2 = (float)beta2;
    op.one_minus_beta2 = (float)(1.0 - beta2);
    op.bc2_sqrt = (float)bias_correction2_sqrt;
    op.eps = (float)eps;
    op.neg_step = (float)-step_size;
    op.weight_decay = (float)weight_decay;
    return optim_step("amtx_optim_adam_step", table, num_tensors, op, sumsq, max_norm, stream);
}

extern "C" int amtx_optim_adadelta_step(const int64_t* table, int64_t num_tensors, double lr, double rho, double eps, double weight_decay,
                                        const float* sumsq, double max_norm, void* stream) {
    AdadeltaOp op;
    op.rho = (float)rho;
    op.one_minus_rho = (float)(1.0 - rho);
    op.eps = (float)eps;
    op.neg_lr = (float)-lr;
    op.weight_decay = (float)weight_decay;
    return optim_step("amtx_optim_adadelta_step", table, num_tensors, op, sumsq, max_norm, stream);
}

extern "C" int amtx_optim_grad_sumsq(const int64_t* table, int64_t num_tensors, float* partials, int64_t partials_elems, float* out, void* stream) {
    const char* who = "amtx_optim_grad_sumsq";
    const int rc = optim_check_table(who, table, num_tensors, true);
    if (rc != AMTX_OK) return rc;
    AMTX_REQUIRE(out, "%s: null out", who);
    // the blocks of all launches, before the first one: partials must hold them all
    int64_t need = 0;
    OptimTable T;
    for (int64_t t0 = 0; t0 < num_tensors;) {
        const OptimRoute r = optim_fill(table, t0, num_tensors, true, &T);
        AMTX_REQUIRE(!r.error, "%s: %s", who, r.error);
        need += r.blocks;
        t0 += r.count;
    }
    AMTX_REQUIRE(need == 0 || (partials && partials_elems >= need), "%s: partials holds %lld floats, the table's blocks need %lld", who,
                 (long long)(partials ? partials_elems : 0), (long long)need);
    int64_t done = 0;
    for (int64_t t0 = 0; t0 < num_tensors;) {
        const OptimRoute r = optim_fill(table, t0, num_tensors, true, &T);
        if (r.blocks > 0) {
            hipLaunchKernelGGL(optim_sumsq_kernel, dim3((unsigned)r.blocks), dim3(OPTIM_THREADS), 0, (hipStream_t)stream, T, partials + done);
            AMTX_CHECK_LAUNCH();
        }
        done += r.blocks;
        t0 += r.count;
    }
    hipLaunchKernelGGL(optim_sumsq_final_kernel, dim3(1), dim3(OPTIM_FINAL_THREADS), 0, (hipStream_t)stream, partials, need, out);
    AMTX_CHECK_LAUNCH();
    return AMTX_OK;
}
