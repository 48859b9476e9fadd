// A grid of decision thresholds on probability maps (include/amtx_thrgrid.h): what choosing the onset and frame thresholds of an
// Onsets & Frames model on a validation split needs from the device, without one roll per threshold.  The cut is pianoroll_kernel's
// (head.hip) on the same float, `s < thr ? 0 : 1` -- written here as !(s < thr), so s == thr and NaN are active -- hence every result is
// bit-equal to thresholding first and running the kernel it restates.
//
// multipitch_grid_counts_kernel   multipitch_counts_kernel (eval.hip) for G <= 32 thresholds in ONE pass over prob and ref: one block of
//                   1024 threads per clip, 16-byte loads with eval.hip's scalar head / tail for a slice off the 16-byte grid.  Per
//                   threshold a cell costs one compare: the wave's 64 verdicts are a ballot mask, and the three sums grow by popcounts of
//                   masks -- wave-uniform integers that need no lane reduction.  The thresholds are unrolled (a uniform branch skips those
//                   at or above G), so the 2 * 32 + 1 counters have static indices.  Sums: per wave in loop order, then the 16 waves in
//                   order by one thread per counter; integers, no atomics.
//
// notes_grid_kernel   the walk of notes_kernel (amtx_notes_walk.h) for P threshold pairs.  A wave owns a (clip, key) row and a TILE of
//                   pairs: it reads a 64-frame chunk of the row's probabilities ONCE (onset, its predecessor, frame) and evaluates the
//                   tile's pairs on it, unrolled, so each pair's walk state has a register of its own.  TILE = 1 is one wave per
//                   (pair, clip, key) -- the default: measured on one 5 000-frame track with 25 pairs it took 40 us against 93 us
//                   (TILE 4) and 138 us (TILE 8); the row stays in cache, and a tile divides the waves in flight by its width
//                   (DESIGN.md 6l).  The wider tiles stay as instantiations for that measurement (notes_grid_tile).

#include "amtx_kernels.h"
#include "amtx_notes_walk.h"

#include <cstdlib>

namespace {

constexpr int GRID_MAX_THRESHOLDS = 32;
constexpr int GRID_COUNT_WAVES = 16;
constexpr int GRID_COUNTERS = 2 * GRID_MAX_THRESHOLDS + 1;        // [2g] both, [2g + 1] estimate, [64] reference

__global__ __launch_bounds__(GRID_COUNT_WAVES * 64) void multipitch_grid_counts_kernel(const float* __restrict__ prob, const float* __restrict__ ref,
                                                                                      int64_t n, const float* __restrict__ thresholds, int G,
                                                                                      long long* __restrict__ counts) {
    __shared__ unsigned part[GRID_COUNT_WAVES][GRID_COUNTERS];
    const int64_t row = blockIdx.x;
    const float* e = prob + row * n;
    const float* r = ref + row * n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int NT = GRID_COUNT_WAVES * 64;
    float thr[GRID_MAX_THRESHOLDS];
    unsigned both[GRID_MAX_THRESHOLDS], est[GRID_MAX_THRESHOLDS], refc = 0u;       // per WAVE (n < 2^31 cells per clip)
#pragma unroll
    for (int g = 0; g < GRID_MAX_THRESHOLDS; ++g) {
        thr[g] = g < G ? thresholds[g] : 0.f;
        both[g] = est[g] = 0u;
    }
    // every lane of a wave calls this together; a lane without a cell passes valid = false
    auto cell = [&](bool valid, float s, float b) {
        const unsigned long long rmask = __ballot(valid && b != 0.f);
        refc += (unsigned)__builtin_popcountll(rmask);
#pragma unroll
        for (int g = 0; g < GRID_MAX_THRESHOLDS; ++g) {
            if (g < G) {
                const unsigned long long emask = __ballot(valid && !(s < thr[g]));
                est[g] += (unsigned)__builtin_popcountll(emask);
                both[g] += (unsigned)__builtin_popcountll(emask & rmask);
            }
        }
    };
    const uintptr_t ae = (uintptr_t)e, ar = (uintptr_t)r;
    if (((ae ^ ar) & 15) == 0) {
        int64_t head = (int64_t)(((16 - (ae & 15)) & 15) >> 2);  // floats in front of the first 16-byte boundary
        if (head > n) head = n;
        const int64_t nvec = (n - head) >> 2;
        if (wave == 0) {
            const bool v = lane < head;
            cell(v, v ? e[lane] : 0.f, v ? r[lane] : 0.f);
        }
        const float4* e4 = reinterpret_cast<const float4*>(e + head);
        const float4* r4 = reinterpret_cast<const float4*>(r + head);
        for (int64_t base = (int64_t)wave * 64; base < nvec; base += NT) {          // wave-uniform trip count
            const int64_t i = base + lane;
            const bool v = i < nvec;
            const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 a = v ? e4[i] : zero, b = v ? r4[i] : zero;
            cell(v, a.x, b.x);
            cell(v, a.y, b.y);
            cell(v, a.z, b.z);
            cell(v, a.w, b.w);
        }
        if (wave == 0) {
            const int64_t tail = head + nvec * 4 + lane;         // at most 3 cells
            const bool v = tail < n;
            cell(v, v ? e[tail] : 0.f, v ? r[tail] : 0.f);
        }
    } else {
        for (int64_t base = (int64_t)wave * 64; base < n; base += NT) {
            const int64_t i = base + lane;
            const bool v = i < n;
            cell(v, v ? e[i] : 0.f, v ? r[i] : 0.f);
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int g = 0; g < GRID_MAX_THRESHOLDS; ++g) {
            part[wave][2 * g] = both[g];
            part[wave][2 * g + 1] = est[g];
        }
        part[wave][2 * GRID_MAX_THRESHOLDS] = refc;
    }
    __syncthreads();
    if (tid < 3 * G) {
        const int g = tid / 3, which = tid - 3 * g;
        const int c = which == 2 ? 2 * GRID_MAX_THRESHOLDS : 2 * g + which;
        long long s = 0;
        for (int w = 0; w < GRID_COUNT_WAVES; ++w) s += part[w][c];                 // fixed order
        counts[(row * G + g) * 3 + which] = s;
    }
}

template <int TILE>
__global__ __launch_bounds__(256) void notes_grid_kernel(const float* __restrict__ on_prob, const float* __restrict__ mp_prob, int rows, int T,
                                                         const float2* __restrict__ pairs_thr, int P, int cap, int2* __restrict__ pairs,
                                                         int* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int p0 = blockIdx.y * TILE;
    const bool use_onsets = on_prob != nullptr;
    const float* on = (use_onsets ? on_prob : mp_prob) + (int64_t)row * T;
    const float* act = mp_prob + (int64_t)row * T;
    float othr[TILE], fthr[TILE];
    NotesWalk w[TILE];
#pragma unroll
    for (int i = 0; i < TILE; ++i) {
        const float2 pr = pairs_thr[min(p0 + i, P - 1)];
        fthr[i] = pr.y;
        othr[i] = use_onsets ? pr.x : pr.y;                      // derived onsets: the frame roll is the onset map
        w[i] = notes_walk_begin(T);
    }
    const int nchunks = (T + 63) >> 6;
    for (int ch = nchunks - 1; ch >= 0; --ch) {
        const int t = ch * 64 + lane;
        const bool valid = t < T;
        const float o = valid ? on[t] : 0.f;
        const float oprev = (valid && t > 0) ? on[t - 1] : 0.f;
        const float a = valid ? act[t] : 0.f;
#pragma unroll
        for (int i = 0; i < TILE; ++i) {
            if (p0 + i < P) {                                    // uniform
                // the rolls notes_kernel reads, cut here: o - oprev > 0 on {0, 1} is "on now, off before"; frame 0 has no predecessor
                const bool ob = !(o < othr[i]);
                const bool pb = t > 0 && !(oprev < othr[i]);
                const bool imp = valid && ob && !pb;
                const bool active = valid && (!(a < fthr[i]) || (use_onsets && ob));
                notes_walk_chunk(w[i], ch, lane, valid, imp, active, cap, pairs + ((int64_t)(p0 + i) * rows + row) * cap);
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < TILE; ++i)
            if (p0 + i < P) counts[(int64_t)(p0 + i) * rows + row] = w[i].n;
    }
}

// Pairs per wave.  AMTX_NOTES_GRID_TILE (1, 2, 4 or 8) picks another instantiation for a measurement (tools/bench_sweep_tracks.py); the
// results are the same bits whatever the tile.
int notes_grid_tile() {
    static const int tile = [] {
        const char* s = std::getenv("AMTX_NOTES_GRID_TILE");
        const int v = s ? std::atoi(s) : 0;
        return (v == 1 || v == 2 || v == 4 || v == 8) ? v : 1;
    }();
    return tile;
}

template <int TILE>
void launch_notes_grid(const float* on_prob, const float* mp_prob, int rows, int T, const float* pairs_thr, int P, int cap, int32_t* pairs,
                       int32_t* counts, hipStream_t stream) {
    hipLaunchKernelGGL(notes_grid_kernel<TILE>, dim3((unsigned)((rows + 3) / 4), (unsigned)((P + TILE - 1) / TILE)), dim3(256), 0, stream, on_prob, mp_prob,
                       rows, T, reinterpret_cast<const float2*>(pairs_thr), P, cap, reinterpret_cast<int2*>(pairs), counts);
}

}  // namespace

extern "C" int amtx_eval_multipitch_grid_counts(const float* prob, const float* ref, int batch, int keys, int num_frames, const float* thresholds,
                                                int G, int64_t* counts, void* stream_) {
    AMTX_REQUIRE(prob && ref && thresholds && counts, "amtx_eval_multipitch_grid_counts: null pointer");
    AMTX_REQUIRE(batch > 0 && keys > 0 && num_frames > 0, "amtx_eval_multipitch_grid_counts: bad sizes");
    AMTX_REQUIRE(G >= 1 && G <= GRID_MAX_THRESHOLDS, "amtx_eval_multipitch_grid_counts: %d thresholds (1 to %d)", G, GRID_MAX_THRESHOLDS);
    AMTX_REQUIRE(((uintptr_t)prob | (uintptr_t)ref | (uintptr_t)thresholds) % 4 == 0 && (uintptr_t)counts % 8 == 0,
                 "amtx_eval_multipitch_grid_counts: misaligned pointer");
    AMTX_REQUIRE((int64_t)keys * num_frames < (1ll << 31), "amtx_eval_multipitch_grid_counts: %d x %d cells per clip: too many", keys, num_frames);
    hipLaunchKernelGGL(multipitch_grid_counts_kernel, dim3((unsigned)batch), dim3(GRID_COUNT_WAVES * 64), 0, (hipStream_t)stream_, prob, ref,
                       (int64_t)keys * num_frames, thresholds, G, (long long*)counts);
    AMTX_CHECK_LAUNCH();
    return AMTX_OK;
}

extern "C" int amtx_notes_decode_grid(const float* on_prob, const float* mp_prob, int batch, int keys, int num_frames, const float* pairs_thr, int P,
                                      int capacity, int32_t* pairs, int32_t* counts, void* stream_) {
    AMTX_REQUIRE(mp_prob && pairs_thr && pairs && counts, "amtx_notes_decode_grid: null pointer");
    AMTX_REQUIRE(batch > 0 && keys > 0 && num_frames > 0 && capacity > 0 && P > 0, "amtx_notes_decode_grid: bad sizes");
    AMTX_REQUIRE((uintptr_t)pairs_thr % 8 == 0 && (uintptr_t)pairs % 8 == 0, "amtx_notes_decode_grid: misaligned pointer");
    AMTX_REQUIRE((int64_t)batch * keys * P < (1ll << 31) && P < 65536,"amtx_notes_decode_grid: %d pairs x %d x %d rows: too many", P, batch, keys);
    const int rows = batch * keys;
    hipStream_t stream = (hipStream_t)stream_;
    switch (notes_grid_tile()) {
        case 2: launch_notes_grid<2>(on_prob, mp_prob, rows, num_frames, pairs_thr, P, capacity, pairs, counts, stream); break;
        case 4: launch_notes_grid<4>(on_prob, mp_prob, rows, num_frames, pairs_thr, P, capacity, pairs, counts, stream); break;
        case 8: launch_notes_grid<8>(on_prob, mp_prob, rows, num_frames, pairs_thr, P, capacity, pairs, counts, stream); break;
        default: launch_notes_grid<1>(on_prob, mp_prob, rows, num_frames, pairs_thr, P, capacity, pairs, counts, stream); break;
    }
    AMTX_CHECK_LAUNCH();
    return AMTX_OK;
}
