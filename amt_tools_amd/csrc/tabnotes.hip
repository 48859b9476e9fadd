// Tablature decoding on the device: what the reference's guitar experiment runs after TabCNN (examples/papers/tabcnn.py:90-91,
// ComboEstimator([TablatureWrapper, StackedMultiPitchCollapser]), plus StackedNoteTranscriber for note lists).
//
// amtx_tab_expand   tablature [B][S][T] int64 (class -1 = silent) -> stacked multi-pitch [B][S][P][T] fp32 and / or its collapse
//                   (max over strings) [B][P][T] fp32 (tools/utils.py:1988-2059, :1787-1815).  Gather form: every output element asks
//                   "is my pitch row the one string s sounds at frame t", so every element is written exactly once (no memset, nothing
//                   depends on what the buffers held) and no class value, however wrong, can turn into an address.  Lanes along T,
//                   16-byte stores when T is a multiple of 4.  HBM-bound on the writes: 4 (S + 1) P T bytes per clip.
//
// amtx_tab_notes    the same tablature -> note rows [onset_s, offset_s, midi_pitch] (float64), never touching the (P x larger) map.
//                   On ONE string at most one pitch sounds per frame, so tools.multi_pitch_to_notes (utils.py:369-471) on the string's
//                   slice of the stacked map reduces to run lengths of the class row: a note starts where tab[t] >= 0 and (t == 0 or
//                   tab[t-1] != tab[t]) and ends at the next frame whose class differs, or at T.  One wave64 per (clip, string) row walks
//                   the row forward in 64-frame chunks; lane i looks at the boundary in front of frame t = 64 ch + i + 1 (t == T: the end of
//                   the row), a ballot tells every boundary lane where its run began, kept notes are compacted with a prefix popcount.
//                   Two passes over the same walk (count, exclusive scan over the B S rows, write): 8 B per cell are read twice, 24 B per
//                   note written, no atomics.  Onsets of one string sit at distinct frames, so the reference's (unstable) sorts by onset
//                   have nothing to reorder: ascending onset frame IS its order.
//                   inhibition_window (transcribe.py:463-469 -> utils.py:2987-3038): a run whose onset lies inside the window of the last
//                   KEPT onset of the same pitch gives no note at all (the previous note ended at the gap between the two runs; walks
//                   start at kept onsets only).  Lane k of the wave holds, for class k, the first frame outside that window (`release[]`
//                   of the kept onset, a host table: the kernel compares frame indices only); the runs of a chunk -- not its frames --
//                   are resolved in order with wave-uniform steps.  minimum_duration (transcribe.py:39-80, :474-476): offset_s - onset_s in
//                   float64, >= threshold, or > 0 for a threshold of 0; applied after the inhibition, which does not look at durations.

#include "amtx_kernels.h"

#define AMTX_TAB_MAX_STRINGS 16

namespace {

struct TabStrings { int v[AMTX_TAB_MAX_STRINGS]; };

constexpr int EXPAND_PROWS = 4;     // pitch rows per block: 11 x 2 x B blocks at P 44, T 1292 (16-byte stores)

template <int VEC>
__global__ __launch_bounds__(256) void tab_expand_kernel(const int64_t* __restrict__ tab, int S, int T, int P, TabStrings start,
                                                         float* __restrict__ stacked, float* __restrict__ collapsed) {
    const int64_t t0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * VEC;
    if (t0 >= T) return;
    const int b = blockIdx.z;
    const int p0 = blockIdx.y * EXPAND_PROWS;
    const int p1 = min(p0 + EXPAND_PROWS, P);
    // the map row each string sounds at each of this thread's frames; -1: none (silent, or a class outside the map)
    int tgt[AMTX_TAB_MAX_STRINGS][VEC];
#pragma unroll
    for (int s = 0; s < AMTX_TAB_MAX_STRINGS; ++s) {
        if (s < S) {
            const int64_t* src = tab + ((int64_t)b * S + s) * T + t0;
            long long c[VEC];
            if (VEC == 4) {
                const longlong2 lo = reinterpret_cast<const longlong2*>(src)[0], hi = reinterpret_cast<const longlong2*>(src)[1];
                c[0] = lo.x; c[1 % VEC] = lo.y; c[2 % VEC] = hi.x; c[3 % VEC] = hi.y;
            } else {
                c[0] = src[0];
            }
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const long long r = c[j] + start.v[s];
                tgt[s][j] = (c[j] >= 0 && r >= 0 && r < P) ? (int)r : -1;
            }
        } else {
#pragma unroll
            for (int j = 0; j < VEC; ++j) tgt[s][j] = -1;
        }
    }
    for (int p = p0; p < p1; ++p) {
        float any[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) any[j] = 0.f;
#pragma unroll
        for (int s = 0; s < AMTX_TAB_MAX_STRINGS; ++s) {
            if (s < S) {
                float v[VEC];
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    v[j] = tgt[s][j] == p ? 1.f : 0.f;
                    any[j] = fmaxf(any[j], v[j]);
                }
                if (stacked) {
                    float* dst = stacked + (((int64_t)b * S + s) * P + p) * T + t0;
                    if (VEC == 4) *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1 % VEC], v[2 % VEC], v[3 % VEC]);
                    else dst[0] = v[0];
                }
            }
        }
        if (collapsed) {
            float* dst = collapsed + ((int64_t)b * P + p) * T + t0;
            if (VEC == 4) *reinterpret_cast<float4*>(dst) = make_float4(any[0], any[1 % VEC], any[2 % VEC], any[3 % VEC]);
            else dst[0] = any[0];
        }
    }
}

// One wave per (clip, string) row.  WRITE false: counts[row] = notes of the row.  WRITE true: the row's notes, ascending onset, from
// rows[offsets[row]] on (nothing at or past rows_capacity).
template <bool WRITE>
__global__ __launch_bounds__(256) void tab_notes_kernel(const int64_t* __restrict__ tab, int nrows, int S, int T, TabStrings tuning,
                                                        const double* __restrict__ times_ext, int64_t times_stride,
                                                        const int* __restrict__ release, int64_t release_stride, int min_mode, double min_duration,
                                                        int* __restrict__ counts, const int* __restrict__ offsets, double* __restrict__ rows,
                                                        int64_t rows_capacity) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= nrows) return;                               // whole waves leave: the ballots below see all 64 lanes
    const int b = row / S, s = row - b * S;
    const int64_t* cls = tab + (int64_t)row * T;
    const double* tg = times_ext + (int64_t)b * times_stride;
    const int* rel = release ? release + (int64_t)b * release_stride : nullptr;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int64_t base = WRITE ? (int64_t)offsets[row] : 0;
    const int pitch0 = tuning.v[s];
    int run_start = 0;          // frame at which the run reaching into the current chunk began
    int n = 0;                  // notes kept so far
    int open_at = 0;            // lane k: first frame at which class k may start again (inhibition)
    const int nchunks = (T + 63) >> 6;
    for (int ch = 0; ch < nchunks; ++ch) {
        const int t = ch * 64 + lane + 1;                   // the boundary in front of frame t; t == T is the end of the row
        const bool valid = t <= T;
        const long long before = valid ? cls[t - 1] : 0;
        const long long after = (valid && t < T) ? cls[t] : 0;
        const bool bnd = valid && (t == T || after != before);
        const unsigned long long bmask = __ballot(bnd);
        const unsigned long long lower = bmask & below;
        const int onset = lower ? ch * 64 + 64 - __builtin_clzll(lower) : run_start;    // the previous boundary
        const int k = (int)before;
        bool keep = bnd && before >= 0;
        if (rel) {
            unsigned long long m = __ballot(keep);
            while (m) {                                      // the chunk's runs in order; every value below is wave-uniform
                const int l = __builtin_ctzll(m);
                m &= m - 1;
                const int kk = __shfl(k, l), o = __shfl(onset, l);
                if (kk < 64) {
                    const int open = __shfl(open_at, kk);
                    if (o >= open) {
                        const int r = rel[o];
                        if (lane == kk) open_at = r;
                    } else if (lane == l) {
                        keep = false;
                    }
                }
            }
        }
        double t_on = 0.0, t_off = 0.0;
        if (keep) {
            t_on = tg[onset];
            t_off = tg[t];
            if (min_mode) {
                const double d = t_off - t_on;
                keep = min_mode == 2 ? d >= min_duration : d > 0.0;
            }
        }
        const unsigned long long emask = __ballot(keep);
        if (WRITE && keep) {
            const int64_t dst = base + n + __builtin_popcountll(emask & below);
            if (dst < rows_capacity) {
                rows[dst * 3 + 0] = t_on;
                rows[dst * 3 + 1] = t_off;
                rows[dst * 3 + 2] = (double)(pitch0 + k);
            }
        }
        n += __builtin_popcountll(emask);
        if (bmask) run_start = ch * 64 + 64 - __builtin_clzll(bmask);
    }
    if (!WRITE && lane == 0) counts[row] = n;
}

// exclusive scan of counts[0 .. n) into offsets[0 .. n] (one block; 64-bit running sum, offsets clamp at INT32_MAX).  counts may be
// offsets + 1: a 1024-row chunk of counts is in LDS before that chunk's offsets, which sit one element lower, are written.
__global__ __launch_bounds__(1024) void tab_scan_kernel(const int* counts, int n, int* offsets) {
    __shared__ long long part[1024];
    __shared__ long long carry;
    const int tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < n; base += 1024) {
        const int i = base + tid;
        const long long v = i < n ? counts[i] : 0;
        part[tid] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const long long add = tid >= o ? part[tid - o] : 0;
            __syncthreads();
            part[tid] += add;
            __syncthreads();
        }
        const long long excl = carry + part[tid] - v;
        if (i < n) offsets[i] = (int)min(excl, (long long)0x7fffffff);
        __syncthreads();
        if (tid == 1023) carry += part[1023];
        __syncthreads();
    }
    if (tid == 0) offsets[n] = (int)min(carry, (long long)0x7fffffff);
}

}  // namespace

extern "C" int amtx_tab_expand(const int64_t* tablature, int batch, int strings, int num_frames, const int32_t* dof_start, int num_classes,
                               int num_pitches, float* stacked, float* collapsed, void* stream_) {
    AMTX_REQUIRE(tablature && dof_start && (stacked || collapsed), "amtx_tab_expand: null pointer");
    AMTX_REQUIRE(batch > 0 && strings > 0 && num_frames > 0 && num_classes > 0 && num_pitches > 0, "amtx_tab_expand: bad sizes");
    if (strings > AMTX_TAB_MAX_STRINGS) {
        amtx_set_error("amtx_tab_expand: %d strings (up to %d are built)", strings, AMTX_TAB_MAX_STRINGS);
        return AMTX_ERR_UNSUPPORTED;
    }
    TabStrings start;
    for (int s = 0; s < AMTX_TAB_MAX_STRINGS; ++s) start.v[s] = 0;
    for (int s = 0; s < strings; ++s) {
        // every class of the profile must land inside the map: 0 <= dof_start[s] and dof_start[s] + num_classes - 1 < num_pitches
        AMTX_REQUIRE(dof_start[s] >= 0 && (int64_t)dof_start[s] + num_classes - 1 < num_pitches,
                     "amtx_tab_expand: string %d: classes 0..%d from row %d do not fit %d pitch rows", s, num_classes - 1, dof_start[s], num_pitches);
        start.v[s] = dof_start[s];
    }
    hipStream_t stream = (hipStream_t)stream_;
    const bool vec = num_frames % 4 == 0 && ((uintptr_t)tablature | (uintptr_t)stacked | (uintptr_t)collapsed) % 16 == 0;
    const int per_block = 256 * (vec ? 4 : 1);
    const int64_t clip_in = (int64_t)strings * num_frames, clip_col = (int64_t)num_pitches * num_frames, clip_st = clip_col * strings;
    for (int b0 = 0; b0 < batch; b0 += 32768) {             // grid.z
        const int nb = min(batch - b0, 32768);
        const dim3 grid((unsigned)((num_frames + per_block - 1) / per_block), (unsigned)((num_pitches + EXPAND_PROWS - 1) / EXPAND_PROWS), (unsigned)nb);
        const int64_t* tab = tablature + b0 * clip_in;
        float* st = stacked ? stacked + b0 * clip_st : nullptr;
        float* co = collapsed ? collapsed + b0 * clip_col : nullptr;
        if (vec) hipLaunchKernelGGL(tab_expand_kernel<4>, grid, dim3(256), 0, stream, tab, strings, num_frames, num_pitches, start, st, co);
        else hipLaunchKernelGGL(tab_expand_kernel<1>, grid, dim3(256), 0, stream, tab, strings, num_frames, num_pitches, start, st, co);
        AMTX_CHECK_LAUNCH();
    }
    return AMTX_OK;
}

extern "C" int amtx_tab_notes(const int64_t* tablature, int batch, int strings, int num_frames, const int32_t* tuning, int num_classes,
                              const double* times_ext, int64_t times_stride, const int32_t* release, int64_t release_stride,
                              int has_minimum_duration, double minimum_duration, double* rows, int64_t rows_capacity, int32_t* row_offsets,
                              void* stream_) {
    AMTX_REQUIRE(tablature && tuning && times_ext && rows && row_offsets, "amtx_tab_notes: null pointer");
    AMTX_REQUIRE(batch > 0 && strings > 0 && num_frames > 0 && num_classes > 0 && rows_capacity > 0 && times_stride >= 0 && release_stride >= 0,
                 "amtx_tab_notes: bad sizes");
    AMTX_REQUIRE((int64_t)batch * strings < (1ll << 31) - 4 && num_frames < (1 << 30), "amtx_tab_notes: too many rows or frames");
    if (strings > AMTX_TAB_MAX_STRINGS || (release && num_classes > 64)) {
        amtx_set_error("amtx_tab_notes: %d strings, %d classes (up to %d strings, and 64 classes with an inhibition window, are built)", strings,
                       num_classes, AMTX_TAB_MAX_STRINGS);
        return AMTX_ERR_UNSUPPORTED;
    }
    TabStrings tun;
    for (int s = 0; s < AMTX_TAB_MAX_STRINGS; ++s) tun.v[s] = s < strings ? tuning[s] : 0;
    hipStream_t stream = (hipStream_t)stream_;
    const int nrows = batch * strings;
    // threshold 0 keeps notes of non-zero length, any other threshold those at least as long (transcribe.py:70-75)
    const int min_mode = !has_minimum_duration ? 0 : (minimum_duration != 0.0 ? 2 : 1);
    const dim3 grid((unsigned)((nrows + 3) / 4));
    int* counts = row_offsets + 1;                          // see tab_scan_kernel
    hipLaunchKernelGGL(tab_notes_kernel<false>, grid, dim3(256), 0, stream, tablature, nrows, strings, num_frames, tun, times_ext, times_stride,
                       release, release_stride, min_mode, minimum_duration, counts, (const int*)nullptr, (double*)nullptr, (int64_t)0);
    AMTX_CHECK_LAUNCH();
    hipLaunchKernelGGL(tab_scan_kernel, dim3(1), dim3(1024), 0, stream, (const int*)counts, nrows, row_offsets);
    AMTX_CHECK_LAUNCH();
    hipLaunchKernelGGL(tab_notes_kernel<true>, grid, dim3(256), 0, stream, tablature, nrows, strings, num_frames, tun, times_ext, times_stride,
                       release, release_stride, min_mode, minimum_duration, (int*)nullptr, (const int*)row_offsets, rows, rows_capacity);
    AMTX_CHECK_LAUNCH();
    return AMTX_OK;
}
