// Evaluation on the device: what amt_tools/evaluate.py's evaluators need from a clip is a handful of integers, and the maps they are
// counted from are already in device memory when a model has run (evaluate.py:780-903 multi-pitch, :906-1037 notes, :1195-1294
// tablature, :1297-1345 softmax accuracy).  Three entries, none allocates, every output element is written by exactly one thread in a
// fixed order (integer sums: nothing depends on old contents or on arrival order).
//
// amtx_eval_multipitch_counts   est, ref [B][slices][keys][T] fp32 maps of 0 / 1 -> [B][slices][3] int64: cells non-zero in both, in est,
//                   in ref -- the three sums of StackedMultipitchEvaluator.evaluate (num_correct, num_predicted, num_ground_truth).  A
//                   (clip, slice) is keys * T contiguous floats: one block of 256 threads walks it ONCE with 16-byte loads of both maps.
//                   The slice starts wherever (clip * slices + slice) * keys * T floats behind the map's first lands: on the 16-byte grid
//                   when keys * T is a multiple of 4 (88 keys: always) and the map itself starts there, at any 4-byte phase otherwise (an
//                   odd keys * T, a view into a larger buffer): a scalar head up to the first 16-byte boundary, the float4 body, a scalar
//                   tail of (n - head) % 4 cells; maps whose addresses differ modulo 16 take the scalar loop throughout.  HBM-bound: 8
//                   bytes per cell, read once.
//
// amtx_eval_tab_counts   est, ref [B][S][T] int64 tablatures (class -1 = silent) -> [B][5] int64, TablatureEvaluator's and SoftmaxAccuracy's
//                   sums without the 6 x 20 one-hot map and the 44-row collapsed map they are taken from in the reference: a thread owns
//                   a frame, holds the at most 16 pitches per side in registers and counts the distinct pitches of the estimate that the
//                   reference sounds too (S^2 compares).  Lanes along T: 8-byte loads, 512 contiguous bytes per wave and string.
//
// amtx_eval_notes_match   size of a MAXIMUM matching between estimated and reference notes per group (a clip, or a (clip, string)) under
//                   mir_eval.transcription.match_notes' rules for integral pitches, where the graph falls apart by pitch.  One block of
//                   128 threads per group, thread p owns MIDI pitch p: (1) the group's rows are brought into pitch order by a stable
//                   counting sort (every thread walks the group's pitch column -- one broadcast load per row and wave -- counts its own
//                   rows, a 128-entry scan in LDS, then writes their indices): rows of one pitch only have to be in ascending onset order,
//                   which is how amtx_notes_rows (key, onset) and amtx_tab_notes (onset per string) write them; (2) candidates of an
//                   estimated note are the reference notes whose ROUNDED onset distance is within the tolerance, a contiguous window of
//                   the pitch's onset-sorted list, its start found by one forward walk; (3) augmenting paths (Kuhn) over those windows
//                   with the offset rule as an edge filter -- with it the candidates are no longer a contiguous run, so earliest-first
//                   greedy is not maximum.  The DFS is iterative; its stack, the cursors and the match / visit tables live in the
//                   caller's workspace, indexed by row position, so lists are as long as the group.  (4) the 128 sizes are summed with a
//                   wave reduction and one LDS exchange.  Bound: AMTX_EVAL_MATCH_MAX_WINDOW reference notes in one window (it caps the
//                   work of one augmentation at list length x window).
//                   Lists are short (a clip has a handful of notes per pitch), so a list per THREAD keeps all lanes busy where a list
//                   per wave would idle 60 of 64; the divergence between lists of different length is what is left.

#include "amtx_kernels.h"

#define AMTX_TAB_MAX_STRINGS 16

namespace {

static __device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// sums of n values per thread over a block of NW waves -> out[0 .. n) (int64), written by thread 0
template <int N, int NW>
static __device__ __forceinline__ void block_sums_store(unsigned (&v)[N], long long* out) {
    __shared__ unsigned part[NW][N];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const unsigned s = wave_sum_u32(v[k]);
        if (lane == 0) part[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            long long s = 0;
            for (int w = 0; w < NW; ++w) s += part[w][k];       // fixed order
            out[k] = s;
        }
    }
}

__global__ __launch_bounds__(256) void multipitch_counts_kernel(const float* __restrict__ est, const float* __restrict__ ref, int64_t n,
                                                                long long* __restrict__ counts) {
    const int64_t row = blockIdx.x;
    const float* e = est + row * n;
    const float* r = ref + row * n;
    unsigned c[3] = {0u, 0u, 0u};                                // both, est, ref (n < 2^31 cells per slice)
    auto cell = [&](float a, float b) {
        const bool ea = a != 0.f, rb = b != 0.f;
        c[0] += (ea && rb) ? 1u : 0u;
        c[1] += ea ? 1u : 0u;
        c[2] += rb ? 1u : 0u;
    };
    const uintptr_t ae = (uintptr_t)e, ar = (uintptr_t)r;
    const int tid = threadIdx.x;
    if (((ae ^ ar) & 15) == 0) {
        int64_t head = (int64_t)(((16 - (ae & 15)) & 15) >> 2);  // floats in front of the first 16-byte boundary
        if (head > n) head = n;
        const int64_t nvec = (n - head) >> 2;
        if (tid < head) cell(e[tid], r[tid]);
        const float4* e4 = reinterpret_cast<const float4*>(e + head);
        const float4* r4 = reinterpret_cast<const float4*>(r + head);
        for (int64_t i = tid; i < nvec; i += 256) {
            const float4 a = e4[i], b = r4[i];
            cell(a.x, b.x);
            cell(a.y, b.y);
            cell(a.z, b.z);
            cell(a.w, b.w);
        }
        const int64_t tail = head + nvec * 4 + tid;              // at most 3 cells
        if (tail < n) cell(e[tail], r[tail]);
    } else {
        for (int64_t i = tid; i < n; i += 256) cell(e[i], r[i]);
    }
    block_sums_store<3, 4>(c, counts + row * 3);
}

struct TabStrings { int v[AMTX_TAB_MAX_STRINGS]; };

__global__ __launch_bounds__(256) void tab_counts_kernel(const int64_t* __restrict__ est, const int64_t* __restrict__ ref, int S, int T,
                                                         TabStrings tuning, int num_classes, long long* __restrict__ counts) {
    const int64_t b = blockIdx.x;
    const int64_t* e = est + b * S * T;
    const int64_t* r = ref + b * S * T;
    unsigned c[5] = {0u, 0u, 0u, 0u, 0u};
    for (int t = threadIdx.x; t < T; t += 256) {
        int pe[AMTX_TAB_MAX_STRINGS], pr[AMTX_TAB_MAX_STRINGS];   // pitch per string; silent: -1 (estimate), -2 (reference)
#pragma unroll
        for (int s = 0; s < AMTX_TAB_MAX_STRINGS; ++s) {
            pe[s] = -1;
            pr[s] = -2;
            if (s < S) {
                const long long ce = e[(int64_t)s * T + t], cr = r[(int64_t)s * T + t];
                const bool ve = ce >= 0 && ce < num_classes, vr = cr >= 0 && cr < num_classes;   // a stray class reads as silence
                if (ve) pe[s] = tuning.v[s] + (int)ce;
                if (vr) pr[s] = tuning.v[s] + (int)cr;
                c[0] += ve ? 1u : 0u;
                c[1] += vr ? 1u : 0u;
                c[2] += (ve && vr && ce == cr) ? 1u : 0u;
                c[4] += ce == cr ? 1u : 0u;
            }
        }
        // pitches sounding in both collapsed maps: each DISTINCT pitch of the estimate that some string of the reference sounds
#pragma unroll
        for (int i = 0; i < AMTX_TAB_MAX_STRINGS; ++i) {
            bool first = pe[i] >= 0, hit = false;
#pragma unroll
            for (int j = 0; j < AMTX_TAB_MAX_STRINGS; ++j) {
                if (j < i) first = first && pe[j] != pe[i];
                hit = hit || pr[j] == pe[i];
            }
            c[3] += (first && hit) ? 1u : 0u;
        }
    }
    block_sums_store<5, 4>(c, counts + b * 5);
}

// ------------------------------------------------------------------------------------------------------------------------------
// note matching
// ------------------------------------------------------------------------------------------------------------------------------
constexpr int MATCH_PITCHES = 128;

struct MatchRules {
    double onset_tol, offset_ratio, offset_min_tol, scale;       // scale = 10^decimals; offset_ratio < 0: onsets only
};

// numpy.around(x, decimals) for decimals >= 0: rint(x * 10^decimals) / 10^decimals
static __device__ __forceinline__ double around_dec(double x, double scale) {
#pragma clang fp contract(off)
    return rint(x * scale) / scale;
}

static __device__ __forceinline__ bool onset_ok(const double* e, const double* r, const MatchRules& m) {
#pragma clang fp contract(off)
    return around_dec(fabs(r[0] - e[0]), m.scale) <= m.onset_tol;
}

static __device__ __forceinline__ bool offset_ok(const double* e, const double* r, const MatchRules& m) {
#pragma clang fp contract(off)
    if (m.offset_ratio < 0.0) return true;
    const double tol = fmax(m.offset_min_tol, m.offset_ratio * (r[1] - r[0]));
    return around_dec(fabs(r[1] - e[1]), m.scale) <= tol;
}

struct MatchWs {
    int* perm_e; int* lo_e; int* stack_e; int* cur_e;            // [est_rows] each
    int* perm_r; int* match_r; int* seen_r;                      // [ref_rows] each
};

static __device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// stable counting sort of rows [r0, r1) by pitch: thread p leaves the indices of its rows, in order, in perm[start .. start + count) and
// returns count.  A row whose pitch is no integer in [0, 128) belongs to no thread: the counts then sum to less than r1 - r0.
static __device__ __forceinline__ int gather_pitch(const double* __restrict__ rows, int r0, int r1, int p, int* __restrict__ perm, int* scan,
                                                   int* start_out) {
    int n = 0;
    for (int i = r0; i < r1; ++i) n += rows[(int64_t)i * 3 + 2] == (double)p ? 1 : 0;
    __syncthreads();                                             // scan[] may still be read from the previous use
    scan[p] = n;
    __syncthreads();
    int start = r0;
    for (int q = 0; q < p; ++q) start += scan[q];
    int k = start;
    for (int i = r0; i < r1; ++i)
        if (rows[(int64_t)i * 3 + 2] == (double)p) perm[k++] = i;
    *start_out = start;
    return n;
}

__global__ __launch_bounds__(MATCH_PITCHES) void notes_match_kernel(const double* __restrict__ est, const int* __restrict__ est_offsets, int est_rows,
                                                                    const double* __restrict__ ref, const int* __restrict__ ref_offsets, int ref_rows,
                                                                    MatchRules m, int max_window, MatchWs ws, int* __restrict__ matched) {
    __shared__ int scan[MATCH_PITCHES];
    __shared__ int part[MATCH_PITCHES / 64][3];
    const int g = blockIdx.x, p = threadIdx.x;
    // offsets come from device memory (a decoder wrote them, and its total may exceed the buffer): nothing outside the arrays is touched.
    // They are non-decreasing by contract: the clamp keeps overlapping groups inside the arrays, not off each other's workspace rows
    const int e0 = clampi(est_offsets[g], 0, est_rows), e1 = clampi(est_offsets[g + 1], e0, est_rows);
    const int r0 = clampi(ref_offsets[g], 0, ref_rows), r1 = clampi(ref_offsets[g + 1], r0, ref_rows);
    int pe0, pr0;
    const int ne = gather_pitch(est, e0, e1, p, ws.perm_e, scan, &pe0);
    const int nr = gather_pitch(ref, r0, r1, p, ws.perm_r, scan, &pr0);
    const int pe1 = pe0 + ne, pr1 = pr0 + nr;
    int size = 0, beyond = 0;
    if (ne > 0 && nr > 0) {
        for (int j = pr0; j < pr1; ++j) {
            ws.match_r[j] = -1;
            ws.seen_r[j] = 0;
        }
        // windows: est and ref onsets ascend within the pitch, so the first candidate never moves back
        int ptr = pr0;
        for (int i = pe0; i < pe1; ++i) {
            const double* e = est + (int64_t)ws.perm_e[i] * 3;
            while (ptr < pr1) {
                const double* r = ref + (int64_t)ws.perm_r[ptr] * 3;
                if (onset_ok(e, r, m) || r[0] >= e[0]) break;
                ++ptr;
            }
            ws.lo_e[i] = ptr;
            int k = ptr;
            while (k < pr1 && onset_ok(e, ref + (int64_t)ws.perm_r[k] * 3, m)) ++k;
            if (k - ptr > max_window) beyond = 1;
        }
        if (!beyond) {
            for (int a = pe0; a < pe1; ++a) {
                const int stamp = a - pe0 + 1;
                int depth = 0;
                ws.stack_e[pe0] = a;
                ws.cur_e[a] = ws.lo_e[a];
                while (depth >= 0) {
                    const int u = ws.stack_e[pe0 + depth];
                    const double* e = est + (int64_t)ws.perm_e[u] * 3;
                    bool moved = false;
                    while (ws.cur_e[u] < pr1) {
                        const int j = ws.cur_e[u];
                        const double* r = ref + (int64_t)ws.perm_r[j] * 3;
                        if (!onset_ok(e, r, m)) {
                            ws.cur_e[u] = pr1;                   // the window ends here
                            break;
                        }
                        ws.cur_e[u] = j + 1;
                        if (ws.seen_r[j] == stamp || !offset_ok(e, r, m)) continue;
                        ws.seen_r[j] = stamp;
                        const int v = ws.match_r[j];
                        if (v < 0) {
                            // free: every note on the stack takes the reference note it went down through (its cursor - 1)
                            for (int d = depth; d >= 0; --d) {
                                const int w = ws.stack_e[pe0 + d];
                                ws.match_r[ws.cur_e[w] - 1] = w;
                            }
                            ++size;
                            depth = -2;                          // done with this root
                        } else {
                            ++depth;                             // depth < ne: a path holds every estimated note at most once
                            ws.stack_e[pe0 + depth] = v;
                            ws.cur_e[v] = ws.lo_e[v];
                        }
                        moved = true;
                        break;
                    }
                    if (!moved) --depth;
                }
            }
        }
    }
    // group result: the sum of the 128 sizes; the number of rows no thread owns (pitch no integer in [0, 128)); any window beyond the bound
    unsigned owned = wave_sum_u32((unsigned)(ne + nr)), total = wave_sum_u32((unsigned)size), far = wave_sum_u32((unsigned)beyond);
    if ((p & 63) == 0) {
        part[p >> 6][0] = (int)owned;
        part[p >> 6][1] = (int)total;
        part[p >> 6][2] = (int)far;
    }
    __syncthreads();
    if (p == 0) {
        int o = 0, t = 0, f = 0;
        for (int w = 0; w < MATCH_PITCHES / 64; ++w) {
            o += part[w][0];
            t += part[w][1];
            f += part[w][2];
        }
        matched[g] = o != (e1 - e0) + (r1 - r0) ? AMTX_ERR_ARG : (f ? AMTX_ERR_UNSUPPORTED : t);
    }
}

// status[0] = AMTX_ERR_ARG if any group answered it, else AMTX_ERR_UNSUPPORTED if any did, else AMTX_OK
__global__ __launch_bounds__(256) void match_status_kernel(const int* __restrict__ matched, int groups, int* __restrict__ status) {
    __shared__ int part[4][2];
    unsigned arg = 0, uns = 0;
    for (int g = threadIdx.x; g < groups; g += 256) {
        const int v = matched[g];
        arg |= v == AMTX_ERR_ARG ? 1u : 0u;
        uns |= v == AMTX_ERR_UNSUPPORTED ? 1u : 0u;
    }
    arg = wave_sum_u32(arg);
    uns = wave_sum_u32(uns);
    if ((threadIdx.x & 63) == 0) {
        part[threadIdx.x >> 6][0] = (int)arg;
        part[threadIdx.x >> 6][1] = (int)uns;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int a = 0, u = 0;
        for (int w = 0; w < 4; ++w) {
            a += part[w][0];
            u += part[w][1];
        }
        status[0] = a ? AMTX_ERR_ARG : (u ? AMTX_ERR_UNSUPPORTED : AMTX_OK);
    }
}

constexpr size_t MATCH_WS_ALIGN = 256;
static size_t match_ws_bytes(int64_t est_rows, int64_t ref_rows) {
    const size_t ints = (size_t)(4 * est_rows + 3 * ref_rows);
    return (ints * sizeof(int) + MATCH_WS_ALIGN - 1) / MATCH_WS_ALIGN * MATCH_WS_ALIGN + MATCH_WS_ALIGN;
}

}  // namespace

extern "C" int amtx_eval_multipitch_counts(const float* est, const float* ref, int batch, int slices, int keys, int num_frames, int64_t* counts,
                                           void* stream_) {
    AMTX_REQUIRE(est && ref && counts, "amtx_eval_multipitch_counts: null pointer");
    AMTX_REQUIRE(batch > 0 && slices > 0 && keys > 0 && num_frames > 0, "amtx_eval_multipitch_counts: bad sizes");
    AMTX_REQUIRE(((uintptr_t)est | (uintptr_t)ref) % 4 == 0 && (uintptr_t)counts % 8 == 0, "amtx_eval_multipitch_counts: misaligned pointer");
    AMTX_REQUIRE((int64_t)keys * num_frames < (1ll << 31) && (int64_t)batch * slices < (1ll << 31),
                 "amtx_eval_multipitch_counts: %d x %d cells per slice, %d x %d slices: too many", keys, num_frames, batch, slices);
    hipLaunchKernelGGL(multipitch_counts_kernel, dim3((unsigned)(batch * slices)), dim3(256), 0, (hipStream_t)stream_, est, ref,
                       (int64_t)keys * num_frames, (long long*)counts);
    AMTX_CHECK_LAUNCH();
    return AMTX_OK;
}

extern "C" int amtx_eval_tab_counts(const int64_t* est, const int64_t* ref, int batch, int strings, int num_frames, const int32_t* tuning,
                                    int num_classes, int64_t* counts, void* stream_) {
    AMTX_REQUIRE(est && ref && tuning && counts, "amtx_eval_tab_counts: null pointer");
    AMTX_REQUIRE(batch > 0 && strings > 0 && num_frames > 0 && num_classes > 0, "amtx_eval_tab_counts: bad sizes");
    AMTX_REQUIRE(((uintptr_t)est | (uintptr_t)ref | (uintptr_t)counts) % 8 == 0, "amtx_eval_tab_counts: misaligned pointer");
    if (strings > AMTX_TAB_MAX_STRINGS) {
        amtx_set_error("amtx_eval_tab_counts: %d strings (up to %d are built)", strings, AMTX_TAB_MAX_STRINGS);
        return AMTX_ERR_UNSUPPORTED;
    }
    AMTX_REQUIRE((int64_t)strings * num_frames < (1ll << 31), "amtx_eval_tab_counts: %d x %d cells per clip: too many", strings, num_frames);
    TabStrings tun;
    for (int s = 0; s < AMTX_TAB_MAX_STRINGS; ++s) tun.v[s] = 0;
    for (int s = 0; s < strings; ++s) {
        // a pitch is an int, and silence is a negative one
        AMTX_REQUIRE(tuning[s] >= 0 && (int64_t)tuning[s] + num_classes < (1ll << 30), "amtx_eval_tab_counts: string %d: tuning %d with %d classes", s,
                     tuning[s], num_classes);
        tun.v[s] = tuning[s];
    }
    hipLaunchKernelGGL(tab_counts_kernel, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream_, est, ref, strings, num_frames, tun, num_classes,
                       (long long*)counts);
    AMTX_CHECK_LAUNCH();
    return AMTX_OK;
}

extern "C" size_t amtx_eval_notes_match_workspace_bytes(int64_t est_rows, int64_t ref_rows) {
    if (est_rows < 0 || ref_rows < 0) return 0;
    return match_ws_bytes(est_rows, ref_rows);
}

extern "C" int amtx_eval_notes_match(const double* est, const int32_t* est_offsets, int64_t est_rows, const double* ref, const int32_t* ref_offsets,
                                     int64_t ref_rows, int groups, double onset_tolerance, double offset_ratio, double offset_min_tolerance,
                                     int decimals, void* workspace, size_t workspace_bytes, int32_t* matched, int32_t* status, int wait,
                                     void* stream_) {
    AMTX_REQUIRE(est && est_offsets && ref && ref_offsets && workspace && matched && status, "amtx_eval_notes_match: null pointer");
    AMTX_REQUIRE(groups > 0 && est_rows > 0 && ref_rows > 0, "amtx_eval_notes_match: bad sizes");
    AMTX_REQUIRE(est_rows < (1ll << 31) / 3 && ref_rows < (1ll << 31) / 3, "amtx_eval_notes_match: too many rows");
    AMTX_REQUIRE(((uintptr_t)est | (uintptr_t)ref) % 8 == 0 && ((uintptr_t)est_offsets | (uintptr_t)ref_offsets | (uintptr_t)matched | (uintptr_t)status) % 4 == 0 &&
                     (uintptr_t)workspace % MATCH_WS_ALIGN == 0,
                 "amtx_eval_notes_match: misaligned pointer");
    AMTX_REQUIRE(onset_tolerance >= 0.0 && (offset_ratio < 0.0 || offset_min_tolerance >= 0.0) && decimals >= 0 && decimals <= 15,
                 "amtx_eval_notes_match: bad rules (onset tolerance %g, offset ratio %g, minimum offset tolerance %g, %d decimals)", onset_tolerance,
                 offset_ratio, offset_min_tolerance, decimals);
    AMTX_REQUIRE(workspace_bytes >= match_ws_bytes(est_rows, ref_rows), "amtx_eval_notes_match: workspace of %zu bytes, %zu needed", workspace_bytes,
                 match_ws_bytes(est_rows, ref_rows));
    MatchRules m;
    m.onset_tol = onset_tolerance;
    m.offset_ratio = offset_ratio;
    m.offset_min_tol = offset_min_tolerance;
    m.scale = 1.0;
    for (int d = 0; d < decimals; ++d) m.scale *= 10.0;          // exact up to 10^22
    MatchWs ws;
    int* w = (int*)workspace;
    ws.perm_e = w;
    ws.lo_e = ws.perm_e + est_rows;
    ws.stack_e = ws.lo_e + est_rows;
    ws.cur_e = ws.stack_e + est_rows;
    ws.perm_r = ws.cur_e + est_rows;
    ws.match_r = ws.perm_r + ref_rows;
    ws.seen_r = ws.match_r + ref_rows;
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(notes_match_kernel, dim3((unsigned)groups), dim3(MATCH_PITCHES), 0, stream, est, (const int*)est_offsets, (int)est_rows, ref,
                       (const int*)ref_offsets, (int)ref_rows, m, (int)AMTX_EVAL_MATCH_MAX_WINDOW, ws, (int*)matched);
    AMTX_CHECK_LAUNCH();
    hipLaunchKernelGGL(match_status_kernel, dim3(1), dim3(256), 0, stream, (const int*)matched, groups, (int*)status);
    AMTX_CHECK_LAUNCH();
    if (!wait) return AMTX_OK;
    int32_t st = AMTX_OK;
    AMTX_CHECK_HIP(hipMemcpyAsync(&st, status, sizeof(st), hipMemcpyDeviceToHost, stream));
    // wait for THIS stream only, through an event: the caller's other streams (its copy and side streams) run on
    hipEvent_t copied;
    AMTX_CHECK_HIP(hipEventCreate(&copied));
    hipError_t err = hipEventRecord(copied, stream);
    if (err == hipSuccess) err = hipEventSynchronize(copied);
    (void)hipEventDestroy(copied);
    AMTX_CHECK_HIP(err);
    if (st == AMTX_ERR_ARG) amtx_set_error("amtx_eval_notes_match: a note's pitch is no integer in [0, %d)", MATCH_PITCHES);
    if (st == AMTX_ERR_UNSUPPORTED)
        amtx_set_error("amtx_eval_notes_match: more than %d reference notes of one pitch within the onset tolerance of one estimated note",
                       (int)AMTX_EVAL_MATCH_MAX_WINDOW);
    return st == AMTX_OK || st == AMTX_ERR_ARG || st == AMTX_ERR_UNSUPPORTED ? st : AMTX_ERR_HIP;
}
