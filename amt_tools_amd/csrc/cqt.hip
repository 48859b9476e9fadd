// Constant-Q / Variable-Q / Harmonic CQT front-end for gfx950.
//
// Replaces librosa.vqt as called from amt_tools/features/vqt.py:183-193 (CQT: cqt.py:22; HVQT/HCQT: one VQT per
// harmonic, hvqt.py:45-58,107-133) plus abs -> amplitude_to_db(ref=max) -> /80+1 (features/common.py:199,218-228).
//
// librosa evaluates, per octave, a sparse FFT-domain wavelet basis against a "ones"-window STFT of the
// progressively 2x-decimated signal.  Here the same linear map is applied in the time domain: for every bank
// (harmonic, octave) the sparsified one-sided FFT basis is folded back on the host (fp64) into its equivalent
// n_fft-tap complex kernel, all banks that live on the same decimation level are stacked into one matrix, and the
// response of a level is ONE strided-row GEMM on the matrix cores
//        R_d[t, :] = W_d . y_d[t*hop_d - n_fft/2 : t*hop_d + n_fft/2]          (A rows overlap: lda = hop_d)
// in split-bf16 "x3" arithmetic (fp32-class accuracy: a bf16-only product would leak a strong partial into bins
// 50 dB below it).  Harmonics that are octaves apart share the pyramid level and the launch.
// The pyramid itself is a 301-tap Kaiser half-band decimator (the project's documented stand-in for soxr, which
// is not bit-reproducible anyway), then |.|, per-(clip, harmonic) max, dB, /80+1.

#include "amtx_kernels.h"
#include "../../include/amtx_pyramid.h"

#include <cstdlib>

#include <algorithm>
#include <cmath>
#include <complex>
#include <vector>

namespace {

constexpr double DEC_CUTOFF = 0.239;
constexpr double DEC_BETA = 10.0;
constexpr int MAX_BANKS = 16;          // banks per pyramid level
constexpr double PI = 3.14159265358979323846;
constexpr double HANN_BW = 1.50018310546875;

struct BankDev { int col0, nf, harm, bin0, frames; };
struct LevelDev { int nbanks; int ncols; BankDev b[MAX_BANKS]; };


double bessel_i0(double x) {
    double s = 1.0, t = 1.0;
    for (int k = 1; k < 200; ++k) {
        t *= (x / (2.0 * k)) * (x / (2.0 * k));
        s += t;
        if (t < 1e-18 * s) break;
    }
    return s;
}

// ---------------------------------------------------------------- kernels
// maximum over the 16 lanes of a DPP row, in every lane of it
__device__ __forceinline__ float row_max_f32(float v) {
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xf, 0xf, false)));    // quad_perm [1,0,3,2]
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xf, 0xf, false)));    // quad_perm [2,3,0,1]
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xf, 0xf, false)));   // row_half_mirror
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xf, 0xf, false)));   // row_mirror
    return v;
}

// a wave-uniform value the compiler cannot prove uniform (loaded through a table pointer), into scalar registers
__device__ __forceinline__ int64_t uniform_i64(int64_t v) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// re^2 + im^2 as two rounded squares and their rounded sum (no fma)
__device__ __forceinline__ float power_unfused(float re, float im) {
#pragma clang fp contract(off)
    return re * re + im * im;
}

// level 0 of the pyramid: the clip copied between its centre paddings.  `zero_pads`: the paddings are written here too (zeros, librosa
// >= 0.10; the reflecting pad of 0.9 keeps its own kernel); the per-(clip, harmonic) maxima the basis products accumulate are reset.
__global__ __launch_bounds__(256) void cqt_level0_kernel(const float* __restrict__ audio, int64_t n, int64_t astride, float* __restrict__ pyr,
                                                         int64_t pstride, int pad, int zero_pads, float* __restrict__ maxbuf, int n_harm) {
    const int b = blockIdx.y;
    const float* src = audio + (int64_t)b * astride;
    float* row = pyr + (int64_t)b * pstride;
    if (blockIdx.x == 0 && (int)threadIdx.x < n_harm) maxbuf[b * n_harm + threadIdx.x] = 0.f;
    if (zero_pads) {
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < pstride; i += (int64_t)gridDim.x * 256)
            row[i] = (i >= pad && i < pad + n) ? src[i - pad] : 0.f;
    } else {
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) row[pad + i] = src[i];
    }
}

// centre padding of one pyramid level: zeros (librosa >= 0.10) or reflection (librosa 0.9)
__global__ __launch_bounds__(256) void cqt_pad_kernel(float* __restrict__ pyr, int64_t n, int64_t stride, int pad, int reflect) {
    const int b = blockIdx.y;
    float* row = pyr + (int64_t)b * stride;
    const int64_t tail = stride - pad - n;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < pad + tail; i += (int64_t)gridDim.x * 256) {
        if (i < pad) {                                      // left pad, position pad-1-i  <->  sample index i+1
            float v = 0.f;
            if (reflect && i + 1 < n) v = row[pad + i + 1];
            row[pad - 1 - i] = v;
        } else {                                            // right region, position pad+n+j  <->  sample n-2-j
            const int64_t j = i - pad;
            float v = 0.f;
            if (reflect && j < pad && n - 2 - j >= 0) v = row[pad + n - 2 - j];
            row[pad + n + j] = v;
        }
    }
}

// amplitude_to_db(ref = max) -> clamp -80 -> /80 + 1 (or plain magnitude), truncated to t_out frames; from the POWER map
__global__ __launch_bounds__(256) void cqt_scale_kernel(const float* __restrict__ mag, const float* __restrict__ maxbuf, int n_bins, int64_t t_buf,
                                                        int64_t t_out, int decibels, float* __restrict__ out) {
    // no contraction: with 10 log10(a) - offs fused into one fma, the bin that IS the maximum came out as the rounding residue of offs instead
    // of 0 dB -- 1 - 2^-24 on the scaled map wherever 10 log10(max power) <= -64 dB (quiet clips), where the reference has exactly 1.0
#pragma clang fp contract(off)
    const int bh = blockIdx.y;
    const float ref = maxbuf[bh];                            // `mag` and `maxbuf` hold POWERS (re^2 + im^2 as the basis products' epilogue leaves them:
                                                             // no root there, no square here)
    const float amin2 = 1e-10f;                              // amin = 1e-5 on magnitude
    const float offs = 10.0f * log10f(fmaxf(amin2, ref));
    const float floor_db = (10.0f * log10f(fmaxf(amin2, ref)) - offs) - 80.0f;
    const int64_t total = (int64_t)n_bins * t_out;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int k = (int)(i / t_out);
        const int64_t t = i - (int64_t)k * t_out;
        const float a = mag[((int64_t)bh * n_bins + k) * t_buf + t];
        float v;
        if (decibels) {
            float db = 10.0f * log10f(fmaxf(amin2, a)) - offs;
            db = fmaxf(db, floor_db);
            v = db / 80.0f + 1.0f;
        } else {
            v = sqrtf(a);
        }
        out[((int64_t)bh * n_bins + k) * t_out + t] = v;
    }
}

// The same scaling written the way the engine's fused first conv stages its features (convg.hip, tap-major: ConvArgs.feats16):
// out16[b][t][bin][8] bf16, the harmonics of a (frame, bin) position side by side in one 16-byte slot (slots n_harm .. 7 zero) -- that kernel
// then fetches a position with one 16-byte load instead of n_harm strided fp32 loads, conversions and 2-byte LDS stores (29 % of its tile),
// and the map is written once in 4 bytes less per value.  The values are the fp32 ones of cqt_scale_kernel rounded to bf16 by the conversion
// the conv kernel applies itself: the same bits reach the matrix cores.  A block transposes 32 frames x (a chunk of) the bins of one clip
// through LDS: reads run along t (mag's inner axis), writes along (t, bin).
constexpr int SC16_TT = 32;
constexpr int SC16_U = 9;          // 72 bins = one round of 8 rows x 9
__global__ __launch_bounds__(256) void cqt_scale16_kernel(const float* __restrict__ mag, const float* __restrict__ maxbuf, int n_harm, int n_bins, int nbc,
                                                          int64_t t_buf, int64_t t_out, int decibels, uint4* __restrict__ out16, int64_t lo_plane) {
#pragma clang fp contract(off)                               // like cqt_scale_kernel: the same bits, and a map's maximum is exactly 1.0
    // lo_plane != 0 (amtx_cqt_forward16_split, the x3 engine's hand-over): a second map, lo = 16-bit(v - 16-bit(v)), lo_plane 16-byte slots
    // behind the first -- the two planes split_bf16x2 makes of the fp32 feature, i.e. what the two-plane conv kernels made of it themselves
    extern __shared__ __attribute__((aligned(16))) char smem[];          // [planes][SC16_TT][nbc + 1] slots of 16 bytes, then 8 x 2 floats
    const int tid = threadIdx.x, b = blockIdx.y;
    const int64_t t0 = (int64_t)blockIdx.x * SC16_TT;
    const int rs = nbc + 1;                                   // slots per frame row (+ 1: rows start 4 banks apart)
    const int npl = lo_plane ? 2 : 1;
    uint4* tile = reinterpret_cast<uint4*>(smem);
    uint4* tile_lo = tile + SC16_TT * rs;
    float* refs = reinterpret_cast<float*>(smem + (size_t)npl * SC16_TT * rs * 16);
    const float amin2 = 1e-10f;                              // amin = 1e-5 on magnitude
    if (tid < n_harm) {
        const float ref = maxbuf[b * n_harm + tid];            // a power, like `mag` (cqt_scale_kernel)
        const float offs = 10.0f * log10f(fmaxf(amin2, ref));
        refs[2 * tid] = offs;
        refs[2 * tid + 1] = (10.0f * log10f(fmaxf(amin2, ref)) - offs) - 80.0f;
    }
    for (int i = tid; i < npl * SC16_TT * rs; i += 256) tile[i] = make_uint4(0, 0, 0, 0);
    const int tt = tid & 31, r = tid >> 5;
    const bool t_ok = t0 + tt < t_out;
    for (int bin0 = 0; bin0 < n_bins; bin0 += nbc) {
        const int nb = min(nbc, n_bins - bin0);
        __syncthreads();                                      // tile zeroed / written out; refs visible
        // SC16_U loads in flight per thread before the first is used (one at a time -- load, log, store -- a block spent its life waiting:
        // 0.54 ms for the kernel instead of the 0.27 ms of cqt_scale_kernel)
        for (int h = 0; h < n_harm; ++h) {
            const float* row = mag + ((int64_t)(b * n_harm + h) * n_bins + bin0) * t_buf + t0 + tt;
            const float offs = refs[2 * h], floor_db = refs[2 * h + 1];
            for (int k0 = r; k0 < nb; k0 += 8 * SC16_U) {
                float a[SC16_U];
#pragma unroll
                for (int u = 0; u < SC16_U; ++u) a[u] = t_ok ? row[(int64_t)min(k0 + 8 * u, nb - 1) * t_buf] : 0.f;
#pragma unroll
                for (int u = 0; u < SC16_U; ++u) {
                    const int k = k0 + 8 * u;
                    float v;
                    if (decibels) {
                        float db = 10.0f * log10f(fmaxf(amin2, a[u])) - offs;
                        db = fmaxf(db, floor_db);
                        v = db / 80.0f + 1.0f;
                    } else {
                        v = sqrtf(a[u]);
                    }
                    if (k < nb) {
                        uint32_t hi, lo;
                        split_bf16x2(v, 0.f, hi, lo);         // hi = the rounding pack_bf16x2 applies
                        reinterpret_cast<unsigned short*>(tile + tt * rs + k)[h] = (unsigned short)hi;
                        if (lo_plane) reinterpret_cast<unsigned short*>(tile_lo + tt * rs + k)[h] = (unsigned short)lo;
                    }
                }
            }
        }
        __syncthreads();
        for (int i = tid; i < SC16_TT * nb; i += 256) {
            const int ti = i / nb, k = i - ti * nb;
            if (t0 + ti < t_out) {
                const int64_t o = ((int64_t)b * t_out + t0 + ti) * n_bins + bin0 + k;
                out16[o] = tile[ti * rs + k];
                if (lo_plane) out16[lo_plane + o] = tile_lo[ti * rs + k];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// The basis products of every pyramid level, one launch (round 5; until then amtx_launch_gemm_multi ran them on the generic fp32-A
// two-plane GEMM).  A row of a level's product is a WINDOW of its signal: row t = y[t hop - K / 2 .. t hop + K / 2), K = n_fft = 128 / 256,
// hop = 512 .. 4 -- consecutive rows overlap by K - hop samples, up to 63 / 64 of a row.  The generic GEMM loaded and converted (fp32 ->
// hi / lo planes, ~3 vector instructions per value) every row on its own: each sample of a deep level up to 64 times.  Here a block
// stages the signal of FT consecutive frames of one clip ONCE (coalesced fp32 loads, one split per sample, two 16-bit planes in LDS) and
// every row's MFMA operand is a 16-byte window of that copy; the level's basis (<= 256 columns x K, two planes) sits in the waves'
// registers for the whole launch.  Frames run down the lanes (lane & 15), so a frame's window starts hop samples after its neighbour's:
// the copy is stored with 16 pad samples behind every hop samples (hop >= 32) -- a frame stride of 2 (mod 4) 16-byte slots, see bas_pad --
// which makes every ds_read_b128 lane group conflict-free; hop = 16 and 8 need none, hop = 4 reads two 8-byte halves.
// Same planes, same product order (hi.hi, hi.lo, lo.hi per 32-deep step, k ascending) and the same epilogue (|re + i im|^2 transposed into
// mag[b][harmonic][bin][t], per-(clip, harmonic) maxima) as gemm_tile: the same bits.
#ifdef AMTX_CQT_TIMING
// debug build only (tools/build_dbg.sh cqtbasis cqt.hip -DAMTX_CQT_TIMING; tools/cqt_basis_prof.py): cycles wave 0 of every block of
// cqt_basis_kernel spends per phase: [0] tile setup, [1] staging (loads, split, LDS stores), [2] barrier, [3] matrix loop + magnitude stores,
// [4] maxima + barrier + global atomics, [7] tiles
__device__ unsigned long long g_bas_prof[8];
#define BQ_TICK(SLOT) do { const unsigned long long now_ = __builtin_readcyclecounter(); bq_acc[SLOT] += now_ - bq_t; bq_t = now_; } while (0)
extern "C" int amtxdbg_bas_prof(unsigned long long* out8, int reset) {
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_bas_prof), 8 * sizeof(unsigned long long)) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[8] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_bas_prof), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#else
#define BQ_TICK(SLOT) do {} while (0)
#endif
// pad samples behind every `hop` samples of the staged copy: the frame stride must be 2 (mod 4) 16-byte slots for the operand reads to be
// conflict-free -- ds_read_b128 serves lanes {0-3, 12-15} of one k-group together with lanes {4-11} of the NEXT (one slot further), so an odd
// stride (the 8 samples of the first version: 9, 5, 3 slots) put seven of every eight of them on a slot twice: 48 % of the kernel's LDS
// cycles were conflicts, and its operand reads as many cycles as its matrix instructions (tools/lds_swizzle_check_basis.py)
__host__ __device__ constexpr int bas_pad(int hop) { return hop >= 32 ? 16 : 0; }
constexpr int BAS_MAXLEV = 10;
constexpr int BAS_AHEAD = 1;            // k-steps the operand reads of cqt_basis_kernel run ahead
constexpr int BAS_MAXWIN = 16384;         // samples of a tile's window at most (66 KB of LDS with the pads: two blocks per CU)
struct BasisLevel {
    const float* sig; int64_t sig_gs;      // level signal of clip 0 (sample 0 = first sample of the clip at this level), elements per clip
    int64_t len;                           // samples that exist: indices [0, len) of `sig`; everything else reads as zero
    int off;                               // index of the level's sample 0 in `sig` (librosa 0.9: the reflecting pad in front of it exists)
    const bf16_t* w; const int2* map;      // packed basis [2][n_pad][k_pad], pair map
    int n_pad, k_pad, ncols, hop, frames, ft, tiles_per_clip;
    int tile0;                             // first tile id of this level in the launch
};
struct BasisArgs {
    BasisLevel lev[BAS_MAXLEV];
    int nlev, ntiles, B;
    float* mag; int64_t mag_gs, mag_pitch; // mag[b * mag_gs + row * mag_pitch + t]
    float* maxbuf; int n_harm;
    int rows[16];                          // frames of harmonic h
};

struct BasisLevs { int n; int lev[BAS_MAXLEV]; int b0[BAS_MAXLEV + 1]; };   // levels of a launch; blocks [b0[i], b0[i + 1]) work on level lev[i]

// The clip form (include/amtx_pyramid.h): a tile belongs to a clip DESCRIPTOR instead of a batch index.  Clip b is frames
// [first, first + frames) of one track of a bank whose level signals are resident; BasisLevel.sig is then the level's buffer (the audio, or the
// pyramid behind its left pad) and the track's own base and length come from its row of the track table.  BasisArgs.B / mag / mag_pitch
// describe the clip-sized maps [B][n_harm][n_bins][num_frames]; BasisLevel.frames = num_frames, sig_gs / len and BasisArgs.rows are unused.
struct BasisClips {
    const int64_t* tab;                    // [tracks][cols]: the track table of include/amtx_pyramid.h
    const int64_t* desc;                   // [B][3] = {track, first_frame, frames}; null: clip b = track b, whole (the maxima launch)
    int cols, rows_col, num_frames;
    int base_col[BAS_MAXLEV], len_col[BAS_MAXLEV];   // per level: the table columns of the track's first element in BasisLevel.sig and of its length
};

// grid: (blocks of all levels of this K, column slices of 128): all levels of a call run side by side, the small deep ones under the large
// shallow ones.  256-thread blocks, two per CU: a wave keeps the basis of ITS two column tiles in registers and walks the tile's frames on
// its own (a dependent read -> MFMA chain per 16 frames), so what fills the matrix pipe is the other waves of the CU; a level with more than
// 128 columns (HCQT's middle levels stack 144) runs a second slice of blocks for the rest, which stages the same signal again (an L2 hit).
#define CQT_BASIS_CLIPS 0
#include "cqt_basis_kernel.h"            // cqt_basis_kernel<KS>: equal clips side by side in a batch
#undef CQT_BASIS_CLIPS
#define CQT_BASIS_CLIPS 1
#include "cqt_basis_kernel.h"            // cqt_basis_clips_kernel<KS>: clips cut from resident pyramids
#undef CQT_BASIS_CLIPS

struct Level {
    int nfft = 0, ncols = 0, hop = 0;
    std::vector<BankDev> banks;
    std::vector<float> W;          // [ncols][nfft] fp32 row-major (built incrementally per bank at bank nfft, re-centred later)
    std::vector<std::pair<int, std::vector<std::complex<double>>>> raw;   // (bank nfft, kernels nf x nfft)
    bf16_t* d_w = nullptr;
    int2* d_map = nullptr;          // per output pair (filter): {row of the (harmonic, bin) in the magnitude map, harmonic}
    int n_pad = 0, k_pad = 0;
};

}  // namespace

struct amtx_cqt_plan {
    int sr, hop, n_bins, bpo, n_harm, lib09, truncate;
    double fmin, gamma, alpha;
    std::vector<double> harmonics;
    std::vector<int> early;           // early-downsample count per harmonic
    std::vector<Level> levels;
    int pad = 0;                      // centre padding of every pyramid level (max n_fft / 2)
    void* d_tfrag = nullptr;                       // Toeplitz fragments of the decimator for cqt_decimate_mfma_kernel
};

namespace {

double alpha_of(int bpo, int lib09) {
    const double r = std::pow(2.0, 1.0 / bpo);
    return lib09 ? (r - 1.0) : (r * r - 1.0) / (r * r + 1.0);
}

int num_two_factors(int x) {
    int n = 0;
    while (x > 0 && x % 2 == 0) { ++n; x /= 2; }
    return n;
}

int early_count(double nyquist, double cutoff, int hop, int n_oct) {
    const int c1 = std::max(0, (int)std::ceil(std::log2(nyquist / cutoff)) - 1 - 1);
    const int c2 = std::max(0, num_two_factors(hop) - n_oct + 1);
    return std::min(c1, c2);
}

// time-domain equivalent of librosa's sparsified one-sided FFT basis of one octave (see header comment)
void build_bank(const std::vector<double>& freqs, double sr_i, double sr_base, double gamma, double alpha,
                const std::vector<double>& len_base, int& nfft, std::vector<std::complex<double>>& kern) {
    const int nf = (int)freqs.size();
    const double Q = 1.0 / alpha;
    std::vector<double> ilen(nf);
    double maxlen = 0;
    for (int k = 0; k < nf; ++k) { ilen[k] = Q * sr_i / (freqs[k] + gamma / alpha); maxlen = std::max(maxlen, ilen[k]); }
    nfft = (int)std::llround(std::pow(2.0, std::ceil(std::log2(maxlen))));
    kern.assign((size_t)nf * nfft, 0.0);
    const int nb = nfft / 2 + 1;
    std::vector<std::complex<double>> tw(nfft);
    for (int i = 0; i < nfft; ++i) tw[i] = std::polar(1.0, -2.0 * PI * i / nfft);
    std::vector<std::complex<double>> basis(nfft), spec(nb);
    std::vector<double> mags(nb), sorted(nb);
    for (int k = 0; k < nf; ++k) {
        const long n0 = (long)std::floor(-ilen[k] / 2.0), n1 = (long)std::floor(ilen[k] / 2.0);
        const int cnt = (int)(n1 - n0);
        std::fill(basis.begin(), basis.end(), 0.0);
        const int lpad = (nfft - cnt) / 2;
        double l1 = 0;
        for (int n = 0; n < cnt; ++n) l1 += 0.5 - 0.5 * std::cos(2.0 * PI * n / cnt);
        for (int n = 0; n < cnt; ++n) {
            const double w = (0.5 - 0.5 * std::cos(2.0 * PI * n / cnt)) / l1;
            basis[lpad + n] = std::polar(w, 2.0 * PI * freqs[k] * (double)(n0 + n) / sr_i) * (ilen[k] / nfft);
        }
        double norm = 0;
        for (int f = 0; f < nb; ++f) {
            std::complex<double> s = 0;
            for (int n = lpad; n < lpad + cnt; ++n) s += basis[n] * tw[(int)(((long long)f * n) % nfft)];
            spec[f] = s;
            mags[f] = std::abs(s);
            norm += mags[f];
        }
        sorted = mags;
        std::sort(sorted.begin(), sorted.end());
        double cum = 0, thr = sorted[0];
        for (int f = 0; f < nb; ++f) {           // first index whose cumulative normalised magnitude reaches the 1 % quantile
            cum += sorted[f] / norm;
            if (!(cum < 0.01)) { thr = sorted[f]; break; }
        }
        const double scale = std::sqrt(sr_base / sr_i) / std::sqrt(len_base[k]);
        for (int n = 0; n < nfft; ++n) {
            std::complex<double> s = 0;
            for (int f = 0; f < nb; ++f)
                if (mags[f] >= thr) s += spec[f] * tw[(int)(((long long)f * n) % nfft)];
            kern[(size_t)k * nfft + n] = s * scale;
        }
    }
}

}  // namespace

extern "C" int amtx_cqt_plan_destroy(amtx_cqt_plan* p) {
    if (!p) return AMTX_OK;
    for (auto& l : p->levels) {
        if (l.d_w) (void)hipFree(l.d_w);
        if (l.d_map) (void)hipFree(l.d_map);
    }
    if (p->d_tfrag) (void)hipFree(p->d_tfrag);
    delete p;
    return AMTX_OK;
}

extern "C" int amtx_cqt_plan_create(amtx_cqt_plan** out, int sample_rate, int hop_length, double fmin, int n_bins, int bins_per_octave,
                                    double gamma, const double* harmonics, int n_harmonics, int truncate_to_expected, int librosa09) {
    AMTX_REQUIRE(out, "amtx_cqt_plan_create: null plan pointer");
    *out = nullptr;
    AMTX_REQUIRE(sample_rate > 0 && hop_length > 0 && fmin > 0 && n_bins > 0 && bins_per_octave > 0 && gamma >= 0 && n_harmonics > 0 &&
                     n_harmonics <= MAX_BANKS && harmonics, "amtx_cqt_plan_create: bad argument");
    amtx_cqt_plan* p = new amtx_cqt_plan();
    p->sr = sample_rate; p->hop = hop_length; p->n_bins = n_bins; p->bpo = bins_per_octave; p->n_harm = n_harmonics;
    p->lib09 = librosa09; p->truncate = truncate_to_expected; p->fmin = fmin; p->gamma = gamma;
    p->alpha = alpha_of(bins_per_octave, librosa09);
    p->harmonics.assign(harmonics, harmonics + n_harmonics);
    const int n_oct = (n_bins + bins_per_octave - 1) / bins_per_octave;
    const int nf_full = std::min(bins_per_octave, n_bins);
    const double Q = 1.0 / p->alpha;
    for (int h = 0; h < n_harmonics; ++h) {
        const double f0 = harmonics[h] * fmin;
        std::vector<double> freqs(n_bins);
        double cutoff = 0;
        for (int k = 0; k < n_bins; ++k) {
            freqs[k] = f0 * std::pow(2.0, (double)k / bins_per_octave);
            cutoff = std::max(cutoff, freqs[k] * (1 + 0.5 * HANN_BW / Q) + 0.5 * gamma);
        }
        if (cutoff > sample_rate / 2.0) {
            amtx_set_error("amtx_cqt_plan_create: wavelet basis with max frequency=%g Hz (harmonic %g) would exceed the Nyquist frequency=%g",
                           freqs[n_bins - 1], harmonics[h], sample_rate / 2.0);
            amtx_cqt_plan_destroy(p);
            return AMTX_ERR_ARG;
        }
        const int c = early_count(sample_rate / 2.0, cutoff, hop_length, n_oct);
        p->early.push_back(c);
        const double sr_base = sample_rate / std::pow(2.0, c);
        std::vector<double> len_all(n_bins);
        for (int k = 0; k < n_bins; ++k) len_all[k] = Q * sr_base / (freqs[k] + gamma / p->alpha);
        for (int j = 0; j < n_oct; ++j) {
            const int hi = n_bins - nf_full * j, lo = std::max(0, n_bins - nf_full * (j + 1));
            if (hi <= 0) break;
            const int level = c + j;
            if ((hop_length >> level) << level != hop_length || (hop_length >> level) < 4) {
                amtx_set_error("amtx_cqt_plan_create: hop_length=%d is not divisible far enough for %d pyramid levels (level hop must be a "
                               "multiple of 4)", hop_length, level + 1);
                amtx_cqt_plan_destroy(p);
                return AMTX_ERR_UNSUPPORTED;
            }
            if ((int)p->levels.size() <= level) p->levels.resize(level + 1);
            Level& L = p->levels[level];
            L.hop = hop_length >> level;
            std::vector<double> fr(freqs.begin() + lo, freqs.begin() + hi), lb(len_all.begin() + lo, len_all.begin() + hi);
            int nfft = 0;
            std::vector<std::complex<double>> kern;
            build_bank(fr, sample_rate / std::pow(2.0, level), sr_base, gamma, p->alpha, lb, nfft, kern);
            if ((int)L.banks.size() >= MAX_BANKS) {
                amtx_set_error("amtx_cqt_plan_create: more than %d banks on one pyramid level", MAX_BANKS);
                amtx_cqt_plan_destroy(p);
                return AMTX_ERR_UNSUPPORTED;
            }
            BankDev bd; bd.col0 = L.ncols; bd.nf = hi - lo; bd.harm = h; bd.bin0 = lo; bd.frames = 0;
            L.banks.push_back(bd);
            L.ncols += 2 * (hi - lo);
            L.nfft = std::max(L.nfft, nfft);
            L.raw.emplace_back(nfft, std::move(kern));
        }
    }
    // stack the banks of every level (kernels centred in the level's n_fft window), pack hi/lo planes, upload
    for (auto& L : p->levels) {
        if (L.banks.empty()) continue;
        p->pad = std::max(p->pad, L.nfft / 2);
        std::vector<float> W((size_t)L.ncols * L.nfft, 0.f);
        for (size_t bi = 0; bi < L.banks.size(); ++bi) {
            const BankDev& bd = L.banks[bi];
            const int nfft = L.raw[bi].first, off = (L.nfft - nfft) / 2;
            for (int k = 0; k < bd.nf; ++k)
                for (int n = 0; n < nfft; ++n) {
                    const std::complex<double> v = L.raw[bi].second[(size_t)k * nfft + n];
                    // (re, im) of a filter in neighbouring columns: the GEMM's magnitude epilogue combines them in registers
                    W[(size_t)(bd.col0 + 2 * k) * L.nfft + off + n] = (float)v.real();
                    W[(size_t)(bd.col0 + 2 * k + 1) * L.nfft + off + n] = (float)v.imag();
                }
        }
        L.raw.clear();
        amtx_gemm_pack_dims(L.ncols, L.nfft, &L.n_pad, &L.k_pad);
        std::vector<bf16_t> packed((size_t)L.n_pad * L.k_pad * 2);
        amtx_gemm_pack_host(W.data(), L.nfft, L.ncols, L.nfft, 2, packed.data());
        hipError_t e = hipMalloc(&L.d_w, packed.size() * 2);
        if (e == hipSuccess) e = hipMemcpy(L.d_w, packed.data(), packed.size() * 2, hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            std::vector<int2> map((size_t)L.ncols / 2);
            for (const BankDev& bd : L.banks)
                for (int k = 0; k < bd.nf; ++k) map[(size_t)bd.col0 / 2 + k] = make_int2(bd.harm * n_bins + bd.bin0 + k, bd.harm);
            e = hipMalloc(&L.d_map, map.size() * sizeof(int2));
            if (e == hipSuccess) e = hipMemcpy(L.d_map, map.data(), map.size() * sizeof(int2), hipMemcpyHostToDevice);
        }
        if (e != hipSuccess) {
            amtx_set_error("amtx_cqt_plan_create: weight upload failed: %s", hipGetErrorString(e));
            amtx_cqt_plan_destroy(p);
            return AMTX_ERR_HIP;
        }
    }
    p->pad = (p->pad + 3) & ~3;
    // decimator taps
    std::vector<float> taps(DEC_TAPS, 0.0f);
    {
        std::vector<double> h(DEC_TAPS);
        double sum = 0;
        for (int i = 0; i < DEC_TAPS; ++i) {
            const double n = i - DEC_HALF, x = 2.0 * DEC_CUTOFF * n;
            const double sinc = (n == 0) ? 1.0 : std::sin(PI * x) / (PI * x);
            const double r = 2.0 * i / (DEC_TAPS - 1) - 1.0;
            h[i] = 2.0 * DEC_CUTOFF * sinc * bessel_i0(DEC_BETA * std::sqrt(std::max(0.0, 1.0 - r * r))) / bessel_i0(DEC_BETA);
            sum += h[i];
        }
        for (int i = 0; i < DEC_TAPS; ++i) taps[i] = (float)(h[i] / sum);
    }
    std::vector<bf16_t> tfrag((size_t)DEC_NKS * 3 * 64 * 8);
    for (int ks = 0; ks < DEC_NKS; ++ks)
        for (int l = 0; l < 64; ++l)
            for (int j = 0; j < 8; ++j) {
                const int i = l & 15, k = 32 * ks + 8 * (l >> 4) + j, tap = k - 2 * i;
                const float v = (tap >= 0 && tap < DEC_TAPS) ? taps[tap] : 0.0f;
                const bf16_t hi = f32_to_bf16_rn(v);
                const float r1 = v - bf16_to_f32(hi);
                const bf16_t mid = f32_to_bf16_rn(r1);
                tfrag[((size_t)(ks * 3 + 0) * 64 + l) * 8 + j] = hi;
                tfrag[((size_t)(ks * 3 + 1) * 64 + l) * 8 + j] = mid;
                tfrag[((size_t)(ks * 3 + 2) * 64 + l) * 8 + j] = f32_to_bf16_rn(r1 - bf16_to_f32(mid));
            }
    hipError_t e = hipMalloc(&p->d_tfrag, tfrag.size() * sizeof(bf16_t));
    if (e == hipSuccess) e = hipMemcpy(p->d_tfrag, tfrag.data(), tfrag.size() * sizeof(bf16_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        amtx_set_error("amtx_cqt_plan_create: device allocation failed: %s", hipGetErrorString(e));
        amtx_cqt_plan_destroy(p);
        return AMTX_ERR_HIP;
    }
    *out = p;
    return AMTX_OK;
}

namespace {

struct CqtDims {
    std::vector<int64_t> len, stride, frames;     // per level
    std::vector<int> frames_h;                    // per harmonic: librosa's own output length
    int64_t t_buf = 0, t_out = 0;
    size_t off_pyr = 0, off_r = 0, off_mag = 0, off_max = 0, total = 0;
    std::vector<size_t> pyr_off, r_off;
};

// VQT.get_expected_frames (features/vqt.py:102-134) with the reference's own early-downsample estimate (librosa-0.9 Q)
int64_t reference_expected_frames(const amtx_cqt_plan* p, double f0, int64_t n) {
    const double fmax = f0 * std::pow(2.0, (double)(p->n_bins - 1) / p->bpo);
    const double cQ = 1.0 / (std::pow(2.0, 1.0 / p->bpo) - 1.0);
    const double cutoff = fmax * (1 + 0.5 * HANN_BW / cQ) + 0.5 * p->gamma;
    const int n_oct = (p->n_bins + p->bpo - 1) / p->bpo;
    const int c = early_count(p->sr / 2.0, cutoff, p->hop, n_oct);
    int64_t best = -1;
    for (int k = c; k < c + n_oct; ++k) {
        const int64_t sig = (int64_t)std::ceil((double)n / std::pow(2.0, k));
        const int64_t hop = p->hop >> k;
        if (hop <= 0) continue;
        const int64_t f = sig / hop + 1;
        if (best < 0 || f < best) best = f;
    }
    return best;
}

CqtDims dims(const amtx_cqt_plan* p, int B, int64_t n) {
    CqtDims d;
    const int nl = (int)p->levels.size();
    d.len.resize(nl); d.stride.resize(nl); d.frames.resize(nl); d.pyr_off.resize(nl); d.r_off.resize(nl);
    int64_t len = n;
    size_t off = 0;
    for (int l = 0; l < nl; ++l) {
        if (l > 0) len = (len + 1) / 2;
        d.len[l] = len;
        d.stride[l] = ((2 * (int64_t)p->pad + len + 3) / 4) * 4 + 4;
        d.frames[l] = p->levels[l].hop > 0 ? 1 + len / p->levels[l].hop : 0;
        d.pyr_off[l] = off;
        off += ((size_t)B * d.stride[l] * 4 + 255) & ~(size_t)255;
    }
    d.off_r = off;          // (the complex responses used to live here; the GEMM's magnitude epilogue writes the map directly)
    for (int l = 0; l < nl; ++l) d.r_off[l] = off;
    const int n_oct = (p->n_bins + p->bpo - 1) / p->bpo;
    d.frames_h.resize(p->n_harm);
    int64_t tmin = -1, tref = -1;
    for (int h = 0; h < p->n_harm; ++h) {
        int64_t t = -1;
        for (int j = 0; j < n_oct; ++j) {
            const int l = p->early[h] + j;
            if (l < nl && !p->levels[l].banks.empty()) t = (t < 0) ? d.frames[l] : std::min(t, d.frames[l]);
        }
        d.frames_h[h] = (int)t;
        d.t_buf = std::max<int64_t>(d.t_buf, t);
        tmin = (tmin < 0) ? t : std::min(tmin, t);
        const int64_t r = reference_expected_frames(p, p->harmonics[h] * p->fmin, n);
        tref = (tref < 0) ? r : std::min(tref, r);
    }
    d.t_out = p->truncate ? std::min(tmin, tref) : tmin;
    d.off_mag = off;
    off += ((size_t)B * p->n_harm * p->n_bins * d.t_buf * 4 + 255) & ~(size_t)255;
    d.off_max = off;
    off += ((size_t)B * p->n_harm * 4 + 255) & ~(size_t)255;
    d.total = off;
    return d;
}

}  // namespace

extern "C" int amtx_cqt_num_harmonics(const amtx_cqt_plan* p) { return p ? p->n_harm : AMTX_ERR_ARG; }

extern "C" int64_t amtx_cqt_num_frames(const amtx_cqt_plan* p, int64_t num_samples) {
    if (!p || num_samples <= 0) return p ? 0 : AMTX_ERR_ARG;
    return dims(p, 1, num_samples).t_out;
}

extern "C" size_t amtx_cqt_workspace_bytes(const amtx_cqt_plan* p, int batch, int64_t num_samples) {
    if (!p || batch <= 0 || num_samples <= 0) return 0;
    return dims(p, batch, num_samples).total;
}

namespace {

// The file's A/B switches, read once per process
struct CqtSwitches {
    bool copy_level0;      // AMTX_CQT_COPY_LEVEL0: amtx_cqt_forward copies the clip between two paddings instead of reading the audio in place
    bool gemm_basis;       // AMTX_CQT_GEMM_BASIS: round 4's basis products (all levels in one launch of the generic fp32-A two-plane GEMM)
};
const CqtSwitches& cqt_switches() {
    static const CqtSwitches sw{getenv("AMTX_CQT_COPY_LEVEL0") != nullptr, getenv("AMTX_CQT_GEMM_BASIS") != nullptr};
    return sw;
}

struct PyrLevel { float* pyr; int64_t len, stride; };      // a level's buffer (first element of clip 0's left pad), samples, elements per clip
// The pyramid chain of `B` equal clips of `n` samples (amtx_cqt_forward) or of one track as a batch of one (amtx_cqt_pyramid_build); level_of(l)
// answers where level l lies.  direct0 (zero pads only): level 0 is the audio where it lies -- the first decimation and the level-0 basis
// product read it there (out-of-clip samples read as zero: the decimator clamps, the basis kernels take a valid range), so the clip is not
// copied between two paddings first (0.45 ms and 1.3 GB per 512 clips).  `maxbuf`: the per-(clip, harmonic) maxima the chain's first kernel
// resets (the level-0 copy, or the decimation that reads the audio); null: nothing to reset.
template <class LevelOf>
int pyramid_chain(const amtx_cqt_plan* p, const float* audio, int64_t n, int64_t audio_stride, int B, bool direct0, float* maxbuf, LevelOf level_of,
                  hipStream_t s) {
    const int nl = (int)p->levels.size(), zero_pads = p->lib09 ? 0 : 1;
    PyrLevel prev{}, cur{};
    for (int l = 0; l < nl; prev = cur, ++l) {
        cur = level_of(l);
        if (l == 0) {
            if (direct0) continue;
            const unsigned nb = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
            hipLaunchKernelGGL(cqt_level0_kernel, dim3(nb, B), dim3(256), 0, s, audio, n, audio_stride, cur.pyr, cur.stride, p->pad, zero_pads, maxbuf, p->n_harm);
        } else {
            const bool from_audio = direct0 && l == 1;
            const int rc = amtx_launch_cqt_decimate(from_audio ? audio : (const float*)prev.pyr, prev.len, from_audio ? audio_stride : prev.stride,
                                                    from_audio ? 0 : p->pad, cur.pyr, cur.len, cur.stride, p->pad, p->d_tfrag, zero_pads,
                                                    from_audio ? maxbuf : (float*)nullptr, p->n_harm, B, s);
            if (rc != AMTX_OK) return rc;
        }
        AMTX_CHECK_LAUNCH();
        if (!zero_pads) {      // librosa 0.9: reflecting centre pad, from the level's own samples
            hipLaunchKernelGGL(cqt_pad_kernel, dim3(8, B), dim3(256), 0, s, cur.pyr, cur.len, cur.stride, p->pad, p->lib09);
            AMTX_CHECK_LAUNCH();
        }
    }
    return AMTX_OK;
}

// The basis products' route: whether the windowed kernel computes them (every other plan goes through the generic GEMM and has no
// clip form) and, if so, its launches, one per n_fft.  Pure: the plan's host fields and sizes in.
struct BasisLaunch { int ks; BasisLevs ls; int slices; unsigned gx; size_t lds; };      // cqt_basis_kernel<ks> / cqt_basis_clips_kernel<ks>, grid (gx, slices)
struct BasisRoute {
    bool windowed;
    int frames[BAS_MAXLEV], ft[BAS_MAXLEV], tiles_per_clip[BAS_MAXLEV];      // per level: frames per clip (0: no banks), frames per tile, tiles
    int nlaunch;
    BasisLaunch launch[2];
};
// d: the clips' level lengths and frames, or PLAN_ONLY: clips of resident tracks, whose lengths amtx_cqt_track_layout was asked about when the
// bank was laid out -- the plan alone decides, and every level runs t_buf frames.  t_buf: frames of the power map's rows; B: clips
constexpr const CqtDims* PLAN_ONLY = nullptr;
BasisRoute basis_route(const amtx_cqt_plan* p, const CqtDims* d, int64_t t_buf, int B) {
    BasisRoute r{};
    const int nl = (int)p->levels.size();
    r.windowed = nl <= BAS_MAXLEV && p->n_harm <= 16 && (int64_t)p->n_harm * p->n_bins * t_buf < (1ll << 31);
    for (int l = 0; l < nl && r.windowed; ++l) {
        const Level& L = p->levels[l];
        if (L.banks.empty()) continue;
        r.windowed = (L.nfft == 128 || L.nfft == 256) && L.k_pad >= L.nfft && L.ncols <= 256 && L.ncols % 2 == 0 && L.hop >= 4 && (L.hop & (L.hop - 1)) == 0 &&
                     (L.hop <= 512) && (d == PLAN_ONLY || d->len[l] >= 4);
    }
    if (!r.windowed) return r;
    for (int l = 0; l < nl; ++l) {      // the tiling of a level over its frames
        const Level& L = p->levels[l];
        if (L.banks.empty()) continue;
        r.frames[l] = (int)(d == PLAN_ONLY ? t_buf : d->frames[l]);
        const int hs0 = std::min(L.hop, L.nfft);
        const int ftl = std::max(16, std::min(128, ((BAS_MAXWIN - L.nfft) / hs0 + 1) / 16 * 16));
        r.ft[l] = std::min(ftl, (r.frames[l] + 15) / 16 * 16);
        r.tiles_per_clip[l] = (r.frames[l] + r.ft[l] - 1) / r.ft[l];
    }
    for (int kk = 128; kk <= 256; kk *= 2) {
        BasisLaunch& bn = r.launch[r.nlaunch];
        bn = BasisLaunch{};
        bn.ks = kk / 32;
        for (int l = 0; l < nl; ++l) {
            if (r.frames[l] <= 0 || p->levels[l].nfft != kk) continue;
            const int hs = std::min(p->levels[l].hop, kk);               // frame stride of the staged copy (cqt_basis_kernel)
            const int ws_s = (r.ft[l] - 1) * hs + kk;
            const int wsp = ws_s + bas_pad(hs) * ((ws_s + hs - 1) / hs);
            bn.lds = std::max(bn.lds, (size_t)((wsp + 7) & ~7) * 2 * 2 + 64);
            bn.ls.lev[bn.ls.n++] = l;
        }
        if (!bn.ls.n) continue;
        // two 256-thread blocks per CU; the levels (and the second column slice of the wide ones) share the chip: 512 blocks dealt EVENLY to the
        // levels (dealing them by staged samples, by matrix work or by a mix was measured slower, 2.2 - 2.6 against 1.97 ms for the
        // front-end: the deep levels' tiles are as many as the shallow ones' and a tile's fixed costs -- barriers, a load round trip, the
        // maxima's atomics -- weigh as much as its size)
        bn.slices = 1;
        for (int i = 0; i < bn.ls.n; ++i) bn.slices = std::max(bn.slices, (p->levels[bn.ls.lev[i]].ncols + 127) / 128);
        bn.ls.b0[0] = 0;
        for (int i = 0; i < bn.ls.n; ++i) {
            const int64_t tiles = (int64_t)r.tiles_per_clip[bn.ls.lev[i]] * B;
            bn.ls.b0[i + 1] = bn.ls.b0[i] + (int)std::min<int64_t>(std::max(8, 512 / bn.ls.n), tiles);
        }
        bn.gx = (unsigned)bn.ls.b0[bn.ls.n];
        ++r.nlaunch;
    }
    return r;
}

// what both forms of the basis launch set alike; the level signals (sig, sig_gs, len, off) and BasisArgs.rows are the caller's
BasisArgs basis_args(const amtx_cqt_plan* p, const BasisRoute& r, int B, float* mag, int64_t t_buf, float* maxbuf) {
    BasisArgs ba{};
    ba.nlev = (int)p->levels.size(); ba.B = B; ba.ntiles = 0;
    ba.mag = mag; ba.mag_gs = (int64_t)p->n_harm * p->n_bins * t_buf; ba.mag_pitch = t_buf;
    ba.maxbuf = maxbuf; ba.n_harm = p->n_harm;
    for (int l = 0; l < ba.nlev; ++l) {
        const Level& L = p->levels[l];
        if (L.banks.empty()) continue;
        BasisLevel& bl = ba.lev[l];
        bl.w = L.d_w; bl.map = L.d_map; bl.n_pad = L.n_pad; bl.k_pad = L.k_pad; bl.ncols = L.ncols; bl.hop = L.hop;
        bl.frames = r.frames[l]; bl.ft = r.ft[l]; bl.tiles_per_clip = r.tiles_per_clip[l];
    }
    return ba;
}

template <int KS>
int basis_launch_ks(const BasisLaunch& bn, const BasisArgs& ba, const BasisClips* cl, hipStream_t s) {
    if (cl) {
        AMTX_GRANT_LDS(cqt_basis_clips_kernel<KS>, bn.lds);
        hipLaunchKernelGGL(cqt_basis_clips_kernel<KS>, dim3(bn.gx, bn.slices), dim3(256), bn.lds, s, ba, bn.ls, *cl);
    } else {
        AMTX_GRANT_LDS(cqt_basis_kernel<KS>, bn.lds);
        hipLaunchKernelGGL(cqt_basis_kernel<KS>, dim3(bn.gx, bn.slices), dim3(256), bn.lds, s, ba, bn.ls);
    }
    AMTX_CHECK_LAUNCH();
    return AMTX_OK;
}

// the route's launches, one per n_fft; cl: the clip form (cqt_basis_clips_kernel)
int basis_launch(const BasisRoute& r, const BasisArgs& ba, const BasisClips* cl, hipStream_t s) {
    for (int i = 0; i < r.nlaunch; ++i) {
        const BasisLaunch& bn = r.launch[i];
        const int rc = bn.ks == 8 ? basis_launch_ks<8>(bn, ba, cl, s) : basis_launch_ks<4>(bn, ba, cl, s);
        if (rc != AMTX_OK) return rc;
    }
    return AMTX_OK;
}

// amplitude_to_db(ref = max) -> /80 + 1 of the power map mag[B][n_harm][n_bins][t_buf], truncated to t_out frames: fp32 into `out`, or, out16 !=
// null, [B][t_out][n_bins][8] bf16 (lo_plane != 0: and its second plane).  `fn` names the 16-bit form in its refusal.
int scale_launch(const char* fn, const amtx_cqt_plan* p, const float* mag, const float* refs, int B, int64_t t_buf, int64_t t_out, int decibels, float* out,
                 void* out16, int64_t lo_plane, hipStream_t s) {
    if (out16) {
        AMTX_REQUIRE(p->n_harm <= 8 && ((uintptr_t)out16 % 16) == 0, "%s: at most 8 harmonics, output 16-byte aligned", fn);
        const int nbc = std::min(p->n_bins, 120);            // bins per pass: 32 x 121 x 16 bytes of LDS
        const size_t lds = (size_t)(lo_plane ? 2 : 1) * SC16_TT * (nbc + 1) * 16 + 64;
        AMTX_GRANT_LDS(cqt_scale16_kernel, lds);
        hipLaunchKernelGGL(cqt_scale16_kernel, dim3((unsigned)((t_out + SC16_TT - 1) / SC16_TT), B), dim3(256), lds, s, mag, refs, p->n_harm, p->n_bins, nbc,
                           t_buf, t_out, decibels, (uint4*)out16, lo_plane);
    } else {
        hipLaunchKernelGGL(cqt_scale_kernel, dim3(8, B * p->n_harm), dim3(256), 0, s, mag, refs, p->n_bins, t_buf, t_out, decibels, out);
    }
    AMTX_CHECK_LAUNCH();
    return AMTX_OK;
}

}  // namespace

// out16 != null: the map as [B][T][n_bins][8] bf16 (amtx_cqt_forward16) instead of `out`
static int cqt_forward_impl(const amtx_cqt_plan* p, const float* audio, int64_t num_samples, int64_t audio_stride, int batch, int decibels,
                            void* workspace, size_t workspace_bytes, float* out, void* out16, void* stream_, int64_t lo_plane = 0) {
    AMTX_REQUIRE(p && audio && workspace && (out || out16), "amtx_cqt_forward: null pointer");
    AMTX_REQUIRE(batch > 0 && batch < 65536 && num_samples > 0 && audio_stride >= num_samples, "amtx_cqt_forward: bad batch/num_samples");
    AMTX_REQUIRE(((uintptr_t)workspace % 256) == 0, "amtx_cqt_forward: workspace must be 256-byte aligned");
    const CqtDims d = dims(p, batch, num_samples);
    AMTX_REQUIRE(workspace_bytes >= d.total, "amtx_cqt_forward: workspace too small (%zu < %zu)", workspace_bytes, d.total);
    AMTX_REQUIRE(d.t_out > 0, "amtx_cqt_forward: clip too short");
    if (p->lib09) AMTX_REQUIRE(d.len.back() > p->pad, "amtx_cqt_forward: reflect padding needs a longer clip");
    hipStream_t s = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    const int B = batch, nl = (int)p->levels.size();
    float* mag = (float*)(ws + d.off_mag);
    float* maxbuf = (float*)(ws + d.off_max);
    const int zero_pads = p->lib09 ? 0 : 1;
    const CqtSwitches& sw = cqt_switches();

    // zero centre padding: level 0 of the pyramid IS the caller's audio (pyramid_chain), unless AMTX_CQT_COPY_LEVEL0 keeps the copy for the A/B
    const bool direct0 = zero_pads && !sw.copy_level0;
    if (direct0 && nl == 1) AMTX_CHECK_HIP(hipMemsetAsync(maxbuf, 0, sizeof(float) * B * p->n_harm, s));
    int rc = pyramid_chain(p, audio, num_samples, audio_stride, B, direct0, maxbuf,
                           [&](int l) { return PyrLevel{(float*)(ws + d.pyr_off[l]), d.len[l], d.stride[l]}; }, s);
    if (rc != AMTX_OK) return rc;
    // the basis products of all levels: the windowed kernel, or (AMTX_CQT_GEMM_BASIS=1: for the A/B) round 4's path
    const BasisRoute route = basis_route(p, &d, d.t_buf, B);
    if (route.windowed && !sw.gemm_basis) {
        BasisArgs ba = basis_args(p, route, B, mag, d.t_buf, maxbuf);
        for (int h = 0; h < p->n_harm; ++h) ba.rows[h] = d.frames_h[h];
        for (int l = 0; l < nl; ++l) {
            BasisLevel& bl = ba.lev[l];
            if (bl.frames <= 0) continue;
            if (direct0 && l == 0) { bl.sig = audio; bl.sig_gs = audio_stride; }
            else { bl.sig = (const float*)(ws + d.pyr_off[l]) + p->pad; bl.sig_gs = d.stride[l]; }
            bl.len = d.len[l];
            // librosa 0.9's reflecting pads live in the pyramid buffer on both sides of the signal: there every sample the windows touch exists
            if (!zero_pads) { bl.sig -= p->pad; bl.off = p->pad; bl.len = d.stride[l]; }
        }
        rc = basis_launch(route, ba, nullptr, s);
        if (rc != AMTX_OK) return rc;
    } else {
    // the basis products of ALL levels in one launch (same kernel, per-level A / W / sizes; 8 launches before)
    GemmArgs gs[AMTX_GEMM_MULTI_MAX];
    int ng = 0;
    for (int l = 0; l < nl; ++l) {
        const Level& L = p->levels[l];
        if (L.banks.empty()) continue;
        // the basis product with the power epilogue: |re + i im|^2 of every filter goes straight into mag[b][harmonic][bin][t]
        // (transposed, truncated to the harmonic's frame count); the complex response never touches HBM (it was written by the GEMM
        // and read back by a magnitude / transpose kernel: 0.4 GB per level and 512 clips, a third of the front-end's traffic)
        GemmArgs g;
        g.A = (const float*)(ws + d.pyr_off[l]) + (p->pad - L.nfft / 2); g.lda = L.hop; g.a_type = AMTX_T_F32;
        if (direct0 && l == 0) {   // rows start n_fft / 2 before the clip and run past its end: bounded reads straight from the audio
            // a pointer n_fft / 2 elements BEFORE the caller's allocation: nothing below a_valid_lo is ever dereferenced (AStage::load), and
            // the range starts exactly where the clip does
            g.A = audio - L.nfft / 2;
            g.a_valid_lo = L.nfft / 2; g.a_valid_hi = (int64_t)L.nfft / 2 + num_samples;
            AMTX_REQUIRE(g.a_valid_lo >= L.nfft / 2, "amtx_cqt_forward: internal: level-0 rows would reach below the clip");
        }
        g.W = L.d_w; g.n_pad = L.n_pad; g.k_pad = L.k_pad; g.planes = 2; g.bias = nullptr;
        g.C = nullptr; g.ldc = L.ncols; g.c_type = AMTX_T_F32;
        g.M = d.frames[l]; g.N = L.ncols; g.K = L.nfft;
        g.groups = B; g.a_gs = (direct0 && l == 0) ? audio_stride : d.stride[l]; g.w_gs = 0; g.bias_gs = 0; g.c_gs = 0;
        g.pair_map = L.d_map; g.pair_out = mag; g.pair_gs = (int64_t)p->n_harm * p->n_bins * d.t_buf; g.pair_pitch = d.t_buf;
        for (int h = 0; h < p->n_harm && h < 16; ++h) g.pair_rows[h] = d.frames_h[h];
        g.pair_max = maxbuf; g.pair_nh = p->n_harm;       // the per-(clip, harmonic) maxima of the dB reference, kept by the epilogue
        if (ng == AMTX_GEMM_MULTI_MAX) {
            rc = amtx_launch_gemm_multi(gs, ng, s);
            if (rc != AMTX_OK) return rc;
            ng = 0;
        }
        gs[ng++] = g;
    }
    if (ng) {
        rc = amtx_launch_gemm_multi(gs, ng, s);
        if (rc != AMTX_OK) return rc;
    }
    }
    return scale_launch("amtx_cqt_forward16", p, mag, maxbuf, B, d.t_buf, d.t_out, decibels, out, out16, lo_plane, s);
}

extern "C" int amtx_cqt_forward(const amtx_cqt_plan* p, const float* audio, int64_t num_samples, int64_t audio_stride, int batch, int decibels,
                                void* workspace, size_t workspace_bytes, float* out, void* stream_) {
    AMTX_REQUIRE(out, "amtx_cqt_forward: null pointer");
    return cqt_forward_impl(p, audio, num_samples, audio_stride, batch, decibels, workspace, workspace_bytes, out, nullptr, stream_);
}

extern "C" int amtx_cqt_forward16(const amtx_cqt_plan* p, const float* audio, int64_t num_samples, int64_t audio_stride, int batch, int decibels,
                                  void* workspace, size_t workspace_bytes, void* out16, void* stream_) {
    AMTX_REQUIRE(out16, "amtx_cqt_forward16: null pointer");
    return cqt_forward_impl(p, audio, num_samples, audio_stride, batch, decibels, workspace, workspace_bytes, nullptr, out16, stream_);
}

// The same map as TWO 16-bit planes for the two-plane (x3) engine: hi = bf16(v) at out16 (exactly amtx_cqt_forward16's map), lo = bf16(v - hi)
// `plane_elems` 16-bit elements behind it (>= B T n_bins 8, a multiple of 8) -- split_bf16x2 of the fp32 feature amtx_cqt_forward writes.
extern "C" int amtx_cqt_forward16_split(const amtx_cqt_plan* p, const float* audio, int64_t num_samples, int64_t audio_stride, int batch, int decibels,
                                        void* workspace, size_t workspace_bytes, void* out16, int64_t plane_elems, void* stream_) {
    AMTX_REQUIRE(out16 && plane_elems > 0 && plane_elems % 8 == 0, "amtx_cqt_forward16_split: null pointer / plane stride not a multiple of 8 elements");
    return cqt_forward_impl(p, audio, num_samples, audio_stride, batch, decibels, workspace, workspace_bytes, nullptr, out16, stream_, plane_elems / 8);
}

// ------------------------------------------------------------------------------------------------------------------------------
// Clips cut from the resident pyramids of whole tracks (include/amtx_pyramid.h).  The tables are device memory: the track table is checked
// on its host copy where the bank is built (amtx_cqt_pyramid_build), the descriptors where they are made (amt_tools_amd/tracks.py).
namespace {

int pyr_cols(const amtx_cqt_plan* p) { return 4 + 3 * (int)p->levels.size() + p->n_harm; }

// the basis products of `B` clips of `num_frames` frames (desc) or of the table's `B` tracks whole (desc = null, num_frames = the longest's
// rows), by the route clips_check made of the same B and num_frames: power maps into `mag` and / or maxima into `maxima`
int clips_basis(const amtx_cqt_plan* p, const BasisRoute& route, const float* audio, const float* pyramid, const int64_t* tab, const int64_t* desc, int B,
                int64_t num_frames, float* mag, float* maxima, hipStream_t s) {
    const int nl = (int)p->levels.size();
    BasisArgs ba = basis_args(p, route, B, mag, num_frames, maxima);
    BasisClips cl;
    cl.tab = tab; cl.desc = desc; cl.cols = pyr_cols(p); cl.rows_col = 4 + 3 * nl; cl.num_frames = (int)num_frames;
    for (int l = 0; l < nl; ++l) {
        BasisLevel& bl = ba.lev[l];
        cl.base_col[l] = 4 + 3 * l;
        if (bl.frames <= 0) { cl.len_col[l] = 4 + 3 * l + 1; continue; }
        if (!p->lib09 && l == 0) {            // zero pads: level 0 is the audio where it lies
            bl.sig = audio; bl.off = 0;
            cl.base_col[l] = 0; cl.len_col[l] = 1;
        } else if (!p->lib09) {               // the samples behind the level's left pad; everything outside them reads as zero
            bl.sig = pyramid + p->pad; bl.off = 0;
            cl.len_col[l] = 4 + 3 * l + 1;
        } else {                              // reflecting pads: every sample of the level's stride exists
            bl.sig = pyramid; bl.off = p->pad;
            cl.len_col[l] = 4 + 3 * l + 2;
        }
    }
    return basis_launch(route, ba, &cl, s);
}

// the request's sizes, and the route of its basis products (PLAN_ONLY: the tracks' lengths were checked where the bank was laid out)
int clips_check(const char* fn, const amtx_cqt_plan* p, int batch, int64_t num_frames, BasisRoute& route) {
    AMTX_REQUIRE(batch > 0 && batch < 65536 && num_frames > 0 && num_frames < (1ll << 31), "%s: bad batch/num_frames", fn);
    route = basis_route(p, PLAN_ONLY, num_frames, batch);
    if (!route.windowed) {
        amtx_set_error("%s: this plan's basis products have no clip form (the windowed kernel does not cover it)", fn);
        return AMTX_ERR_UNSUPPORTED;
    }
    return AMTX_OK;
}

int clips_scaled(const char* fn, const amtx_cqt_plan* p, const float* audio, const float* pyramid, const int64_t* tab, const int64_t* desc, int batch,
                 int64_t num_frames, const float* refs, int decibels, void* workspace, size_t workspace_bytes, float* out, void* out16,
                 int64_t lo_plane, void* stream_) {
    AMTX_REQUIRE(p && audio && pyramid && tab && desc && refs && workspace && (out || out16), "%s: null argument", fn);
    BasisRoute route;
    int rc = clips_check(fn, p, batch, num_frames, route);
    if (rc != AMTX_OK) return rc;
    AMTX_REQUIRE(((uintptr_t)workspace % 256) == 0, "%s: workspace must be 256-byte aligned", fn);
    const size_t need = amtx_cqt_clips_workspace_bytes(p, batch, num_frames);
    AMTX_REQUIRE(workspace_bytes >= need, "%s: workspace too small (%zu < %zu)", fn, workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream_;
    float* mag = (float*)workspace;
    rc = clips_basis(p, route, audio, pyramid, tab, desc, batch, num_frames, mag, nullptr, s);
    if (rc != AMTX_OK) return rc;
    // the whole-track scaling kernels with a clip-sized map (t_buf = t_out = num_frames) and the tracks' maxima as references
    return scale_launch(fn, p, mag, refs, batch, num_frames, num_frames, decibels, out, out16, lo_plane, s);
}

}  // namespace

extern "C" int amtx_cqt_track_cols(const amtx_cqt_plan* p) {
    AMTX_REQUIRE(p, "amtx_cqt_track_cols: null plan");
    return pyr_cols(p);
}

extern "C" int amtx_cqt_track_layout(const amtx_cqt_plan* p, int64_t num_samples, int64_t* level_len, int64_t* level_stride, int64_t* rows_h,
                                     int64_t* frames) {
    AMTX_REQUIRE(p && level_len && level_stride && rows_h && frames, "amtx_cqt_track_layout: null argument");
    AMTX_REQUIRE(num_samples > 0, "amtx_cqt_track_layout: bad num_samples");
    const int nl = (int)p->levels.size();
    const CqtDims d = dims(p, 1, num_samples);
    if (nl > 16 || !basis_route(p, &d, d.t_buf, 1).windowed) {
        amtx_set_error("amtx_cqt_track_layout: no clip form: the windowed basis kernel does not cover this plan (n_fft 128 or 256 on every level; "
                       "or a pyramid level of these %lld samples has fewer than 4)", (long long)num_samples);
        return AMTX_ERR_UNSUPPORTED;
    }
    AMTX_REQUIRE(d.t_out > 0, "amtx_cqt_track_layout: track too short for one frame");
    // amtx_cqt_forward's own condition: the deepest level reflects about its ends
    if (p->lib09) AMTX_REQUIRE(d.len.back() > p->pad, "amtx_cqt_track_layout: reflect padding needs a longer track (deepest level: %lld samples, pad %d)",
                               (long long)d.len.back(), p->pad);
    for (int l = 0; l < nl; ++l) {
        level_len[l] = d.len[l];
        level_stride[l] = (!p->lib09 && l == 0) ? 0 : d.stride[l];      // zero pads: level 0 is the audio, read in place
    }
    for (int h = 0; h < p->n_harm; ++h) rows_h[h] = d.frames_h[h];
    *frames = d.t_out;
    return nl;
}

extern "C" int amtx_cqt_pyramid_build(const amtx_cqt_plan* p, const float* audio, int64_t audio_elems, const int64_t* tracks_host,
                                      const int64_t* tracks, int num_tracks, float* pyramid, int64_t pyramid_elems, float* maxima, void* stream_) {
    AMTX_REQUIRE(p && audio && tracks_host && tracks && pyramid && maxima, "amtx_cqt_pyramid_build: null argument");
    AMTX_REQUIRE(num_tracks > 0 && num_tracks < 65536 && audio_elems > 0 && pyramid_elems > 0, "amtx_cqt_pyramid_build: bad num_tracks / buffer sizes");
    AMTX_REQUIRE(((uintptr_t)audio % 16) == 0 && ((uintptr_t)pyramid % 16) == 0, "amtx_cqt_pyramid_build: audio and pyramid must be 16-byte aligned");
    const int nl = (int)p->levels.size(), cols = pyr_cols(p);
    // the host table against the plan's own layout and the buffers: nothing below writes or reads outside what it describes
    int64_t audio_end = 0, pyr_end = 0, rows_max = 0;
    for (int t = 0; t < num_tracks; ++t) {
        const int64_t* tr = tracks_host + (int64_t)t * cols;
        int64_t len[16], stride[16], rows[16], frames = 0;
        AMTX_REQUIRE(tr[1] > 0, "amtx_cqt_pyramid_build: track %d has no samples", t);
        const int rc = amtx_cqt_track_layout(p, tr[1], len, stride, rows, &frames);
        if (rc < 0) return rc;
        AMTX_REQUIRE(tr[0] >= audio_end && tr[0] % 4 == 0 && tr[0] + tr[1] <= audio_elems, "amtx_cqt_pyramid_build: track %d: bad place in the audio buffer", t);
        audio_end = tr[0] + tr[1];
        int64_t rmax = 0;
        for (int h = 0; h < p->n_harm; ++h) {
            AMTX_REQUIRE(tr[4 + 3 * nl + h] == rows[h], "amtx_cqt_pyramid_build: track %d: rows of harmonic %d differ from the plan's", t, h);
            rmax = std::max(rmax, rows[h]);
        }
        AMTX_REQUIRE(tr[2] == rmax && tr[3] == frames, "amtx_cqt_pyramid_build: track %d: frame counts differ from the plan's", t);
        rows_max = std::max(rows_max, rmax);
        for (int l = 0; l < nl; ++l) {
            const int64_t* lv = tr + 4 + 3 * l;
            AMTX_REQUIRE(lv[1] == len[l] && lv[2] == stride[l], "amtx_cqt_pyramid_build: track %d: level %d differs from the plan's layout", t, l);
            AMTX_REQUIRE(lv[0] >= pyr_end && lv[0] % 4 == 0 && lv[0] + lv[2] <= pyramid_elems, "amtx_cqt_pyramid_build: track %d: bad place of level %d in the pyramid", t, l);
            pyr_end = lv[0] + lv[2];
        }
    }
    BasisRoute route;
    int rc = clips_check("amtx_cqt_pyramid_build", p, num_tracks, rows_max, route);
    if (rc != AMTX_OK) return rc;
    hipStream_t s = (hipStream_t)stream_;
    const bool zero_pads = !p->lib09;
    AMTX_CHECK_HIP(hipMemsetAsync(maxima, 0, sizeof(float) * num_tracks * p->n_harm, s));
    // the chain of amtx_cqt_forward on every track as a batch of one: the level signals are the whole-track forward's.  Zero pads: level 0 is
    // always the audio in place (a bank has no level-0 storage) and the maxima were reset above
    for (int t = 0; t < num_tracks; ++t) {
        const int64_t* tr = tracks_host + (int64_t)t * cols;
        rc = pyramid_chain(p, audio + tr[0], tr[1], tr[1], 1, zero_pads, zero_pads ? (float*)nullptr : maxima + (int64_t)t * p->n_harm,
                           [&](int l) { return PyrLevel{pyramid + tr[4 + 3 * l], tr[4 + 3 * l + 1], tr[4 + 3 * l + 2]}; }, s);
        if (rc != AMTX_OK) return rc;
    }
    // every track whole, no map: the maxima of each harmonic over its own rows
    return clips_basis(p, route, audio, pyramid, tracks, nullptr, num_tracks, rows_max, nullptr, maxima, s);
}

extern "C" int amtx_cqt_power_clips(const amtx_cqt_plan* p, const float* audio, const float* pyramid, const int64_t* tracks, const int64_t* desc,
                                    int batch, int64_t num_frames, float* power, void* stream_) {
    AMTX_REQUIRE(p && audio && pyramid && tracks && desc && power, "amtx_cqt_power_clips: null argument");
    BasisRoute route;
    const int rc = clips_check("amtx_cqt_power_clips", p, batch, num_frames, route);
    if (rc != AMTX_OK) return rc;
    return clips_basis(p, route, audio, pyramid, tracks, desc, batch, num_frames, power, nullptr, (hipStream_t)stream_);
}

extern "C" size_t amtx_cqt_clips_workspace_bytes(const amtx_cqt_plan* p, int batch, int64_t num_frames) {
    if (!p || batch <= 0 || num_frames <= 0) return 0;
    return ((size_t)batch * p->n_harm * p->n_bins * num_frames * 4 + 255) & ~(size_t)255;
}

extern "C" int amtx_cqt_clips(const amtx_cqt_plan* p, const float* audio, const float* pyramid, const int64_t* tracks, const int64_t* desc, int batch,
                              int64_t num_frames, const float* refs, int decibels, void* workspace, size_t workspace_bytes, float* out, void* stream_) {
    AMTX_REQUIRE(out, "amtx_cqt_clips: null argument");
    return clips_scaled("amtx_cqt_clips", p, audio, pyramid, tracks, desc, batch, num_frames, refs, decibels, workspace, workspace_bytes, out, nullptr, 0,
                        stream_);
}

extern "C" int amtx_cqt_clips16(const amtx_cqt_plan* p, const float* audio, const float* pyramid, const int64_t* tracks, const int64_t* desc, int batch,
                                int64_t num_frames, const float* refs, int decibels, void* workspace, size_t workspace_bytes, void* out16, void* stream_) {
    AMTX_REQUIRE(out16, "amtx_cqt_clips16: null argument");
    return clips_scaled("amtx_cqt_clips16", p, audio, pyramid, tracks, desc, batch, num_frames, refs, decibels, workspace, workspace_bytes, nullptr, out16,
                        0, stream_);
}

extern "C" int amtx_cqt_clips16_split(const amtx_cqt_plan* p, const float* audio, const float* pyramid, const int64_t* tracks, const int64_t* desc,
                                      int batch, int64_t num_frames, const float* refs, int decibels, void* workspace, size_t workspace_bytes,
                                      void* out16, int64_t plane_elems, void* stream_) {
    AMTX_REQUIRE(out16 && plane_elems > 0 && plane_elems % 8 == 0, "amtx_cqt_clips16_split: null argument / plane stride not a multiple of 8 elements");
    return clips_scaled("amtx_cqt_clips16_split", p, audio, pyramid, tracks, desc, batch, num_frames, refs, decibels, workspace, workspace_bytes, nullptr,
                        out16, plane_elems / 8, stream_);
}
