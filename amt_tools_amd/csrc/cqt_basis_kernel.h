// cqt_basis_kernel of cqt.hip, included there twice (not a header of its own: it uses that file's BasisArgs / BasisLevs / BasisClips and
// helpers).  CQT_BASIS_CLIPS 0: cqt_basis_kernel<KS>(BasisArgs, BasisLevs), a tile belongs to a batch index -- the kernel as it always was,
// name, arguments and instructions.  CQT_BASIS_CLIPS 1: cqt_basis_clips_kernel<KS>(BasisArgs, BasisLevs, BasisClips), a tile belongs to a clip
// descriptor (include/amtx_pyramid.h).  One text, because the two must compute a frame in the same way to the bit; two kernels and not
// one shared inline body, because hipcc compiles the whole-track kernel differently (1907 against 1982 lines of ISA) as soon as its body is
// a function called from two __global__ wrappers.
#if CQT_BASIS_CLIPS
template <int KS>
__global__ __launch_bounds__(256, 2) void cqt_basis_clips_kernel(BasisArgs a, BasisLevs ls, BasisClips cl) {
#else
template <int KS>
__global__ __launch_bounds__(256, 2) void cqt_basis_kernel(BasisArgs a, BasisLevs ls) {
#endif
    constexpr bool CLIPS = CQT_BASIS_CLIPS;
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [hi plane | lo plane] of the padded window, then 16 maxima
    constexpr int K = 32 * KS;
    // this block's level: the launch deals its blocks to the levels by their work (staged samples + a per-tile charge)
    int li = 0;
    while (li + 1 < ls.n && (int)blockIdx.x >= ls.b0[li + 1]) ++li;
    const BasisLevel& L = a.lev[ls.lev[li]];
    const int bid = (int)blockIdx.x - ls.b0[li], nblk = ls.b0[li + 1] - ls.b0[li];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // `hop` below is the frame stride of the STAGED copy: the level's hop, or K where the hop is larger (level 0, hop 512 > K = 256: rows do
    // not overlap and only the K samples of every frame are staged, back to back)
    const int ghop = L.hop, ft = L.ft;
    const int hop = min(ghop, K), lh = __builtin_ctz(hop);        // powers of two
    const int pad = bas_pad(hop);                                  // pad samples behind every `hop`
    const int ws = (ft - 1) * hop + K;                             // samples of a tile's window
    const int wsp = ws + pad * ((ws + hop - 1) / hop);             // ... in LDS
    const int plane = ((wsp + 7) & ~7) * 2;                        // bytes per plane
    unsigned* lmax = reinterpret_cast<unsigned*>(smem + 2 * plane);

    // ---- this wave's columns: two 16-column tiles per wave, four waves = one slice of 128 columns; waves beyond the slice's columns share
    // the frame tiles of a column group
    const int col0 = 128 * blockIdx.y;                             // first column of this slice
    if (col0 >= L.ncols) return;
    const int nct = (min(L.ncols - col0, 128) + 15) >> 4;          // 16-column tiles with real columns in the slice (<= 8)
    const int ncg = (nct + 1) >> 1;                                // column groups of two tiles (1 .. 4)
    const int wpg = 4 / ncg;                                       // waves per group (4, 2, 1, 1)
    const bool idle = wave >= ncg * wpg;
    const int cg = (idle ? 0 : wave % ncg) + 4 * blockIdx.y, sub = wave / ncg;
    const int g = lane >> 4, fl = lane & 15;
    uint4 wh[2][KS], wl[2][KS];
    {
        const int64_t wplane = (int64_t)L.n_pad * L.k_pad;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int n = min((2 * cg + c) * 16 + fl, L.n_pad - 1);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                wh[c][ks] = *reinterpret_cast<const uint4*>(L.w + (int64_t)n * L.k_pad + ks * 32 + 8 * g);
                wl[c][ks] = *reinterpret_cast<const uint4*>(L.w + wplane + (int64_t)n * L.k_pad + ks * 32 + 8 * g);
            }
        }
    }
    // pair maps of this lane's four columns per tile: columns n0 + 4 g + {0, 1} = (re, im) of one filter, + {2, 3} of the next
    int2 pm[2][2];
    bool pv[2][2];
    int rl[2][2], ro[2][2];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int n = (2 * cg + c) * 16 + 4 * g + 2 * h;
            pv[c][h] = !idle && n < L.ncols;
            pm[c][h] = L.map[min(n, L.ncols - 2) >> 1];
            // frames of this filter's harmonic (0: the lane's columns do not exist): read ONCE -- indexed per lane inside the frame loop it was
            // a memory round trip per filter and 16 frames
            // (the clip form has a limit per clip: set in the tile loop)
            rl[c][h] = !CLIPS && pv[c][h] ? a.rows[pm[c][h].y & 15] : 0;
            ro[c][h] = pm[c][h].x * (int)a.mag_pitch;            // row offset inside the clip's map
        }
    // byte offset of this lane's operand inside a frame's window: sample 8 g of k-step 0 (+ 32 samples per k-step), pads included
    auto soff = [&](int s) { return (s + pad * (s >> lh)) * 2; };
    // ... split for the matrix loop: frame f starts at byte f * fstride, k-step ks of this lane koff[ks] bytes further
    const int fstride = 2 * (hop + pad);
    int koff[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) koff[ks] = soff(ks * 32 + 8 * g);

    // ---- tile loop.  Staging: four samples per thread and step (a 16-byte load at any 4-byte boundary: clips of odd length in one buffer), in
    // ROUNDS of six steps whose loads are issued back to back from clamped addresses (a load -> test -> store loop pays one memory round
    // trip per step); what lies outside the signal is zeroed at the split.  Staged indices are multiples of 4 and so are the window origins,
    // so a group hangs over the signal's END only (by 1 - 3 samples when the length is not a multiple of 4): its values are picked out of
    // the clamped load by the distance it was moved.  The block's barriers wait for LDS traffic only (the stores of a tile's magnitudes
    // and the maxima's atomics stay in flight), and the other block of the CU covers a tile's load round trips.
    struct __attribute__((packed, aligned(4))) f32x4_a4 { float x, y, z, w; };
    constexpr int NST = 6, NSTF = 9;             // loads per round: the general path / a tile inside the signal (fewer temporaries: 36 registers of loads fit)
    const int ntile = L.tiles_per_clip * a.B;
    if (tid < 16) lmax[tid] = 0u;
#ifdef AMTX_CQT_TIMING
    unsigned long long bq_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, bq_t = __builtin_readcyclecounter();
#endif
    for (int tile = bid; tile < ntile; tile += nblk) {
        BQ_TICK(0);
        const int b = tile / L.tiles_per_clip, tt = tile - b * L.tiles_per_clip;
        const int f0 = tt * ft;                                    // first frame of the tile (clip form: counted from the clip's first)
        // clip form: the track's signal, the samples of it that exist, the window's first sample and the frames [0, cframes) to compute
        const float* csig = nullptr;
        int64_t clen = 0, cs0 = 0;
        int cframes = 0;
#if CQT_BASIS_CLIPS
        {
            // block-uniform table entries, read through pointers: kept out of the vector registers (the K = 256 kernel has four to spare)
            const int64_t* d = cl.desc ? cl.desc + 3 * (int64_t)b : nullptr;
            const int64_t* tr = cl.tab + uniform_i64(d ? d[0] : (int64_t)b) * cl.cols;
            const int first = d ? __builtin_amdgcn_readfirstlane((int)d[1]) : 0;
            const int nfr = __builtin_amdgcn_readfirstlane(d ? min((int)d[2], cl.num_frames) : (int)tr[2]);
            // rows beyond the clip's own frames are written as zeros; the maxima launch (no map) has nothing to do there
            cframes = a.mag ? cl.num_frames : nfr;
            if (f0 >= cframes) continue;                           // block-uniform, in front of the tile's barriers
            csig = L.sig + uniform_i64(tr[cl.base_col[ls.lev[li]]]);
            clen = uniform_i64(tr[cl.len_col[ls.lev[li]]]);
            cs0 = (int64_t)(first + f0) * ghop - K / 2 + L.off;
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int h = 0; h < 2; ++h)                        // rows of this filter that exist: the clip's, and its harmonic's in the track
                    rl[c][h] = pv[c][h] ? min(nfr, (int)tr[cl.rows_col + (pm[c][h].y & 15)] - first) : 0;
        }
#endif
        const float* sig = CLIPS ? csig : L.sig + (int64_t)b * L.sig_gs;
        const int64_t s0 = CLIPS ? cs0 : (int64_t)f0 * ghop - K / 2 + L.off;     // first sample of the window (index into sig)
        // samples of `sig` that exist, frames of the level: the whole-track form reads them where it uses them, as it always did
        auto slen = [&]() -> int64_t { if constexpr (CLIPS) return clen; else return L.len; };
        auto lframes = [&]() -> int { if constexpr (CLIPS) return cframes; else return L.frames; };
        // staged index i -> signal index: identity while the windows overlap, frame-wise (hop > K) otherwise
        auto sidx = [&](int i) { return s0 + (ghop > K ? (int64_t)(i >> lh) * ghop + (i & (hop - 1)) : (int64_t)i); };
        // a tile whose whole window lies inside the signal (all but a clip's first and last tiles): no clamping, no picking -- a third of the
        // instructions of the general case below (which was 37 % of the kernel's vector instructions)
        const int64_t s_end = s0 + (ghop > K ? (int64_t)(ft - 1) * ghop + K : (int64_t)ws);
        if (s0 >= 0 && s_end <= slen()) {
            const float* st = sig + s0;                            // wave-uniform base, 32-bit offsets per lane
            for (int base = 0; base < ws; base += 1024 * NSTF) {
                f32x4_a4 rr[NSTF];
#pragma unroll
                for (int n = 0; n < NSTF; ++n) {
                    const int i = min(base + 4 * tid + 1024 * n, ws - 4);
                    rr[n] = *reinterpret_cast<const f32x4_a4*>(st + (unsigned)(ghop > K ? (i >> lh) * ghop + (i & (hop - 1)) : i));
                }
#pragma unroll
                for (int n = 0; n < NSTF; ++n) {
                    const int i = base + 4 * tid + 1024 * n;
                    uint32_t h0, h1, l0, l1;
                    split_bf16x2(rr[n].x, rr[n].y, h0, l0);
                    split_bf16x2(rr[n].z, rr[n].w, h1, l1);
                    if (i < ws) {
                        const int o = soff(i);
                        *reinterpret_cast<uint2*>(smem + o) = make_uint2(h0, h1);
                        *reinterpret_cast<uint2*>(smem + plane + o) = make_uint2(l0, l1);
                    }
                }
            }
        } else
        for (int base = 0; base < ws; base += 1024 * NST) {
            f32x4_a4 rr[NST];
#pragma unroll
            for (int n = 0; n < NST; ++n) {
                const int64_t q = sidx(min(base + 4 * tid + 1024 * n, ws - 4));
                rr[n] = *reinterpret_cast<const f32x4_a4*>(sig + min(max(q, (int64_t)0), slen() - 4));
            }
#pragma unroll
            for (int n = 0; n < NST; ++n) {
                const int i = base + 4 * tid + 1024 * n;
                const int64_t q = sidx(min(i, ws - 4));
                // 0: as loaded; 1 - 3: the load was moved back by that much; 4: nothing of the group exists
                const int d = (q < 0 || q >= slen()) ? 4 : (int)(q - min(q, slen() - 4));
                const float r[4] = {rr[n].x, rr[n].y, rr[n].z, rr[n].w};
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    // element e of the group is element e + d of the load, if that exists
                    float x = r[e];
                    if (e + 1 < 4) x = d == 1 ? r[e + 1] : x;
                    if (e + 2 < 4) x = d == 2 ? r[e + 2] : x;
                    if (e + 3 < 4) x = d == 3 ? r[e + 3] : x;
                    v[e] = e + d < 4 ? x : 0.f;
                }
                uint32_t h0, h1, l0, l1;
                split_bf16x2(v[0], v[1], h0, l0);
                split_bf16x2(v[2], v[3], h1, l1);
                if (i < ws) {
                    const int o = soff(i);                         // four samples never straddle a pad (blocks are multiples of 4)
                    *reinterpret_cast<uint2*>(smem + o) = make_uint2(h0, h1);
                    *reinterpret_cast<uint2*>(smem + plane + o) = make_uint2(l0, l1);
                }
            }
        }
        BQ_TICK(1);
        lds_only_barrier();
        BQ_TICK(2);
        float mx[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
        const int nft = idle ? 0 : min(ft, lframes() - f0 + 15) >> 4;   // 16-frame tiles with real frames (a wave without columns has none)
        float* magb = a.mag + (int64_t)b * a.mag_gs;               // wave-uniform base, 32-bit offsets per lane (a clip's map is < 2^31 elements)
        // TWO 16-frame tiles per step: four independent accumulator chains and twice the reads in flight (one tile at a time, a wave waited for
        // every k-step's reads in front of its six dependent MFMAs)
        for (int q = sub; q < nft; q += 2 * wpg) {
            const int q2 = q + wpg < nft ? q + wpg : q;            // the second tile of the step (the first again when there is none: not stored)
            const int fr[2] = {q * 16 + fl, q2 * 16 + fl};         // this lane's frames inside the tile
            f32x4_t acc[2][2];
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int c = 0; c < 2; ++c) acc[u][c] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
            // operand reads run BAS_AHEAD k-steps ahead of the matrix instructions that use them, both pinned: left to itself hipcc reads a
            // k-step's four operands right in front of its twelve instructions (an LDS round trip per k-step, ~45 % on top of the matrix time)
            const int fbase[2] = {fr[0] * fstride, fr[1] * fstride};
            constexpr int NB = BAS_AHEAD + 1;              // operand sets in flight (a ring)
            uint4 ah[NB][2], al[NB][2];
            auto fetch = [&](int ks) {
                const int sl = ks % NB;
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int o = fbase[u] + koff[ks];
                    if (hop >= 8) {
                        ah[sl][u] = *reinterpret_cast<const uint4*>(smem + o);
                        al[sl][u] = *reinterpret_cast<const uint4*>(smem + plane + o);
                    } else {                                       // hop 4: windows start at 8-byte boundaries
                        const uint2 h0 = *reinterpret_cast<const uint2*>(smem + o), h1 = *reinterpret_cast<const uint2*>(smem + o + 8);
                        const uint2 l0 = *reinterpret_cast<const uint2*>(smem + plane + o), l1 = *reinterpret_cast<const uint2*>(smem + plane + o + 8);
                        ah[sl][u] = make_uint4(h0.x, h0.y, h1.x, h1.y);
                        al[sl][u] = make_uint4(l0.x, l0.y, l1.x, l1.y);
                    }
                }
            };
#pragma unroll
            for (int ks = 0; ks < BAS_AHEAD; ++ks) fetch(ks);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                if (ks + BAS_AHEAD < KS) fetch(ks + BAS_AHEAD);
                __builtin_amdgcn_sched_barrier(0);
                // per accumulator hi.hi, hi.lo, lo.hi (gemm_tile's order), the four accumulators taking turns
#pragma unroll
                for (int pr = 0; pr < 3; ++pr) {
#pragma unroll
                    for (int u = 0; u < 2; ++u)
#pragma unroll
                        for (int c = 0; c < 2; ++c)
                            acc[u][c] = mfma16(pr == 2 ? wl[c][ks] : wh[c][ks], pr == 1 ? al[ks % NB][u] : ah[ks % NB][u], acc[u][c]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (u == 1 && q2 == q) break;                      // wave-uniform
                const int m = f0 + fr[u];
#pragma unroll
                for (int c = 0; c < 2; ++c)
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        if constexpr (CLIPS) {
                            if (pv[c][h] && m < lframes()) {
                                const float re = acc[u][c][2 * h], im = acc[u][c][2 * h + 1];
                                // two rounded squares and their rounded sum, as the whole-track form below computes them (hipcc pairs its squares
                                // into v_pk_mul_f32 and adds; left to contract, this branch came out as a multiply and an fma: 8 % of a
                                // map one ulp away from the whole track's)
                                const float pw = power_unfused(re, im);
                                const float v = m < rl[c][h] ? pw : 0.f;
                                if (a.mag) magb[(unsigned)(ro[c][h] + m)] = v;
                                mx[c][h] = fmaxf(mx[c][h], v);
                            }
                        } else
                        if (m < rl[c][h]) {
                            const float re = acc[u][c][2 * h], im = acc[u][c][2 * h + 1];
                            const float v = re * re + im * im;           // power: the scaling kernels take its logarithm (or its root)
                            magb[(unsigned)(ro[c][h] + m)] = v;
                            mx[c][h] = fmaxf(mx[c][h], v);
                        }
                    }
            }
        }
        BQ_TICK(3);
        // per-(clip, harmonic) maxima: magnitudes are >= 0, so uint order == float order
        // the 16 lanes of a row (one lane group g) hold the same four filters: their maximum by DPP, one LDS atomic per row and filter (64
        // lanes on <= 6 addresses each were half of the kernel's LDS bank-conflict cycles)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const float m = row_max_f32(mx[c][h]);
                if (fl == 0 && m > 0.f) atomicMax(lmax + (pm[c][h].y & 15), __float_as_uint(m));
            }
        lds_only_barrier();                                        // everybody is done with the staged copy, the maxima are in
        if (tid < 16) {
            const unsigned v = lmax[tid];
            lmax[tid] = 0u;                                        // for the next tile (ordered behind its barrier)
            if (v != 0u && (!CLIPS || a.maxbuf)) atomicMax(reinterpret_cast<unsigned*>(a.maxbuf) + (int64_t)b * a.n_harm + tid, v);
        }
        BQ_TICK(4);
#ifdef AMTX_CQT_TIMING
        bq_acc[7] += 1;
#endif
    }
#ifdef AMTX_CQT_TIMING
    if (tid == 0)
        for (int i = 0; i < 8; ++i) atomicAdd(&g_bas_prof[i], bq_acc[i]);
#endif
}
