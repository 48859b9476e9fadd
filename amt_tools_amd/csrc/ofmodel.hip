// Onsets & Frames inference engine for gfx950: weight packing + the launch sequence of one
// `run_on_batch` forward (amt_tools/models/onsetsframes.py:94-136 forward, :138-196 post_proc without the
// loss; TranscriptionModel.run_on_batch amt_tools/models/common.py:151-184).
//
// Tensors are handed over under the reference's own state_dict names (e.g. "onset_head.0.layer2.0.weight"),
// eval-mode BatchNorm is folded, fc1's columns are permuted from the reference's (channel, freq) flatten
// order to the channels-last (freq, channel) order the conv kernels write, LSTM biases b_ih + b_hh are merged
// into the input-projection GEMM, everything is packed into MFMA fragment order once.
//
// Launch sequence (acoustic heads batched as kernel groups):
//   conv1 -> conv2+pool -> conv3+pool -> fc1            [groups = heads: onset, (offset), pitch]
//   onset(/offset) x-proj GEMM -> BiLSTM -> head GEMM -> joint[:, 0:88(:176)]
//   pitch head GEMM -> joint[:, 88:176]
//   adjoin x-proj GEMM (A = joint logits, fp32) -> BiLSTM -> head GEMM -> frame logits
//   piano-roll finalize (sigmoid, threshold 0.5, transpose) x2

#include "amtx_kernels.h"
#include "amtx_model_common.h"
#include "amtx_pack_layouts.h"
#include "../../include/amtx_ofseq.h"

#include <cmath>
#include <cstdlib>
#include <thread>

namespace {

struct LinearPack { DevBuf w, b; int N = 0, K = 0, n_pad = 0, k_pad = 0, groups = 0; };     // w: [groups][planes][n_pad][k_pad], b: [groups][N]

// The kernels and packers that exist once per 16-bit operand format (amtx_kernels_fmt.h): member `name` of a KernelSet is amtx_`name` of one
// format namespace, its type the declaration's.  Struct and tables come from this one list, so a name that either namespace lacks does
// not compile.  A model picks its table when it is created and calls through it.
#define AMTX_FMT_KERNELS(X, ns)                                                                                                    \
    X(ns, pack_linear_host) X(ns, bilstm_pack_host) X(ns, conv1_pack_host) X(ns, conv1g_pack_host) X(ns, conv3x3_pack_host)     \
    X(ns, conv3x3_gen_pack_host) X(ns, pack_conv1_dev) X(ns, pack_conv1g_dev) X(ns, pack_conv3x3_dev) X(ns, pack_conv_gen_dev)    \
    X(ns, pack_linear_dev) X(ns, launch_bilstm_pack_dev) X(ns, launch_conv1) X(ns, launch_conv3x3) X(ns, launch_conv3x3_gen)    \
    X(ns, launch_conv_stack) X(ns, launch_gemm) X(ns, launch_bilstm) X(ns, launch_bilstm_seq)
#define AMTX_KERNEL_FIELD(ns, name) decltype(&ns::amtx_##name) name;
#define AMTX_KERNEL_ENTRY(ns, name) &ns::amtx_##name,
struct KernelSet { AMTX_FMT_KERNELS(AMTX_KERNEL_FIELD, amtx_bf16) };
const KernelSet kKernelsBf16 = {AMTX_FMT_KERNELS(AMTX_KERNEL_ENTRY, amtx_bf16)};
#ifdef AMTX_WITH_F16
const KernelSet kKernelsF16 = {AMTX_FMT_KERNELS(AMTX_KERNEL_ENTRY, amtx_f16)};
#endif

// Which convolution kernels a model runs.  make_conv_plan decides it once, when the model is created; resolve_conv adds what depends on
// the call.  Packing, workspace carving, the forward pass and the query entry points only read the two (table: DESIGN.md).
enum ConvFamily { K_CONV1,      // conv.hip's separate first conv (fp32 weights): only where the first conv cannot be fused into conv2
                  K_CONV,       // conv.hip: 32 / 32 / 64 channels, weights stationary in registers (two planes: with convx.hip behind the same launcher)
                  K_CONVG };    // convg.hip: the general kernel, weights in LDS
struct ConvLayer { const char* name; int c_in, c_out; ConvFamily fam; size_t frag_per; };   // frag_per: packed 16-bit weight elements per head

// the A/B switches of this file (switch table), all read here, once per model
struct ConvSwitches { bool no_convg_mc2, no_conv_fuse, x3_no_split, no_convx12m, rowmajor_a3, no_roll_epilogue; };
ConvSwitches switches_from_env() {
    auto on = [](const char* name) { return getenv(name) != nullptr; };
    return {on("AMTX_NO_CONVG_MC2"), on("AMTX_NO_CONV_FUSE"), on("AMTX_X3_NO_SPLIT"), on("AMTX_NO_CONVX12M"), on("AMTX_OF_ROWMAJOR_A3"), on("AMTX_OF_NO_ROLL_EPILOGUE")};
}

struct ConvPlan {
    ConvLayer layer[3];         // layer1 .. layer3 of every acoustic head
    bool conv1_fused;           // the first conv runs inside the conv2 kernel (layer[0].fam == layer[1].fam), a1 never exists
    bool stack;                 // eligible for layer1 -> layer2 -> layer3 in one kernel (convf.hip); batches that fill the chip with strips take it
    bool two_plane_acts;        // x3 (round 5): activations in HBM as two 16-bit planes (AMTX_T_SPLIT) from conv2 on; the GEMMs DMA them straight into LDS
    bool convx12; size_t c2x_per;   // round 6: conv1 + conv2 from two-plane 16-bit features on convx.hip; it reads a second copy of layer2's weights (conv2_wx, c2x_per per head)
    bool rowmajor_a3, no_roll_epilogue;   // A/B: the fused stack's output row-major; piano rolls / refinement input from separate kernels
    bool device_resync;         // amtx_of_model_finalize_device has a packer for every layer
    int fuses_db_scale, takes_feats16;   // the answers of amtx_of_fuses_db_scale / amtx_of_takes_feats16 once the model is finalized (feats16 = 2:
                                         // convx12's two planes [2][B][T][F][8], the lo plane B T F 8 elements behind the hi plane, amtx_cqt_forward16_split)
};

ConvPlan make_conv_plan(int in_channels, int model_complexity, int precision, const ConvSwitches& sw) {
    const int ic = in_channels, nf1 = 16 * model_complexity, nf3 = 2 * nf1, pl = precision == AMTX_PREC_X3 ? 2 : 1;
    ConvPlan p{};
    // channel counts other than 32 / 32 / 64: convg.hip throughout.  32 / 32 / 64 with more than one input channel (HCQT): conv.hip's fused first
    // conv runs its 9 c_in taps as four legacy 16-deep MFMA steps and stages c_in x 20 x (columns + 4) feature values per tile through a
    // register-starved loop (3.6 ms per 512 HCQT clips); convg.hip's fused first conv (two 32-deep steps, weights in LDS) is the faster one there
    // (2.7 ms).  With one input channel conv.hip stays far ahead: 5.6 vs 9.7 ms per 1024 mel clips (weights stationary in registers, 18 x 46 tiles).
    const ConvFamily f3 = nf1 != 32 ? K_CONVG : K_CONV;
    const bool g_fuse1 = amtx_conv3x3_gen_can_fuse1(ic, nf1, nf1, pl);
    const ConvFamily f2 = f3 == K_CONVG || (ic > 1 && !sw.no_convg_mc2 && g_fuse1) ? K_CONVG : K_CONV;
    p.conv1_fused = f2 == K_CONVG ? g_fuse1 : 9 * ic <= 64;
    auto frag3x3 = [pl](ConvFamily f, int c_in, int c_out) { return f == K_CONVG ? amtx_conv3x3_gen_wfrag_elems(c_in, c_out, pl) : amtx_conv3x3_wfrag_elems(c_out, pl); };
    p.layer[0] = {"layer1", ic, nf1, p.conv1_fused ? f2 : K_CONV1,
                  !p.conv1_fused ? 0 : f2 == K_CONVG ? amtx_conv1g_wfrag_elems(ic, nf1, pl) : amtx_conv1_wfrag_elems(ic, pl)};
    p.layer[1] = {"layer2", nf1, nf1, f2, frag3x3(f2, nf1, nf1)};
    p.layer[2] = {"layer3", nf1, nf3, f3, frag3x3(f3, nf1, nf3)};
    p.stack = f2 == K_CONV && p.conv1_fused && ic == 1 && pl == 1 && !sw.no_conv_fuse;
    // one input channel: conv.hip / convx.hip write the planes; 2 .. 7 input channels at 32 / 32 / 64 channels -- HCQT --: convg.hip's
    // two-plane kernel writes a2 as planes, convx.hip's conv3 and the GEMMs behind it are the same
    p.two_plane_acts = pl == 2 && f3 == K_CONV && p.conv1_fused && !sw.x3_no_split && (f2 == K_CONV ? ic == 1 : ic > 1 && (9 * ic + 31) / 32 <= 2);
    p.convx12 = p.two_plane_acts && f2 == K_CONVG && ic >= 2 && ic <= 8 && amtx_conv1g_tapk(ic, 2) && !sw.no_convx12m;
    p.c2x_per = frag3x3(K_CONV, nf1, nf1);
    p.rowmajor_a3 = sw.rowmajor_a3; p.no_roll_epilogue = sw.no_roll_epilogue;
    p.device_resync = f2 == K_CONVG || ic == 1;          // no device packer for conv.hip's multi-channel first conv (AMTX_NO_CONVG_MC2, or 9 and more channels)
    p.fuses_db_scale = p.conv1_fused && f2 == K_CONV && ic == 1;
    p.takes_feats16 = !(p.conv1_fused && f2 == K_CONVG && precision != AMTX_PREC_F16) ? 0 : p.convx12 ? 2 : pl == 1 && nf1 == 32 && amtx_conv1g_tapk(ic, pl);
    return p;
}

}  // namespace

struct amtx_of_model {
    int dim_in, in_channels, mc, n_out, has_offsets, precision;
    int planes, act_type;
    bool f16 = false;                          // AMTX_PREC_F16: weights and 16-bit activations are IEEE half
    const KernelSet* k = &kKernelsBf16;        // the kernels of this model's 16-bit operand format (f16: the half-operand twins)
    int nf1, nf2, nf3, dim_am, dim_lm, fq, kfc;
    int kfc_pad;                               // fc1's K rounded up to the DMA GEMM's 64-deep k-tile (rows of a3 are this long)
    int hid, xw;                               // LSTM hidden size per direction, width of an x-projection row (2 dirs x 4 gates x hid)
    size_t hh_elems;                           // packed W_hh elements of one BiLSTM
    ConvPlan plan;                             // which convolution kernels this model runs
    int n_heads;                               // acoustic heads: onset, (offset), pitch
    int n_rec;                                 // recurrent heads feeding the joint: onset, (offset)
    std::vector<std::string> head_names;       // state_dict prefixes of the acoustic models, group order
    TensorStore store{"of_model", "was not provided"};   // amtx_of_model_set_tensor / _set_tensor_device
    DevBuf pack_scratch;                       // device re-sync: BatchNorm scale / shift, the folded pitch head, the unused backward LSTM fragments
    bool finalized = false;
    bool packed_once = false;                  // the packed buffers hold a weight version that forwards may still be reading
    // packed device weights (group-major)
    DevBuf conv_w[3], conv_s[3];               // per conv layer: fragments (layer1: only when fused into conv2), fp32 shifts
    DevBuf conv1_w;                            // layer1's weights in fp32, BatchNorm scale folded in: the separate first conv reads them
    DevBuf conv2_wx;                           // convx12: layer2's weights a second time, in conv.hip's fragment order (convx12_kernel<true> reads them)
    LinearPack fc1;                            // groups = n_heads
    LinearPack rec_ih;                         // groups = n_rec, N = 1024
    DevBuf rec_hh;                             // groups = n_rec
    LinearPack rec_out;                        // groups = n_rec, N = n_out, K = dim_lm
    LinearPack pitch_out;                      // the pitch head's fc1 and LogisticBank folded into one layer: K = kfc_pad, N = n_out
    LinearPack adj_ih;                         // K = dim_aj, N = 1024
    DevBuf adj_hh;
    LinearPack adj_out;
    int dim_aj;
    // optional per-stage timing with HIP events recorded on the launch stream (bench.py roofline)
    mutable bool prof = false;
    mutable std::vector<std::vector<hipEvent_t>> prof_events;
};

enum { ST_CONV1 = 0, ST_CONV2, ST_CONV3, ST_FC1, ST_REC_XPROJ, ST_REC_LSTM, ST_REC_HEAD, ST_PITCH_HEAD, ST_ADJ_XPROJ, ST_ADJ_LSTM,
       ST_ADJ_HEAD, ST_PIANOROLL, ST_COUNT };
static const char* kStageNames[ST_COUNT] = {"conv1", "conv2_pool", "conv3_pool", "fc1_gemm", "rec_xproj_gemm", "rec_bilstm", "rec_head_gemm",
                                            "pitch_head_gemm", "adj_xproj_gemm", "adj_bilstm", "adj_head_gemm", "pianoroll"};

namespace {

struct Workspace {
    char *a1, *a2, *a3, *e, *xp, *l1, *joint, *joint16, *xp2, *l2, *mp;
    size_t total;
};

// What one call launches for conv1 + conv2 (conv3 follows on layer3's family unless the fused stack has covered it).  carve and the
// forward pass both ask here, so the workspace and the launches cannot disagree.
enum ConvPath { PATH_STACK,                  // convf.hip: all three layers in one kernel, neither intermediate map reaches HBM
                PATH_CONVX12,                   // convx.hip: conv1 + conv2 from two-plane 16-bit features
                PATH_CONV12, PATH_CONVG12,   // conv1 inside the conv2 kernel of conv.hip / convg.hip
                PATH_CONV1 };                // conv.hip's separate first conv, then conv2 on layer2's family
struct ConvCall { ConvPath path; bool a2_in_hbm; int64_t a3_plane; };

ConvCall resolve_conv(const amtx_of_model* m, int B, int T, bool feats16) {
    const ConvPlan& p = m->plan;
    if (p.stack && amtx_conv_stack_fused_ok(B, T, m->dim_in, m->n_heads))
        // output in planes of 64 channels per pooled frequency column ([F / 4][B T][64]): a k-tile of the GEMMs that read it is contiguous memory
        return {PATH_STACK, false, p.rowmajor_a3 ? 0 : (int64_t)B * T * 64};
    return {feats16 && p.convx12 ? PATH_CONVX12 : !p.conv1_fused ? PATH_CONV1 : p.layer[1].fam == K_CONVG ? PATH_CONVG12 : PATH_CONV12, true, 0};
}

Workspace carve(const amtx_of_model* m, int B, int T, char* base) {
    Workspace w;
    const size_t es = amtx_tsize(m->act_type);
    const size_t BT = (size_t)B * T;
    const int F = m->dim_in, F2 = F / 2;
    WorkspaceCarver ws{base};
    w.a1 = ws.take(m->plan.conv1_fused ? 256 : BT * F * m->nf1 * es * m->n_heads);
    w.a2 = ws.take(resolve_conv(m, B, T, false).a2_in_hbm ? BT * F2 * m->nf2 * es * m->n_heads : 256);
    w.a3 = ws.take(BT * m->kfc_pad * es * m->n_heads);
    w.e = ws.take(BT * m->dim_am * es * m->n_heads);
    w.xp = ws.take(BT * m->xw * es * m->n_rec);
    w.l1 = ws.take(BT * m->dim_lm * es * m->n_rec);
    w.joint = ws.take(BT * m->dim_aj * sizeof(float));
    w.joint16 = ws.take(BT * (size_t)((m->dim_aj + 63) / 64 * 64) * 2 * (m->plan.two_plane_acts ? 2 : 1));   // bf16 copy (two planes with two_plane_acts), K padded to the GEMM's 64-deep k-tile
    w.xp2 = ws.take(BT * m->xw * es);
    w.l2 = ws.take(BT * m->dim_lm * es);
    w.mp = ws.take(BT * m->n_out * sizeof(float));
    w.total = ws.off;
    return w;
}

}  // namespace

// 1 when the half-operand twins of conv / convf / convg / gemm / lstm / pack.hip are linked in (precision AMTX_PREC_F16 available)
extern "C" int amtx_has_f16(void) {
#ifdef AMTX_WITH_F16
    return 1;
#else
    return 0;
#endif
}

extern "C" int amtx_of_model_create(amtx_of_model** out, int dim_in, int in_channels, int model_complexity, int n_out,
                                    int has_offsets, int precision) {
    AMTX_REQUIRE(out, "amtx_of_model_create: null model pointer");
    *out = nullptr;
    AMTX_REQUIRE(precision == AMTX_PREC_BF16 || precision == AMTX_PREC_X3 || precision == AMTX_PREC_F16, "amtx_of_model_create: bad precision");
    AMTX_REQUIRE(dim_in >= 4 && in_channels >= 1 && n_out > 0 && n_out % 4 == 0, "amtx_of_model_create: bad dims");
    if (precision == AMTX_PREC_F16 && !amtx_has_f16()) {
        amtx_set_error("amtx_of_model_create: precision f16 needs a library built with the half-operand kernel twins (AMTX_BUILD_F16=1 python -m amt_tools_amd.build)");
        return AMTX_ERR_UNSUPPORTED;
    }
    if (model_complexity < 2 || model_complexity > 5) {
        amtx_set_error("amtx_of_model_create: model_complexity 2 (32/32/64-channel convolutions, LSTM hidden 128), 3 (48/48/96, hidden 256) and "
                       "4 (64/64/128, hidden 384), 5 (80/80/160, hidden 512) are implemented, with or without the OnsetsFrames2 offset head (got model_complexity=%d)", model_complexity);
        return AMTX_ERR_UNSUPPORTED;
    }
    amtx_of_model* m = new amtx_of_model();
    m->dim_in = dim_in; m->in_channels = in_channels; m->mc = model_complexity; m->n_out = n_out;
    m->has_offsets = has_offsets; m->precision = precision;
    m->planes = precision == AMTX_PREC_X3 ? 2 : 1;
    m->act_type = precision == AMTX_PREC_X3 ? AMTX_T_F32 : AMTX_T_BF16;      // AMTX_T_BF16 = "16-bit operand format": half in the f16 mode
    m->f16 = precision == AMTX_PREC_F16;
#ifdef AMTX_WITH_F16
    if (m->f16) m->k = &kKernelsF16;
#endif
    m->nf1 = 16 * model_complexity; m->nf2 = m->nf1; m->nf3 = 32 * model_complexity;
    m->dim_am = 256 * model_complexity; m->dim_lm = 256 * (model_complexity - 1);
    m->fq = dim_in / 4;                      // two MaxPool(1,2): floor(floor(F/2)/2) == F//4
    m->kfc = m->nf3 * m->fq;
    m->kfc_pad = (m->kfc + 63) / 64 * 64;
    m->hid = m->dim_lm / 2; m->xw = 8 * m->hid;
    m->hh_elems = amtx_bilstm_wfrag_elems(m->hid, m->planes);
    m->plan = make_conv_plan(in_channels, model_complexity, precision, switches_from_env());
    m->head_names = {"onset_head"};
    if (has_offsets) m->head_names.push_back("offset_head");
    m->n_rec = (int)m->head_names.size();
    m->head_names.push_back("pitch_head");
    m->n_heads = (int)m->head_names.size();
    m->dim_aj = (m->n_rec + 1) * n_out;
    *out = m;
    return AMTX_OK;
}

extern "C" int amtx_of_model_destroy(amtx_of_model* m) {
    if (!m) return AMTX_OK;
    DevBuf* bufs[] = {&m->conv1_w, &m->conv_w[0], &m->conv_w[1], &m->conv_w[2], &m->conv_s[0], &m->conv_s[1], &m->conv_s[2], &m->conv2_wx, &m->fc1.w, &m->fc1.b,
                      &m->rec_ih.w, &m->rec_ih.b, &m->rec_hh, &m->rec_out.w, &m->rec_out.b, &m->pitch_out.w, &m->pitch_out.b,
                      &m->adj_ih.w, &m->adj_ih.b, &m->adj_hh, &m->adj_out.w, &m->adj_out.b, &m->pack_scratch};
    for (DevBuf* b : bufs) b->release();
    delete m;
    return AMTX_OK;
}

extern "C" int amtx_of_model_set_tensor(amtx_of_model* m, const char* name, const float* host_data, int64_t numel) {
    AMTX_REQUIRE(m && name && host_data && numel > 0, "amtx_of_model_set_tensor: bad argument");
    m->store.set(name, host_data, numel);
    m->finalized = false;
    return AMTX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Weight sync.  pack_model is the ONE walk over the state_dict: per head and stage, which tensors are needed (name, element count),
// which layout or fold applies, and where in which packed buffer the result goes.  An executor does the steps.  HostPack
// (amtx_of_model_finalize; the first sync, it sizes and allocates the buffers) runs the host packers on the host copies into staging
// images of the buffers, which are then uploaded.  DevicePack (amtx_of_model_finalize_device) launches the kernels of pack.hip on
// borrowed device tensors into the buffers themselves.  Both loop over the layouts of amtx_pack_layouts.h: the same bits.
namespace {

struct HostPack {
    amtx_of_model* m;
    std::map<DevBuf*, std::vector<char>> image;        // staging images of the packed buffers
    std::vector<float> scratch_;

    int need(const std::string& name, size_t numel, const float** p) { return m->store.need(name, numel, p); }
    template <class T> T* dst(DevBuf& b, size_t elems) {
        std::vector<char>& v = image[&b];
        v.resize(elems * sizeof(T));
        return (T*)v.data();
    }
    int scratch(size_t floats, float** p) { scratch_.resize(floats); *p = scratch_.data(); return AMTX_OK; }
    int bn_fold(const float* cb, const float* g, const float* be, const float* mu, const float* var, int c_out, float* scale, float* shift) {
        for (int c = 0; c < c_out; ++c) amtx_bn_fold(cb, g, be, mu, var, c, scale, shift);
        return AMTX_OK;
    }
    int scale_rows(const float* w, const float* scale, int rows, int cols, float* out) {
        for (int item = 0; item < rows * cols; ++item) amtx_layout_scale_rows(item, w, scale, cols, out);
        return AMTX_OK;
    }
    int conv1(const float* w, const float* scale, int c_in, bf16_t* out) { m->k->conv1_pack_host(w, scale, c_in, m->planes, out); return AMTX_OK; }
    int conv1g(const float* w, const float* scale, int c_in, int c_mid, bf16_t* out) { m->k->conv1g_pack_host(w, scale, c_in, c_mid, m->planes, out); return AMTX_OK; }
    int conv3x3(const float* w, const float* scale, int c_out, bf16_t* out) { m->k->conv3x3_pack_host(w, scale, c_out, m->planes, out); return AMTX_OK; }
    int conv_gen(const float* w, const float* scale, int c_in, int c_out, bf16_t* out) { m->k->conv3x3_gen_pack_host(w, scale, c_in, c_out, m->planes, out); return AMTX_OK; }
    int linear(const float* W, int64_t ldw, int N, int K, const LinearPack& lp, int row0, int rows, int perm_c, int perm_f, bf16_t* out) {
        m->k->pack_linear_host(W, ldw, N, K, m->planes, lp.n_pad, lp.k_pad, row0, rows, perm_c, perm_f, out);
        return AMTX_OK;
    }
    int vec_add(const float* a, const float* b, int n, float* out) { for (int i = 0; i < n; ++i) out[i] = a[i] + b[i]; return AMTX_OK; }
    int copy(float* out, const float* src, size_t n) { memcpy(out, src, n * sizeof(float)); return AMTX_OK; }
    int bilstm(const float* whh_fwd, const float* whh_bwd, bf16_t* out) { m->k->bilstm_pack_host(whh_fwd, whh_bwd, m->hid, m->planes, out); return AMTX_OK; }
    // The ONE step with a loop structure of its own: n_out x dim_am x kfc double multiply-adds (164 M at model_complexity 2) would be
    // many times slower on a CPU one output element at a time, as head_fold_kernel (pack.hip) does them.  Output rows are dealt to a few
    // host threads; a row is accumulated over W_fc1's rows in W_fc1's own, contiguous column order and permuted when it is written.
    // What the two share: the column map amtx_fc1_col and the summation order, j ascending per element (the result does not depend on
    // the thread count).
    int head_fold(const float* w_out, const float* w_fc1, const float* b_fc1, const float* b_out, float* wfold, float* bfold) {
        const int n_out = m->n_out, dim_am = m->dim_am, kfc = m->kfc, kfc_pad = m->kfc_pad, nf3 = m->nf3, fq = m->fq;
        auto fold_rows = [=](int o0, int o1) {
            std::vector<double> rowacc(kfc);
            for (int o = o0; o < o1; ++o) {
                std::fill(rowacc.begin(), rowacc.end(), 0.0);
                double bacc = b_out[o];
                for (int j = 0; j < dim_am; ++j) {
                    const double wo = w_out[(size_t)o * dim_am + j];
                    const float* frow = w_fc1 + (size_t)j * kfc;
                    for (int ks = 0; ks < kfc; ++ks) rowacc[ks] += wo * frow[ks];
                    bacc += wo * b_fc1[j];
                }
                for (int k = 0; k < kfc_pad; ++k) wfold[(size_t)o * kfc_pad + k] = k < kfc ? (float)rowacc[amtx_fc1_col(k, nf3, fq)] : 0.0f;
                bfold[o] = (float)bacc;
            }
        };
        const int nthreads = (int)std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
        std::vector<std::thread> pool;
        const int per = (n_out + nthreads - 1) / nthreads;
        for (int t = 1; t < nthreads; ++t)
            if (t * per < n_out) pool.emplace_back(fold_rows, t * per, std::min(n_out, (t + 1) * per));
        fold_rows(0, std::min(n_out, per));
        for (auto& th : pool) th.join();
        return AMTX_OK;
    }
};

// `dry`: look up and size-check every tensor, launch nothing -- amtx_of_model_finalize_device runs this pass first, so a missing or
// mis-sized tensor is reported before a single packed buffer has been touched (the buffers never end up half new, half old).
struct DevicePack {
    amtx_of_model* m;
    hipStream_t s;
    bool dry;

    int need(const std::string& name, size_t numel, const float** p) { return m->store.need_device(name, numel, p); }
    template <class T> T* dst(DevBuf& b, size_t) { return (T*)b.p; }
    // behind the walk's floats: the backward LSTM fragments (written by the shared pack kernel, not used by inference)
    bf16_t* hh_bwd = nullptr;
    int scratch(size_t floats, float** p) {
        const size_t bytes = floats * sizeof(float) + m->hh_elems * sizeof(bf16_t) + 256;
        if (!m->pack_scratch.p || m->pack_scratch.bytes < bytes) {
            m->pack_scratch.release();
            AMTX_CHECK_HIP(hipMalloc(&m->pack_scratch.p, bytes));
            m->pack_scratch.bytes = bytes;
        }
        *p = (float*)m->pack_scratch.p;
        hh_bwd = (bf16_t*)(((uintptr_t)(*p + floats) + 255) & ~(uintptr_t)255);
        return AMTX_OK;
    }
    int bn_fold(const float* cb, const float* g, const float* be, const float* mu, const float* var, int c_out, float* scale, float* shift) {
        return dry ? AMTX_OK : amtx_pack_bn_fold_dev(cb, g, be, mu, var, c_out, scale, shift, s);
    }
    int scale_rows(const float* w, const float* scale, int rows, int cols, float* out) { return dry ? AMTX_OK : amtx_pack_scale_rows_dev(w, scale, rows, cols, out, s); }
    int conv1(const float* w, const float* scale, int c_in, bf16_t* out) {
        AMTX_REQUIRE(c_in == 1, "amtx_of_model_finalize_device: internal: no device packer for a multi-channel first conv on conv.hip");
        return dry ? AMTX_OK : m->k->pack_conv1_dev(w, scale, m->planes, out, s);
    }
    int conv1g(const float* w, const float* scale, int c_in, int c_mid, bf16_t* out) { return dry ? AMTX_OK : m->k->pack_conv1g_dev(w, scale, c_in, c_mid, m->planes, out, s); }
    int conv3x3(const float* w, const float* scale, int c_out, bf16_t* out) { return dry ? AMTX_OK : m->k->pack_conv3x3_dev(w, scale, c_out, m->planes, out, s); }
    int conv_gen(const float* w, const float* scale, int c_in, int c_out, bf16_t* out) {
        return dry ? AMTX_OK : m->k->pack_conv_gen_dev(w, scale, c_in, c_out, amtx_conv3x3_gen_ntc(c_in, c_out), m->planes, out, s);
    }
    int linear(const float* W, int64_t ldw, int N, int K, const LinearPack& lp, int row0, int rows, int perm_c, int perm_f, bf16_t* out) {
        return dry ? AMTX_OK : m->k->pack_linear_dev(W, ldw, N, K, m->planes, lp.n_pad, lp.k_pad, row0, rows, perm_c, perm_f, out, s);
    }
    int vec_add(const float* a, const float* b, int n, float* out) { return dry ? AMTX_OK : amtx_pack_vec_add_dev(a, b, n, out, s); }
    int copy(float* out, const float* src, size_t n) {
        if (!dry) AMTX_CHECK_HIP(hipMemcpyAsync(out, src, n * sizeof(float), hipMemcpyDeviceToDevice, s));
        return AMTX_OK;
    }
    int bilstm(const float* whh_fwd, const float* whh_bwd, bf16_t* out) {
        return dry ? AMTX_OK : m->k->launch_bilstm_pack_dev(whh_fwd, whh_bwd, m->hid, m->planes, out, hh_bwd, s);
    }
    int head_fold(const float* w_out, const float* w_fc1, const float* b_fc1, const float* b_out, float* wfold, float* bfold) {
        return dry ? AMTX_OK : amtx_pack_head_fold_dev(w_out, w_fc1, b_fc1, b_out, m->n_out, m->dim_am, m->kfc, m->kfc_pad, m->nf3, m->fq, wfold, bfold, s);
    }
};

#define NEED(name, numel, ptr)                                         \
    do {                                                               \
        int _rc = x.need(name, numel, &(ptr));                         \
        if (_rc != AMTX_OK) return _rc;                                \
    } while (0)
#define STEP(expr)                                                     \
    do {                                                               \
        int _rc = (expr);                                              \
        if (_rc != AMTX_OK) return _rc;                                \
    } while (0)

template <class X>
int pack_model(amtx_of_model* m, X& x) {
    const int nh = m->n_heads, pl = m->planes, G = 4 * m->hid, ic = m->in_channels;
    const ConvPlan& p = m->plan;
    auto size_linear = [](LinearPack& lp, int N, int K, int groups) {
        lp.N = N; lp.K = K; lp.groups = groups;
        amtx_gemm_pack_dims(N, K, &lp.n_pad, &lp.k_pad);
    };
    size_linear(m->fc1, m->dim_am, m->kfc_pad, m->n_rec);
    size_linear(m->rec_ih, m->xw, m->dim_am, m->n_rec);
    size_linear(m->rec_out, m->n_out, m->dim_lm, m->n_rec);
    size_linear(m->pitch_out, m->n_out, m->kfc_pad, 1);
    size_linear(m->adj_ih, m->xw, m->dim_aj, 1);
    size_linear(m->adj_out, m->n_out, m->dim_lm, 1);
    // rows [row0, row0 + rows) of group grp of a Linear layer's packed weights, from W (N x K); its bias
    auto linear = [&](LinearPack& lp, int grp, const float* W, int N, int K, int row0, int rows, int perm_c, int perm_f) {
        const size_t per = (size_t)lp.n_pad * lp.k_pad * pl;
        return x.linear(W, K, N, K, lp, row0, rows, perm_c, perm_f, x.template dst<bf16_t>(lp.w, per * lp.groups) + per * grp);
    };
    auto bias = [&](LinearPack& lp, int grp) { return x.template dst<float>(lp.b, (size_t)lp.N * lp.groups) + (size_t)lp.N * grp; };
    auto need_fc1 = [&](int h, const float*& w, const float*& b) {
        NEED(m->head_names[h] + ".0.fc1.0.weight", (size_t)m->dim_am * m->kfc, w);
        NEED(m->head_names[h] + ".0.fc1.0.bias", (size_t)m->dim_am, b);
        return (int)AMTX_OK;
    };
    auto need_bank = [&](const std::string& bank, int K, const float*& w, const float*& b) {
        NEED(bank + ".output_layer.weight", (size_t)m->n_out * K, w);
        NEED(bank + ".output_layer.bias", (size_t)m->n_out, b);
        return (int)AMTX_OK;
    };
    // scratch: BatchNorm scale[256] | folded pitch head (n_out x kfc_pad) | folded bias
    AMTX_REQUIRE(m->nf3 <= 256, "of_model: internal: scale scratch");
    float* scale;
    STEP(x.scratch(256 + (size_t)m->n_out * m->kfc_pad + m->n_out, &scale));
    float* wfold = scale + 256;
    float* bfold = wfold + (size_t)m->n_out * m->kfc_pad;

    // ---- acoustic heads
    for (int h = 0; h < nh; ++h) {
        const std::string am = m->head_names[h] + ".0";
        const float *w, *cb, *g, *be, *mu, *var;
        for (int l = 0; l < 3; ++l) {
            // Conv + eval-mode BatchNorm: the scale goes into the packed weights, the shift stays fp32
            const ConvLayer& y = p.layer[l];
            const std::string conv = am + "." + y.name + ".0", bn = am + "." + y.name + ".1";
            NEED(conv + ".weight", (size_t)y.c_out * y.c_in * 9, w);
            NEED(conv + ".bias", (size_t)y.c_out, cb); NEED(bn + ".weight", (size_t)y.c_out, g); NEED(bn + ".bias", (size_t)y.c_out, be);
            NEED(bn + ".running_mean", (size_t)y.c_out, mu); NEED(bn + ".running_var", (size_t)y.c_out, var);
            STEP(x.bn_fold(cb, g, be, mu, var, y.c_out, scale, x.template dst<float>(m->conv_s[l], (size_t)nh * y.c_out) + (size_t)h * y.c_out));
            bf16_t* frag = x.template dst<bf16_t>(m->conv_w[l], y.frag_per * nh) + y.frag_per * h;
            if (l == 0) {     // the fp32 copy feeds only the separate first conv
                const size_t per = (size_t)y.c_out * ic * 9;
                STEP(x.scale_rows(w, scale, y.c_out, ic * 9, x.template dst<float>(m->conv1_w, per * nh) + per * h));
                if (y.fam == K_CONVG) STEP(x.conv1g(w, scale, ic, y.c_out, frag));
                else if (y.fam == K_CONV) STEP(x.conv1(w, scale, ic, frag));
            } else if (y.fam == K_CONVG) STEP(x.conv_gen(w, scale, y.c_in, y.c_out, frag));
            else STEP(x.conv3x3(w, scale, y.c_out, frag));
            if (l == 1 && p.convx12) STEP(x.conv3x3(w, scale, y.c_out, x.template dst<bf16_t>(m->conv2_wx, p.c2x_per * nh) + p.c2x_per * h));
        }
        // fc1 of the RECURRENT heads only (the pitch head's is folded into its LogisticBank below), columns permuted from the reference's
        // (channel, freq) to the conv kernels' (freq, channel) order; columns kfc .. kfc_pad are zero
        if (h < m->n_rec) {
            const float* fb;
            STEP(need_fc1(h, w, fb));
            STEP(linear(m->fc1, h, w, m->dim_am, m->kfc, 0, m->fc1.n_pad, m->nf3, m->fq));
            STEP(x.copy(bias(m->fc1, h), fb, m->dim_am));
        }
    }
    // ---- LSTM + LogisticBank of a recurrent stage: input projection rows [fwd | reverse], merged biases b_ih + b_hh, W_hh fragments, output layer
    auto pack_rec = [&](const std::string& lstm, const std::string& bank, int dim_in, LinearPack& ih, DevBuf& hh, LinearPack& outp, int grp) {
        const float *wif, *wib, *whf, *whb, *bif, *bib, *bhf, *bhb, *wo, *bo;
        const std::string q = lstm + ".mlm.";
        NEED(q + "weight_ih_l0", (size_t)G * dim_in, wif); NEED(q + "weight_ih_l0_reverse", (size_t)G * dim_in, wib);
        NEED(q + "weight_hh_l0", (size_t)G * m->hid, whf); NEED(q + "weight_hh_l0_reverse", (size_t)G * m->hid, whb);
        NEED(q + "bias_ih_l0", (size_t)G, bif); NEED(q + "bias_ih_l0_reverse", (size_t)G, bib);
        NEED(q + "bias_hh_l0", (size_t)G, bhf); NEED(q + "bias_hh_l0_reverse", (size_t)G, bhb);
        STEP(linear(ih, grp, wif, G, dim_in, 0, G, 0, 0));
        STEP(linear(ih, grp, wib, G, dim_in, G, ih.n_pad - G, 0, 0));
        STEP(x.vec_add(bif, bhf, G, bias(ih, grp)));
        STEP(x.vec_add(bib, bhb, G, bias(ih, grp) + G));
        STEP(x.bilstm(whf, whb, x.template dst<bf16_t>(hh, m->hh_elems * ih.groups) + m->hh_elems * grp));
        STEP(need_bank(bank, m->dim_lm, wo, bo));
        STEP(linear(outp, grp, wo, m->n_out, m->dim_lm, 0, outp.n_pad, 0, 0));
        STEP(x.copy(bias(outp, grp), bo, m->n_out));
        return (int)AMTX_OK;
    };
    for (int r = 0; r < m->n_rec; ++r) STEP(pack_rec(m->head_names[r] + ".1", m->head_names[r] + ".2", m->dim_am, m->rec_ih, m->rec_hh, m->rec_out, r));
    // ---- pitch head.  Its fc1 feeds its LogisticBank directly (AcousticModel.fc1 is Linear + Dropout, no activation:
    // onsetsframes.py:422-427, then models/common.py:539), so in eval mode the two Linear layers are one:
    //     logits = W_out (W_fc1 a + b_fc1) + b_out = (W_out W_fc1) a + (W_out b_fc1 + b_out)
    // folded in double precision (the same kind of weight folding as the BatchNorms above): a K = kfc, N = n_out GEMM replaces a
    // K = kfc, N = dim_am one plus a K = dim_am, N = n_out one, and the dim_am-wide activation never exists.
    {
        const float *wo, *bo, *w1, *b1;
        STEP(need_bank("pitch_head.1", m->dim_am, wo, bo));
        STEP(need_fc1(nh - 1, w1, b1));
        STEP(x.head_fold(wo, w1, b1, bo, wfold, bfold));
        STEP(linear(m->pitch_out, 0, wfold, m->n_out, m->kfc_pad, 0, m->pitch_out.n_pad, 0, 0));
        STEP(x.copy(bias(m->pitch_out, 0), bfold, m->n_out));
    }
    // ---- adjoin: LSTM over the joint logits + LogisticBank
    return pack_rec("adjoin.0", "adjoin.1", m->dim_aj, m->adj_ih, m->adj_hh, m->adj_out, 0);
}

}  // namespace

extern "C" int amtx_of_model_finalize(amtx_of_model* m) {
    AMTX_REQUIRE(m, "amtx_of_model_finalize: null model");
    STEP(amtx_quiesce_before_resync(m->packed_once));
    if (m->plan.layer[2].fam == K_CONVG && (!amtx_conv3x3_gen_ntc(m->nf1, m->nf2) || !amtx_conv3x3_gen_ntc(m->nf2, m->nf3))) {
        amtx_set_error("of_model: no convolution kernel for %d -> %d -> %d channels", m->nf1, m->nf2, m->nf3);
        return AMTX_ERR_UNSUPPORTED;
    }
    HostPack x{m};
    STEP(pack_model(m, x));
    // the upload order is part of the recorded table (tests/golden/of_conv_plan.json); a buffer this model does not have has no image
    DevBuf* order[] = {&m->conv1_w, &m->conv_s[0], &m->conv_w[0], &m->conv_w[1], &m->conv2_wx, &m->conv_s[1], &m->conv_w[2], &m->conv_s[2],
                       &m->fc1.w, &m->fc1.b, &m->rec_ih.w, &m->rec_ih.b, &m->rec_hh, &m->rec_out.w, &m->rec_out.b, &m->pitch_out.w, &m->pitch_out.b,
                       &m->adj_ih.w, &m->adj_ih.b, &m->adj_hh, &m->adj_out.w, &m->adj_out.b};
    for (DevBuf* b : order) {
        const std::vector<char>& v = x.image[b];
        if (!v.empty()) STEP(b->upload(v.data(), v.size()));
    }
    m->store.host.clear();
    m->finalized = true;
    m->packed_once = true;
    return AMTX_OK;
}

// Weight RE-SYNC without leaving the GPU.  After one host-side amtx_of_model_finalize, later weight versions can be handed over as
// device pointers under the same state_dict names.  Built for every configuration the engine runs (the engine validates at every
// checkpoint of train.py, amt_tools/train.py:183-189): model_complexity 2 .. 5, one or several input channels, any precision -- except a
// multi-channel first conv on conv.hip's kernel (AMTX_NO_CONVG_MC2, or 9 and more input channels at 32 / 32 / 64; ConvPlan::device_resync),
// which answers AMTX_ERR_UNSUPPORTED and keeps the host path.
extern "C" int amtx_of_model_set_tensor_device(amtx_of_model* m, const char* name, const float* device_data, int64_t numel) {
    AMTX_REQUIRE(m && name && device_data && numel > 0, "amtx_of_model_set_tensor_device: bad argument");
    m->store.set_device(name, device_data, numel);
    return AMTX_OK;
}

extern "C" int amtx_of_model_finalize_device(amtx_of_model* m, void* stream_) {
    AMTX_REQUIRE(m, "amtx_of_model_finalize_device: null model");
    struct Clear {                             // the borrowed device pointers are dropped on EVERY exit: the caller may free them afterwards
        amtx_of_model* m;
        ~Clear() { m->store.device.clear(); }
    } clear{m};
    AMTX_REQUIRE(m->finalized, "amtx_of_model_finalize_device: the first sync goes through amtx_of_model_finalize (it allocates the packed buffers)");
    if (!m->plan.device_resync) {
        amtx_set_error("amtx_of_model_finalize_device: no device packer for conv.hip's multi-channel first conv; use amtx_of_model_finalize");
        return AMTX_ERR_UNSUPPORTED;
    }
    DevicePack x{m, (hipStream_t)stream_, true};
    STEP(pack_model(m, x));
    STEP(amtx_quiesce_before_resync(m->packed_once));
    x.dry = false;
    const int rc = pack_model(m, x);
    if (rc != AMTX_OK) m->finalized = false;   // a launch failed half-way: the packed weights are no version at all, refuse to run on them
    return rc;
}

extern "C" size_t amtx_of_workspace_bytes(const amtx_of_model* m, int batch, int num_frames) {
    if (!m || batch <= 0 || num_frames <= 0) return 0;
    return carve(m, batch, num_frames, nullptr).total;
}

static GemmArgs gemm_args(const void* A, int64_t lda, int a_type, const LinearPack& lp, int planes, void* C, int64_t ldc, int c_type,
                          int64_t M, int groups, int64_t a_gs, int64_t c_gs) {
    GemmArgs g;
    g.A = A; g.lda = lda; g.a_type = a_type;
    g.W = (const bf16_t*)lp.w.p; g.n_pad = lp.n_pad; g.k_pad = lp.k_pad; g.planes = planes;
    g.bias = (const float*)lp.b.p;
    g.C = C; g.ldc = ldc; g.c_type = c_type;
    g.M = M; g.N = lp.N; g.K = lp.K;
    g.groups = groups; g.a_gs = a_gs; g.w_gs = (int64_t)lp.n_pad * lp.k_pad * planes; g.bias_gs = lp.N; g.c_gs = c_gs;
    return g;
}

// The features of one forward call.  clip_max != null: `feats` are raw power values, dB-scaled by the conv kernel while it stages them
// (amtx_of_forward_power); feats16 != null: the features as [B][T][F][8] 16-bit channels-last instead of `feats` (amtx_of_forward_feats16)
struct FeatsIn { const float* feats; const void* feats16; int64_t stride_b, stride_c, stride_t, stride_f; const float *clip_max, *ref; };

// conv1 -> conv2 + pool -> conv3 + pool of every acoustic head on the path `call` names: features -> w.a3.  `mark` closes the stages
// conv1, conv2_pool (the fused stack: all of it) and conv3_pool.
template <class Mark>
static int run_convs(const amtx_of_model* m, const ConvCall& call, const FeatsIn& in, const Workspace& w, int B, int T, hipStream_t s, Mark&& mark) {
    const ConvPlan& p = m->plan;
    const KernelSet* k = m->k;
    const int64_t BT = (int64_t)B * T;
    const int F = m->dim_in, F2 = F / 2, at = m->act_type, pl = m->planes, nh = m->n_heads;
    int rc;
    if (call.path == PATH_CONV1) {
        Conv1Args c1;
        c1.in = in.feats; c1.stride_b = in.stride_b; c1.stride_c = in.stride_c; c1.stride_t = in.stride_t; c1.stride_f = in.stride_f;
        c1.w = (const float*)m->conv1_w.p; c1.shift = (const float*)m->conv_s[0].p; c1.out = w.a1; c1.out_type = at;
        c1.B = B; c1.T = T; c1.F = F; c1.c_in = m->in_channels; c1.c_out = m->nf1;
        c1.groups = nh; c1.w_gs = (int64_t)m->nf1 * m->in_channels * 9; c1.shift_gs = m->nf1; c1.out_gs = BT * F * m->nf1;
        if ((rc = k->launch_conv1(c1, s)) != AMTX_OK) return rc;
    }
    mark();
    ConvArgs c2;
    c2.in = w.a1; c2.in_type = at; c2.wfrag = (const bf16_t*)m->conv_w[1].p; c2.planes = pl; c2.shift = (const float*)m->conv_s[1].p;
    c2.out = w.a2; c2.out_type = at; c2.B = B; c2.T = T; c2.F = F; c2.c_out = m->nf2;
    c2.groups = nh; c2.in_gs = BT * F * m->nf1; c2.shift_gs = m->nf2; c2.w_gs = (int64_t)p.layer[1].frag_per; c2.out_gs = BT * F2 * m->nf2;
    const int64_t a2_split = BT * F2 * m->nf2 * nh, a3_split = BT * m->kfc_pad * nh;   // two-plane maps: plane stride = all groups of one plane
    if (p.two_plane_acts) { c2.out_type = AMTX_T_SPLIT; c2.out_split = a2_split; }
    if (p.conv1_fused) {   // Conv(c_in->32)+BN+ReLU computed inside the conv2 kernel; a1 is never materialised
        c2.in = nullptr;
        c2.feats = in.feats; c2.f_stride_b = in.stride_b; c2.f_stride_c = in.stride_c; c2.f_stride_t = in.stride_t; c2.f_stride_f = in.stride_f;
        c2.c_in = m->in_channels; c2.w1frag = (const bf16_t*)m->conv_w[0].p; c2.shift1 = (const float*)m->conv_s[0].p; c2.w1_gs = (int64_t)p.layer[0].frag_per;
        c2.f_clip_max = in.clip_max; c2.f_ref = in.ref;
        if (in.feats16) { c2.feats = nullptr; c2.feats16 = in.feats16; }
    }
    // convx12: layer2's weights in conv.hip's order; the lo plane of the features lies right behind the hi plane
    if (call.path == PATH_CONVX12) { c2.in_split = BT * F * 8; c2.wfrag = (const bf16_t*)m->conv2_wx.p; c2.w_gs = (int64_t)p.c2x_per; }
    if (call.path == PATH_STACK)
        rc = k->launch_conv_stack(c2, (const bf16_t*)m->conv_w[2].p, (int64_t)p.layer[2].frag_per, (const float*)m->conv_s[2].p, w.a3, BT * m->kfc_pad, call.a3_plane, s);
    else if (call.path == PATH_CONVX12) rc = amtx_launch_convx12(c2, s);
    else rc = p.layer[1].fam == K_CONVG ? k->launch_conv3x3_gen(c2, m->nf1, s) : k->launch_conv3x3(c2, s);
    if (rc != AMTX_OK) return rc;
    mark();
    ConvArgs c3 = c2;
    c3.feats = nullptr; c3.feats16 = nullptr; c3.w1frag = nullptr; c3.shift1 = nullptr; c3.c_in = 0;
    c3.in = w.a2; c3.wfrag = (const bf16_t*)m->conv_w[2].p; c3.shift = (const float*)m->conv_s[2].p; c3.out = w.a3;
    c3.F = F2; c3.c_out = m->nf3; c3.in_gs = BT * F2 * m->nf2; c3.w_gs = (int64_t)p.layer[2].frag_per; c3.shift_gs = m->nf3; c3.out_gs = BT * m->kfc_pad;
    if (p.two_plane_acts) { c3.in_type = AMTX_T_SPLIT; c3.in_split = a2_split; c3.out_type = AMTX_T_SPLIT; c3.out_split = a3_split; }
    if (m->kfc_pad != m->kfc) {
        // rows of a3 are padded to the DMA GEMM's k-tile: the pad columns meet zero weights, they only have to be finite
        AMTX_REQUIRE(p.layer[2].fam == K_CONVG, "amtx_of_forward: internal: padded fc1 rows need the general conv kernel");
        c3.out_ts = m->kfc_pad;
        const size_t es = amtx_tsize(at);
        if ((rc = amtx_launch_zero_cols(w.a3 + (size_t)m->kfc * es, (int64_t)m->kfc_pad * es, (int)((m->kfc_pad - m->kfc) * es), BT * nh, s)) != AMTX_OK) return rc;
    }
    if (call.path != PATH_STACK && (rc = p.layer[2].fam == K_CONVG ? k->launch_conv3x3_gen(c3, m->nf2, s) : k->launch_conv3x3(c3, s)) != AMTX_OK) return rc;
    mark();
    return AMTX_OK;
}

static int of_forward_impl(const amtx_of_model* m, const FeatsIn& in, int B, int T, void* workspace, size_t workspace_bytes, float* out_onsets,
                           float* out_multi_pitch, float* logits_onsets, float* logits_multi_pitch, float* logits_pitch_head, void* stream_) {
    AMTX_REQUIRE(m && m->finalized, "amtx_of_forward: model not finalized");
    AMTX_REQUIRE(!in.clip_max || m->plan.fuses_db_scale, "amtx_of_forward_power: this model does not stage its features in the conv kernel");
    AMTX_REQUIRE(!in.feats16 || m->plan.takes_feats16, "amtx_of_forward_feats16: this model does not stage 16-bit channels-last features");
    AMTX_REQUIRE((in.feats || in.feats16) && workspace, "amtx_of_forward: null pointer");
    AMTX_REQUIRE(B > 0 && T > 0, "amtx_of_forward: bad batch/num_frames");
    Workspace w = carve(m, B, T, (char*)workspace);
    AMTX_REQUIRE(workspace_bytes >= w.total, "amtx_of_forward: workspace too small (%zu < %zu)", workspace_bytes, w.total);
    AMTX_REQUIRE(((uintptr_t)workspace % 256) == 0, "amtx_of_forward: workspace must be 256-byte aligned");
    hipStream_t s = (hipStream_t)stream_;
    const int64_t BT = (int64_t)B * T;
    const int at = m->act_type, pl = m->planes;
    const KernelSet* k = m->k;
    int rc;
    std::vector<hipEvent_t>* evs = nullptr;
    if (m->prof) {
        m->prof_events.emplace_back();
        evs = &m->prof_events.back();
    }
    auto mark = [&]() {
        if (!evs) return;
        hipEvent_t e;
        if (hipEventCreate(&e) == hipSuccess) { (void)hipEventRecord(e, s); evs->push_back(e); }
    };
    mark();

    const ConvCall call = resolve_conv(m, B, T, in.feats16 != nullptr);
    if ((rc = run_convs(m, call, in, w, B, T, s, mark)) != AMTX_OK) return rc;
    const bool sp = m->plan.two_plane_acts, no_roll_epi = m->plan.no_roll_epilogue;
    const int64_t a3_plane = call.a3_plane, a3_split = BT * m->kfc_pad * m->n_heads, e_split = BT * m->dim_am * m->n_heads;   // two-plane maps: plane stride = all groups of one plane

    // fc1 of the recurrent heads (heads 0..n_rec-1 of a3); the pitch head's fc1 is folded into its output layer below
    const int at_d = sp ? AMTX_T_SPLIT : at;   // element type of the dense layers' activations
    GemmArgs g = gemm_args(w.a3, m->kfc_pad, at_d, m->fc1, pl, w.e, m->dim_am, at_d, BT, m->n_rec, BT * m->kfc_pad, BT * m->dim_am);
    g.a_plane = a3_plane; g.a_split = a3_split; g.c_split = e_split;
    if ((rc = k->launch_gemm(g, s)) != AMTX_OK) return rc;
    mark();

    // recurrent heads: heads 0..n_rec-1 of `e`
    g = gemm_args(w.e, m->dim_am, at_d, m->rec_ih, pl, w.xp, m->xw, at, BT, m->n_rec, BT * m->dim_am, BT * m->xw);
    g.a_split = e_split;
    if ((rc = k->launch_gemm(g, s)) != AMTX_OK) return rc;
    mark();
    LstmArgs l;
    l.xproj = w.xp; l.x_type = at; l.whh = (const bf16_t*)m->rec_hh.p; l.planes = pl; l.out = w.l1; l.out_type = at;
    l.B = B; l.T = T; l.groups = m->n_rec; l.x_gs = BT * m->xw; l.w_gs = (int64_t)m->hh_elems; l.out_gs = BT * m->dim_lm;
    l.hidden = m->hid;
    if ((rc = k->launch_bilstm(l, s)) != AMTX_OK) return rc;
    mark();
    // LogisticBank of each recurrent head -> joint[:, r*n_out : (r+1)*n_out]; group stride of C = n_out columns
    g = gemm_args(w.l1, m->dim_lm, at, m->rec_out, pl, w.joint, m->dim_aj, AMTX_T_F32, BT, m->n_rec, BT * m->dim_lm, m->n_out);
    // piano rolls (LogisticBank.finalize_output with threshold 0.5) come out of the LogisticBank GEMMs' epilogues where that kernel has
    // one (bf16 mode); otherwise amtx_launch_pianoroll below reads the logits back
    const bool roll_on = out_onsets && !no_roll_epi && amtx_gemm_has_roll_epilogue(g);
    if (roll_on) { g.roll_out = out_onsets; g.roll_T = T; g.roll_thr = 0.5f; g.roll_group = 0; }
    // bf16 mode: the refinement stage's input (the joint logits rounded to bf16, K zero-padded to the DMA GEMM's 64-deep k-tile) is
    // written by the same two epilogues instead of a conversion pass over the fp32 joint buffer; the fp32 joint logits themselves are
    // only written when something reads them (logit outputs, the offset head's probabilities, the modes without these epilogues)
    const int kp = (m->dim_aj + 63) / 64 * 64;
    GemmArgs gp = gemm_args(w.a3 + (size_t)(m->n_heads - 1) * BT * m->kfc_pad * (sp ? 2 : amtx_tsize(at)), m->kfc_pad, at_d, m->pitch_out, pl,
                            w.joint + (size_t)m->n_rec * m->n_out * sizeof(float), m->dim_aj, AMTX_T_F32, BT, 1, 0, 0);
    gp.a_plane = a3_plane; gp.a_split = a3_split;
    const bool copy_on = pl == 1 && !no_roll_epi && amtx_gemm_has_roll_epilogue(g) && amtx_gemm_has_roll_epilogue(gp) && m->n_out % 4 == 0 &&
                         (kp - m->dim_aj) % 4 == 0 && gp.N + (kp - m->dim_aj) <= gp.n_pad;
    if (copy_on) {
        g.copy16 = (bf16_t*)w.joint16; g.copy16_ld = kp; g.copy16_col0 = 0; g.copy16_gs = m->n_out; g.copy16_pad = 0;
        gp.copy16 = (bf16_t*)w.joint16; gp.copy16_ld = kp; gp.copy16_col0 = m->n_rec * m->n_out; gp.copy16_gs = 0; gp.copy16_pad = kp - m->dim_aj;
        if (roll_on && !logits_onsets && !logits_pitch_head && !m->has_offsets) { g.C = nullptr; gp.C = nullptr; }
    }
    if ((rc = k->launch_gemm(g, s)) != AMTX_OK) return rc;
    mark();
    // pitch head: (fc1 . LogisticBank) folded, straight from its conv3 map -> last n_out columns of joint
    if ((rc = k->launch_gemm(gp, s)) != AMTX_OK) return rc;
    mark();

    // adjoin
    if (pl == 1) {
        // bf16 mode: the joint logits rounded to bf16 (zero-padded to a 64-multiple K) feed the direct-to-LDS GEMM
        if (!copy_on && (rc = amtx_launch_cvt_pad_bf16((const float*)w.joint, m->dim_aj, m->dim_aj, (bf16_t*)w.joint16, kp, BT, s, m->f16)) != AMTX_OK) return rc;
        g = gemm_args(w.joint16, kp, AMTX_T_BF16, m->adj_ih, pl, w.xp2, m->xw, at, BT, 1, 0, 0);
        g.K = kp;
    } else if (sp) {
        // two-plane mode: the joint logits as two 16-bit planes, K zero-padded to whole 32-deep stages, feed the direct-to-LDS two-plane GEMM
        if ((rc = amtx_launch_cvt_split((const float*)w.joint, m->dim_aj, m->dim_aj, (bf16_t*)w.joint16, kp, BT * kp, BT, s)) != AMTX_OK) return rc;
        g = gemm_args(w.joint16, kp, AMTX_T_SPLIT, m->adj_ih, pl, w.xp2, m->xw, at, BT, 1, 0, 0);
        g.K = kp; g.a_split = BT * kp;
    } else {
        g = gemm_args(w.joint, m->dim_aj, AMTX_T_F32, m->adj_ih, pl, w.xp2, m->xw, at, BT, 1, 0, 0);
    }
    if ((rc = k->launch_gemm(g, s)) != AMTX_OK) return rc;
    mark();
    l.xproj = w.xp2; l.whh = (const bf16_t*)m->adj_hh.p; l.out = w.l2; l.groups = 1;
    if ((rc = k->launch_bilstm(l, s)) != AMTX_OK) return rc;
    mark();
    g = gemm_args(w.l2, m->dim_lm, at, m->adj_out, pl, w.mp, m->n_out, AMTX_T_F32, BT, 1, 0, 0);
    const bool roll_mp = out_multi_pitch && !no_roll_epi && amtx_gemm_has_roll_epilogue(g);
    if (roll_mp) {
        g.roll_out = out_multi_pitch; g.roll_T = T; g.roll_thr = 0.5f; g.roll_group = 0;
        if (!logits_multi_pitch) g.C = nullptr;            // nobody reads the refined logits then: only the roll is written
    }
    if ((rc = k->launch_gemm(g, s)) != AMTX_OK) return rc;
    mark();

    // piano rolls of the modes whose LogisticBank GEMM has no roll epilogue (x3)
    if (out_onsets && !roll_on && (rc = amtx_launch_pianoroll((const float*)w.joint, m->dim_aj, 0, B, T, m->n_out, 0.5f, out_onsets, s)) != AMTX_OK) return rc;
    if (out_multi_pitch && !roll_mp && (rc = amtx_launch_pianoroll((const float*)w.mp, m->n_out, 0, B, T, m->n_out, 0.5f, out_multi_pitch, s)) != AMTX_OK) return rc;

    mark();
    // optional raw logits, contiguous (B, T, n_out)
    const size_t row = (size_t)m->n_out * sizeof(float);
    if (logits_onsets)
        AMTX_CHECK_HIP(hipMemcpy2DAsync(logits_onsets, row, w.joint, (size_t)m->dim_aj * 4, row, BT, hipMemcpyDeviceToDevice, s));
    if (logits_pitch_head)
        AMTX_CHECK_HIP(hipMemcpy2DAsync(logits_pitch_head, row, w.joint + (size_t)m->n_rec * row, (size_t)m->dim_aj * 4, row, BT,
                                        hipMemcpyDeviceToDevice, s));
    if (logits_multi_pitch)
        AMTX_CHECK_HIP(hipMemcpyAsync(logits_multi_pitch, w.mp, row * BT, hipMemcpyDeviceToDevice, s));
    return AMTX_OK;
}

// 1 when amtx_of_forward_power applies: one input channel and the first conv fused into the C_out = 32 conv kernel (conv.hip, KS = 1)
extern "C" int amtx_of_fuses_db_scale(const amtx_of_model* m) { return m && m->finalized && m->plan.fuses_db_scale; }
extern "C" int amtx_of_conv_stack_fused(const amtx_of_model* m, int batch, int num_frames) { return m && resolve_conv(m, batch, num_frames, false).path == PATH_STACK; }

extern "C" int amtx_of_forward(const amtx_of_model* m, const float* feats, int64_t stride_b, int64_t stride_c, int64_t stride_t,
                               int64_t stride_f, int batch, int num_frames, void* workspace, size_t workspace_bytes,
                               float* out_onsets, float* out_multi_pitch, float* logits_onsets, float* logits_multi_pitch,
                               float* logits_pitch_head, void* stream_) {
    return of_forward_impl(m, {feats, nullptr, stride_b, stride_c, stride_t, stride_f, nullptr, nullptr}, batch, num_frames, workspace, workspace_bytes,
                           out_onsets, out_multi_pitch, logits_onsets, logits_multi_pitch, logits_pitch_head, stream_);
}

extern "C" int amtx_of_forward_power(const amtx_of_model* m, const float* power, int64_t stride_b, int64_t stride_t, int64_t stride_f,
                                     const float* clip_max, const float* ref, int batch, int num_frames, void* workspace,
                                     size_t workspace_bytes, float* out_onsets, float* out_multi_pitch, float* logits_onsets,
                                     float* logits_multi_pitch, float* logits_pitch_head, void* stream_) {
    AMTX_REQUIRE(clip_max, "amtx_of_forward_power: clip_max is null");
    return of_forward_impl(m, {power, nullptr, stride_b, 0, stride_t, stride_f, clip_max, ref}, batch, num_frames, workspace, workspace_bytes,
                           out_onsets, out_multi_pitch, logits_onsets, logits_multi_pitch, logits_pitch_head, stream_);
}

// 1 when amtx_of_forward_feats16 applies: 2 .. 8 input channels and the first conv fused tap-major into the general conv kernel's 32-channel
// pipelined variant (convg.hip: one-plane bf16 mode, model_complexity 2) -- the HCQT configuration (BASELINE config 3)
extern "C" int amtx_of_takes_feats16(const amtx_of_model* m) { return m && m->finalized ? m->plan.takes_feats16 : 0; }

extern "C" int amtx_of_forward_feats16(const amtx_of_model* m, const void* feats16, int batch, int num_frames, void* workspace, size_t workspace_bytes,
                                       float* out_onsets, float* out_multi_pitch, float* logits_onsets, float* logits_multi_pitch,
                                       float* logits_pitch_head, void* stream_) {
    AMTX_REQUIRE(feats16, "amtx_of_forward_feats16: feats16 is null");
    return of_forward_impl(m, {nullptr, feats16, 0, 0, 0, 0, nullptr, nullptr}, batch, num_frames, workspace, workspace_bytes, out_onsets, out_multi_pitch,
                           logits_onsets, logits_multi_pitch, logits_pitch_head, stream_);
}

// OnsetsFrames2: the offset head's LogisticBank output of the LAST amtx_of_forward on this workspace
// (onsetsframes.py:256-261,323-325: finalize_output without a threshold = sigmoid probabilities, (B, n_out, T)).
extern "C" int amtx_of_offsets(const amtx_of_model* m, void* workspace, size_t workspace_bytes, int batch, int num_frames, float* out_offsets,
                               float* logits_offsets, void* stream_) {
    AMTX_REQUIRE(m && m->finalized, "amtx_of_offsets: model not finalized");
    AMTX_REQUIRE(m->has_offsets, "amtx_of_offsets: the model has no offset head");
    AMTX_REQUIRE(workspace && batch > 0 && num_frames > 0, "amtx_of_offsets: bad argument");
    Workspace w = carve(m, batch, num_frames, (char*)workspace);
    AMTX_REQUIRE(workspace_bytes >= w.total, "amtx_of_offsets: workspace too small");
    hipStream_t s = (hipStream_t)stream_;
    const int64_t BT = (int64_t)batch * num_frames;
    int rc;
    if (out_offsets && (rc = amtx_launch_pianoroll((const float*)w.joint, m->dim_aj, m->n_out, batch, num_frames, m->n_out, -1.0f, out_offsets, s)) != AMTX_OK)
        return rc;
    const size_t row = (size_t)m->n_out * sizeof(float);
    if (logits_offsets)
        AMTX_CHECK_HIP(hipMemcpy2DAsync(logits_offsets, row, w.joint + row, (size_t)m->dim_aj * 4, row, BT, hipMemcpyDeviceToDevice, s));
    return AMTX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The engine in two phases (include/amtx_ofseq.h): exact whole-track inference.  Past the convolutions every stage of of_forward_impl is
// row-wise except the recurrences, so the acoustic half runs on overlapped clips and hands the rows each clip keeps to the language half,
// which runs the rest once over whole tracks: the same launches on M = total_rows packed rows, with the packed-sequence recurrence
// (lstm.hip) and piano rolls (seqrows.hip) in place of the (B, T) ones.  The roll and copy16 epilogues of the LogisticBank GEMMs stay
// off in both phases: they transpose by (B, T).
namespace {

struct LanguageWorkspace { char *xp, *l1, *joint, *joint16, *xp2, *l2, *mp; size_t total; };

// the rows of `carve` from xp on, per packed row
LanguageWorkspace carve_language(const amtx_of_model* m, int64_t R, char* base) {
    LanguageWorkspace w;
    const size_t es = amtx_tsize(m->act_type), M = (size_t)R;
    WorkspaceCarver ws{base};
    w.xp = ws.take(M * m->xw * es * m->n_rec);
    w.l1 = ws.take(M * m->dim_lm * es * m->n_rec);
    w.joint = ws.take(M * m->dim_aj * sizeof(float));
    w.joint16 = ws.take(M * (size_t)((m->dim_aj + 63) / 64 * 64) * 2 * (m->plan.two_plane_acts ? 2 : 1));
    w.xp2 = ws.take(M * m->xw * es);
    w.l2 = ws.take(M * m->dim_lm * es);
    w.mp = ws.take(M * m->n_out * sizeof(float));
    w.total = ws.off;
    return w;
}

int of_acoustic_rows_impl(const amtx_of_model* m, const FeatsIn& in, int B, int T, void* workspace, size_t workspace_bytes, const int64_t* table_host,
                          const int64_t* table_dev, int64_t R, void* rows_e, float* rows_pitch, void* stream_) {
    AMTX_REQUIRE(m && m->finalized, "amtx_of_acoustic_rows: model not finalized");
    AMTX_REQUIRE(!in.clip_max || m->plan.fuses_db_scale, "amtx_of_acoustic_rows_power: this model does not stage its features in the conv kernel");
    AMTX_REQUIRE(!in.feats16 || m->plan.takes_feats16, "amtx_of_acoustic_rows_feats16: this model does not stage 16-bit channels-last features");
    AMTX_REQUIRE((in.feats || in.feats16) && workspace && table_host && table_dev && rows_e && rows_pitch, "amtx_of_acoustic_rows: null pointer");
    AMTX_REQUIRE(B > 0 && T > 0 && R > 0, "amtx_of_acoustic_rows: bad batch/num_frames/total_rows");
    Workspace w = carve(m, B, T, (char*)workspace);
    AMTX_REQUIRE(workspace_bytes >= w.total, "amtx_of_acoustic_rows: workspace too small (%zu < %zu)", workspace_bytes, w.total);
    AMTX_REQUIRE(((uintptr_t)workspace % 256) == 0, "amtx_of_acoustic_rows: workspace must be 256-byte aligned");
    for (int b = 0; b < B; ++b) {        // before anything is launched; amtx_launch_rows_gather checks the same rows again behind the GEMMs
        const int64_t* d = table_host + 3 * (int64_t)b;
        AMTX_REQUIRE(d[0] >= 0 && d[1] >= 0 && d[2] >= 0 && d[1] <= T && d[0] <= T - d[1] && d[1] <= R && d[2] <= R - d[1],
                     "amtx_of_acoustic_rows: clip %d: the row {%lld, %lld, %lld} leaves the clip's %d frames or the %lld packed rows", b, (long long)d[0],
                     (long long)d[1], (long long)d[2], T, (long long)R);
    }
    hipStream_t s = (hipStream_t)stream_;
    const int64_t BT = (int64_t)B * T;
    const int at = m->act_type, pl = m->planes;
    const KernelSet* k = m->k;
    int rc;
    const ConvCall call = resolve_conv(m, B, T, in.feats16 != nullptr);
    if ((rc = run_convs(m, call, in, w, B, T, s, [] {})) != AMTX_OK) return rc;
    const bool sp = m->plan.two_plane_acts;
    const int64_t a3_split = BT * m->kfc_pad * m->n_heads, e_split = BT * m->dim_am * m->n_heads;
    const int at_d = sp ? AMTX_T_SPLIT : at;
    GemmArgs g = gemm_args(w.a3, m->kfc_pad, at_d, m->fc1, pl, w.e, m->dim_am, at_d, BT, m->n_rec, BT * m->kfc_pad, BT * m->dim_am);
    g.a_plane = call.a3_plane; g.a_split = a3_split; g.c_split = e_split;
    if ((rc = k->launch_gemm(g, s)) != AMTX_OK) return rc;
    // the pitch head's folded GEMM into dense fp32 logits [B T][n_out]: w.mp, which nothing else of this phase uses
    GemmArgs gp = gemm_args(w.a3 + (size_t)(m->n_heads - 1) * BT * m->kfc_pad * (sp ? 2 : amtx_tsize(at)), m->kfc_pad, at_d, m->pitch_out, pl, w.mp,
                            m->n_out, AMTX_T_F32, BT, 1, 0, 0);
    gp.a_plane = call.a3_plane; gp.a_split = a3_split;
    if ((rc = k->launch_gemm(gp, s)) != AMTX_OK) return rc;
    // kept rows -> packed rows: head by head (a two-plane map: both planes per launch)
    const size_t es = sp ? 2 : amtx_tsize(at);
    for (int h = 0; h < m->n_rec; ++h)
        if ((rc = amtx_launch_rows_gather(w.e + (size_t)h * BT * m->dim_am * es, B, T, (int64_t)m->dim_am * es, sp ? 2 : 1, e_split * 2, table_host, table_dev,
                                          (char*)rows_e + (size_t)h * R * m->dim_am * es, R, (int64_t)m->n_rec * R * m->dim_am * 2, s)) != AMTX_OK)
            return rc;
    return amtx_launch_rows_gather(w.mp, B, T, (int64_t)m->n_out * 4, 1, 0, table_host, table_dev, rows_pitch, R, 0, s);
}

}  // namespace

extern "C" size_t amtx_of_rows_e_bytes(const amtx_of_model* m, int64_t total_rows) {
    return m && total_rows > 0 ? (size_t)total_rows * m->dim_am * amtx_tsize(m->act_type) * m->n_rec : 0;
}

extern "C" int amtx_of_acoustic_rows(const amtx_of_model* m, const float* feats, int64_t stride_b, int64_t stride_c, int64_t stride_t, int64_t stride_f,
                                     int batch, int num_frames, void* workspace, size_t workspace_bytes, const int64_t* table_host,
                                     const int64_t* table_dev, int64_t total_rows, void* rows_e, float* rows_pitch, void* stream) {
    return of_acoustic_rows_impl(m, {feats, nullptr, stride_b, stride_c, stride_t, stride_f, nullptr, nullptr}, batch, num_frames, workspace, workspace_bytes,
                                 table_host, table_dev, total_rows, rows_e, rows_pitch, stream);
}

extern "C" int amtx_of_acoustic_rows_power(const amtx_of_model* m, const float* power, int64_t stride_b, int64_t stride_t, int64_t stride_f,
                                           const float* clip_max, const float* ref, int batch, int num_frames, void* workspace, size_t workspace_bytes,
                                           const int64_t* table_host, const int64_t* table_dev, int64_t total_rows, void* rows_e, float* rows_pitch,
                                           void* stream) {
    AMTX_REQUIRE(clip_max, "amtx_of_acoustic_rows_power: clip_max is null");
    return of_acoustic_rows_impl(m, {power, nullptr, stride_b, 0, stride_t, stride_f, clip_max, ref}, batch, num_frames, workspace, workspace_bytes, table_host,
                                 table_dev, total_rows, rows_e, rows_pitch, stream);
}

extern "C" int amtx_of_acoustic_rows_feats16(const amtx_of_model* m, const void* feats16, int batch, int num_frames, void* workspace,
                                             size_t workspace_bytes, const int64_t* table_host, const int64_t* table_dev, int64_t total_rows,
                                             void* rows_e, float* rows_pitch, void* stream) {
    AMTX_REQUIRE(feats16, "amtx_of_acoustic_rows_feats16: feats16 is null");
    return of_acoustic_rows_impl(m, {nullptr, feats16, 0, 0, 0, 0, nullptr, nullptr}, batch, num_frames, workspace, workspace_bytes, table_host, table_dev,
                                 total_rows, rows_e, rows_pitch, stream);
}

extern "C" size_t amtx_of_language_workspace_bytes(const amtx_of_model* m, int64_t total_rows) {
    if (!m || total_rows <= 0) return 0;
    return carve_language(m, total_rows, nullptr).total;
}

extern "C" int amtx_of_language_rows(const amtx_of_model* m, const void* rows_e, const float* rows_pitch, const int64_t* seqs_host,
                                     const int64_t* seqs_dev, int num_seqs, int64_t total_rows, void* workspace, size_t workspace_bytes,
                                     float* out_onsets, float* out_multi_pitch, float* out_offsets, float* logits_onsets, float* logits_multi_pitch,
                                     float* logits_offsets, void* stream_) {
    AMTX_REQUIRE(m && m->finalized, "amtx_of_language_rows: model not finalized");
    AMTX_REQUIRE(rows_e && rows_pitch && seqs_dev && workspace, "amtx_of_language_rows: null pointer");
    AMTX_REQUIRE(m->has_offsets || (!out_offsets && !logits_offsets), "amtx_of_language_rows: the model has no offset head");
    int64_t max_len = 0;
    int rc = amtx_check_seq_table("amtx_of_language_rows", seqs_host, num_seqs, total_rows, &max_len);
    if (rc != AMTX_OK) return rc;
    const int64_t R = total_rows;
    LanguageWorkspace w = carve_language(m, R, (char*)workspace);
    AMTX_REQUIRE(workspace_bytes >= w.total, "amtx_of_language_rows: workspace too small (%zu < %zu)", workspace_bytes, w.total);
    AMTX_REQUIRE(((uintptr_t)workspace % 256) == 0, "amtx_of_language_rows: workspace must be 256-byte aligned");
    hipStream_t s = (hipStream_t)stream_;
    const int at = m->act_type, pl = m->planes;
    const KernelSet* k = m->k;
    const bool sp = m->plan.two_plane_acts;
    const int at_d = sp ? AMTX_T_SPLIT : at;

    // recurrent heads: x-projection, packed recurrence, LogisticBank -> joint[:, r n_out : (r + 1) n_out]
    GemmArgs g = gemm_args(rows_e, m->dim_am, at_d, m->rec_ih, pl, w.xp, m->xw, at, R, m->n_rec, R * m->dim_am, R * m->xw);
    g.a_split = R * m->dim_am * m->n_rec;
    if ((rc = k->launch_gemm(g, s)) != AMTX_OK) return rc;
    LstmSeqArgs l;
    l.l.xproj = w.xp; l.l.x_type = at; l.l.whh = (const bf16_t*)m->rec_hh.p; l.l.planes = pl; l.l.out = w.l1; l.l.out_type = at;
    l.l.B = num_seqs; l.l.T = 0; l.l.groups = m->n_rec; l.l.x_gs = R * m->xw; l.l.w_gs = (int64_t)m->hh_elems; l.l.out_gs = R * m->dim_lm;
    l.l.hidden = m->hid;
    l.seqs = seqs_dev; l.S = num_seqs;
    if ((rc = k->launch_bilstm_seq(l, s)) != AMTX_OK) return rc;
    g = gemm_args(w.l1, m->dim_lm, at, m->rec_out, pl, w.joint, m->dim_aj, AMTX_T_F32, R, m->n_rec, R * m->dim_lm, m->n_out);
    if ((rc = k->launch_gemm(g, s)) != AMTX_OK) return rc;
    // the pitch head's columns, computed by the acoustic phase
    const size_t row = (size_t)m->n_out * sizeof(float);
    AMTX_CHECK_HIP(hipMemcpy2DAsync(w.joint + (size_t)m->n_rec * row, (size_t)m->dim_aj * 4, rows_pitch, row, row, R, hipMemcpyDeviceToDevice, s));

    // refinement stage
    const int kp = (m->dim_aj + 63) / 64 * 64;
    if (pl == 1) {
        if ((rc = amtx_launch_cvt_pad_bf16((const float*)w.joint, m->dim_aj, m->dim_aj, (bf16_t*)w.joint16, kp, R, s, m->f16)) != AMTX_OK) return rc;
        g = gemm_args(w.joint16, kp, AMTX_T_BF16, m->adj_ih, pl, w.xp2, m->xw, at, R, 1, 0, 0);
        g.K = kp;
    } else if (sp) {
        if ((rc = amtx_launch_cvt_split((const float*)w.joint, m->dim_aj, m->dim_aj, (bf16_t*)w.joint16, kp, R * kp, R, s)) != AMTX_OK) return rc;
        g = gemm_args(w.joint16, kp, AMTX_T_SPLIT, m->adj_ih, pl, w.xp2, m->xw, at, R, 1, 0, 0);
        g.K = kp; g.a_split = R * kp;
    } else {
        g = gemm_args(w.joint, m->dim_aj, AMTX_T_F32, m->adj_ih, pl, w.xp2, m->xw, at, R, 1, 0, 0);
    }
    if ((rc = k->launch_gemm(g, s)) != AMTX_OK) return rc;
    l.l.xproj = w.xp2; l.l.whh = (const bf16_t*)m->adj_hh.p; l.l.out = w.l2; l.l.groups = 1;
    if ((rc = k->launch_bilstm_seq(l, s)) != AMTX_OK) return rc;
    g = gemm_args(w.l2, m->dim_lm, at, m->adj_out, pl, w.mp, m->n_out, AMTX_T_F32, R, 1, 0, 0);
    if ((rc = k->launch_gemm(g, s)) != AMTX_OK) return rc;

    // piano rolls, every track's (n_out, L_t) map contiguous at element n_out row0_t
    if (out_onsets && (rc = amtx_launch_pianoroll_seq((const float*)w.joint, m->dim_aj, 0, seqs_dev, num_seqs, max_len, m->n_out, 0.5f, out_onsets, s)) != AMTX_OK) return rc;
    if (out_offsets && (rc = amtx_launch_pianoroll_seq((const float*)w.joint, m->dim_aj, m->n_out, seqs_dev, num_seqs, max_len, m->n_out, -1.0f, out_offsets, s)) != AMTX_OK) return rc;
    if (out_multi_pitch && (rc = amtx_launch_pianoroll_seq((const float*)w.mp, m->n_out, 0, seqs_dev, num_seqs, max_len, m->n_out, 0.5f, out_multi_pitch, s)) != AMTX_OK) return rc;
    // optional raw logits, packed (R, n_out)
    if (logits_onsets) AMTX_CHECK_HIP(hipMemcpy2DAsync(logits_onsets, row, w.joint, (size_t)m->dim_aj * 4, row, R, hipMemcpyDeviceToDevice, s));
    if (logits_offsets) AMTX_CHECK_HIP(hipMemcpy2DAsync(logits_offsets, row, w.joint + row, (size_t)m->dim_aj * 4, row, R, hipMemcpyDeviceToDevice, s));
    if (logits_multi_pitch) AMTX_CHECK_HIP(hipMemcpyAsync(logits_multi_pitch, w.mp, row * R, hipMemcpyDeviceToDevice, s));
    return AMTX_OK;
}

extern "C" int amtx_of_num_stages(void) { return ST_COUNT; }
extern "C" const char* amtx_of_stage_name(int i) { return (i >= 0 && i < ST_COUNT) ? kStageNames[i] : ""; }

extern "C" int amtx_of_profile_enable(amtx_of_model* m, int enable) {
    AMTX_REQUIRE(m, "amtx_of_profile_enable: null model");
    for (auto& v : m->prof_events)
        for (hipEvent_t e : v) (void)hipEventDestroy(e);
    m->prof_events.clear();
    m->prof = enable != 0;
    return AMTX_OK;
}

// Sum of per-stage durations (ms) over all forwards since profiling was enabled; waits for them to finish.
extern "C" int amtx_of_profile_read(amtx_of_model* m, double* stage_ms, int* num_forwards) {
    AMTX_REQUIRE(m && stage_ms && num_forwards, "amtx_of_profile_read: null argument");
    for (int i = 0; i < ST_COUNT; ++i) stage_ms[i] = 0.0;
    *num_forwards = 0;
    for (auto& v : m->prof_events) {
        if ((int)v.size() != ST_COUNT + 1) continue;
        AMTX_CHECK_HIP(hipEventSynchronize(v.back()));
        for (int i = 0; i < ST_COUNT; ++i) {
            float ms = 0.f;
            AMTX_CHECK_HIP(hipEventElapsedTime(&ms, v[i], v[i + 1]));
            stage_ms[i] += ms;
        }
        ++*num_forwards;
    }
    return AMTX_OK;
}
