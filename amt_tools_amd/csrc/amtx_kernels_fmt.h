// Everything that conv.hip, convf.hip, convg.hip, gemm.hip, lstm.hip and pack.hip define: the functions that exist once per 16-bit operand
// format (amtx_common.h: AMTX_FMT_NS).  No include guard: amtx_kernels.h includes this file inside namespace amtx_bf16 and, in a library
// with the half-operand twins, once more inside namespace amtx_f16 -- same arguments and layouts, packed weights and 16-bit activations
// hold IEEE half there.  The argument structs are amtx_kernels.h's, shared by both.

// ---------------------------------------------------------------- gemm.hip
bool amtx_gemm_has_roll_epilogue(const GemmArgs& g);
int amtx_launch_gemm(const GemmArgs& g, hipStream_t stream);
// several fp32-A / fp32-C / two-plane problems with one group count in one launch (generic 128 x 128 kernel)
int amtx_launch_gemm_multi(const GemmArgs* gs, int n, hipStream_t stream);
void amtx_gemm_pack_dims(int N, int K, int* n_pad, int* k_pad);
// host packing: W (N x K fp32 row-major, leading dim ldw) -> [planes][n_pad][k_pad] bf16
void amtx_gemm_pack_host(const float* W, int64_t ldw, int N, int K, int planes, bf16_t* out);

// ---------------------------------------------------------------- conv.hip
int amtx_launch_conv3x3(const ConvArgs& c, hipStream_t stream);
size_t amtx_conv1_wfrag_elems(int c_in, int planes);
// host packing of the fused first conv: weight (32, c_in, 3, 3) fp32 * scale[32] -> fragment order
void amtx_conv1_pack_host(const float* w, const float* scale, int c_in, int planes, bf16_t* out);
size_t amtx_conv3x3_wfrag_elems(int c_out, int planes);
// host packing: weight (c_out, 32, 3, 3) fp32 * scale[c_out] -> fragment order
void amtx_conv3x3_pack_host(const float* w, const float* scale, int c_out, int planes, bf16_t* out);
int amtx_launch_conv1(const Conv1Args& c, hipStream_t stream);

// ---------------------------------------------------------------- convf.hip
// the whole stack layer1 -> layer2 -> layer3 of a one-channel, 32/32/64-channel, bf16 model in one kernel: `c2` as for
// amtx_launch_conv3x3 with the fused first conv (feats, w1frag, shift1, wfrag, shift; `out` ignored), plus layer3's packed weights and
// shift; out = [groups][B][T][F / 4][64] bf16.  amtx_conv_stack_fused_ok: the batch is large enough for its one-strip-per-CU granularity.
bool amtx_conv_stack_fused_ok(int B, int T, int F, int groups);
int amtx_launch_conv_stack(const ConvArgs& c2, const bf16_t* w3frag, int64_t w3_gs, const float* shift3, void* out, int64_t out_gs,
                           int64_t out_plane, hipStream_t stream);

// ---------------------------------------------------------------- convg.hip
// general channel counts: C_in a multiple of 16, weights staged in LDS per C_out chunk; `a.in` is [B][T][F][c_in]
int amtx_conv3x3_gen_ntc(int c_in, int c_out);           // 0 = this pair of channel counts is not built
size_t amtx_conv3x3_gen_wfrag_elems(int c_in, int c_out, int planes);
void amtx_conv3x3_gen_pack_host(const float* w /*(c_out,c_in,3,3)*/, const float* scale, int c_in, int c_out, int planes, bf16_t* out);
int amtx_launch_conv3x3_gen(const ConvArgs& c, int c_in, hipStream_t stream);
// fused first conv of the general kernel (ConvArgs.feats / c_in / w1frag / shift1 as for conv.hip; `c_in` above = its output channels),
// in one of two K orders: amtx_conv1g_tapk (amtx_kernels.h)
size_t amtx_conv1g_wfrag_elems(int c_in, int c_mid, int planes);
void amtx_conv1g_pack_host(const float* w /*(c_mid,c_in,3,3)*/, const float* scale, int c_in, int c_mid, int planes, bf16_t* out);
bool amtx_conv3x3_gen_can_fuse1(int c_in, int c_mid, int c_out, int planes);

// ---------------------------------------------------------------- lstm.hip: hidden = 128, 256, 384 or 512 per direction
int amtx_launch_bilstm(const LstmArgs& l, hipStream_t stream);
int amtx_launch_bilstm_seq(const LstmSeqArgs& l, hipStream_t stream);   // packed sequences: (1 plane, 16-bit rows) or (2 planes, fp32 rows)
size_t amtx_bilstm_wfrag_elems(int hidden, int planes);  // per LSTM (both directions)
void amtx_bilstm_pack_host(const float* whh_fwd, const float* whh_bwd, int hidden, int planes, bf16_t* out);   // each (4 hidden, hidden)
// training: device-side packing of fp32 W_hh into forward + transposed (backward) fragments; backward recurrence -> dL/d(xproj) of
// `groups` independent LSTMs of the same (B, T) (hidden 256 / 384 / 512: two planes only)
int amtx_launch_bilstm_pack_dev(const float* whh_fwd, const float* whh_bwd, int hidden, int planes, bf16_t* frag_fwd, bf16_t* frag_bwd, hipStream_t stream);
int amtx_launch_bilstm_bwd(const float* dout, const float* save, const bf16_t* whh_t, int hidden, int planes, float* dxproj, int B, int T, int groups,
                           hipStream_t stream);

// ---------------------------------------------------------------- pack.hip: device-side weight packing, kernels over the layouts of
// amtx_pack_layouts.h, which the host packers loop over too, for a weight re-sync that does not leave the GPU (amtx_of_model_finalize_device)
int amtx_pack_bn_fold_dev(const float* conv_bias, const float* gamma, const float* beta, const float* mean, const float* var, int c_out, float* scale,
                          float* shift, hipStream_t s);
int amtx_pack_conv3x3_dev(const float* w, const float* scale, int c_out, int planes, bf16_t* out, hipStream_t s);
int amtx_pack_conv1_dev(const float* w, const float* scale, int planes, bf16_t* out, hipStream_t s);
int amtx_pack_conv_gen_dev(const float* w, const float* scale, int c_in, int c_out, int ntc, int planes, bf16_t* out, hipStream_t s);
int amtx_pack_conv1g_dev(const float* w, const float* scale, int c_in, int c_mid, int planes, bf16_t* out, hipStream_t s);
int amtx_pack_scale_rows_dev(const float* w, const float* scale, int rows, int cols, float* out, hipStream_t s);
int amtx_pack_linear_dev(const float* W, int64_t ldw, int N, int K, int planes, int n_pad, int k_pad, int row0, int rows_owned, int perm_c, int perm_f,
                         bf16_t* out, hipStream_t s);
void amtx_pack_linear_host(const float* W, int64_t ldw, int N, int K, int planes, int n_pad, int k_pad, int row0, int rows_owned, int perm_c, int perm_f,
                           bf16_t* out);      // the same rows on the host (amtx_gemm_pack_host: all of them)
int amtx_pack_head_fold_dev(const float* w_out, const float* w_fc1, const float* b_fc1, const float* b_out, int n_out, int dim_am, int kfc, int kfc_pad,
                            int nf3, int fq, float* wfold, float* bfold, hipStream_t s);
int amtx_pack_vec_add_dev(const float* a, const float* b, int n, float* out, hipStream_t s);
