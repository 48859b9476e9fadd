// Packed rows (include/amtx_ofseq.h): the sequence table's check, the kept rows of a clip batch into packed rows, the piano rolls of packed
// rows, and the packed-sequence BiLSTM's entry point (its kernels: lstm.hip).
//
// rows_gather: byte work, 16 bytes per lane and trip; a block column (blockIdx.y) owns one clip, blockIdx.z the plane; rows are contiguous on
// both sides, so consecutive lanes read and write consecutive 16-byte pieces.  No LDS, no atomics, no workspace.
// pianoroll_seq: head.hip's 32 x 32 LDS transpose per sequence, the sequence's own length as the map's width.
#include "amtx_kernels.h"
#include "../../include/amtx_ofseq.h"

#include <algorithm>
#include <utility>
#include <vector>

namespace {

__global__ __launch_bounds__(256) void rows_gather_kernel(const char* __restrict__ src, int64_t clip_bytes, int w16, int64_t src_plane,
                                                          const int64_t* __restrict__ table, char* __restrict__ dst, int64_t dst_plane) {
    const int64_t* d = table + 3 * (int64_t)blockIdx.y;              // {src_first, count, dst_row}
    const int64_t n = d[1] * w16;
    const uint4* from = reinterpret_cast<const uint4*>(src + blockIdx.z * src_plane + blockIdx.y * clip_bytes) + d[0] * w16;
    uint4* to = reinterpret_cast<uint4*>(dst + blockIdx.z * dst_plane) + d[2] * w16;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) to[i] = from[i];
}

__global__ __launch_bounds__(256) void pianoroll_seq_kernel(const float* __restrict__ logits, int64_t ld, int col0, const int64_t* __restrict__ seqs,
                                                            int keys, float threshold, float* __restrict__ out) {
    __shared__ float tile[32][33];
    const int64_t row0 = seqs[2 * (int64_t)blockIdx.z], T = seqs[2 * (int64_t)blockIdx.z + 1];
    const int64_t t0 = (int64_t)blockIdx.x * 32;
    if (t0 >= T) return;                                             // block-uniform, before the barrier
    const int k0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t t = t0 + ty + 8 * i;
        const int k = k0 + tx;
        float v = 0.f;
        if (t < T && k < keys) {
            const float x = logits[(row0 + t) * ld + col0 + k];
            const float s = 1.0f / (1.0f + expf(-x));                // torch.sigmoid in fp32, as pianoroll_kernel
            v = threshold < 0.f ? s : (s < threshold ? 0.f : 1.f);
        }
        tile[ty + 8 * i][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = k0 + ty + 8 * i;
        const int64_t t = t0 + tx;
        if (t < T && k < keys) out[keys * row0 + k * T + t] = tile[tx][ty + 8 * i];
    }
}

}  // namespace

int amtx_check_seq_table(const char* who, const int64_t* seqs_host, int num_seqs, int64_t total_rows, int64_t* max_len) {
    AMTX_REQUIRE(seqs_host, "%s: the host copy of the sequence table is null", who);
    AMTX_REQUIRE(num_seqs >= 1 && total_rows >= 1, "%s: num_seqs=%d, total_rows=%lld: at least one each", who, num_seqs, (long long)total_rows);
    std::vector<std::pair<int64_t, int>> order(num_seqs);
    int64_t longest = 0;
    for (int s = 0; s < num_seqs; ++s) {
        const int64_t row0 = seqs_host[2 * (int64_t)s], len = seqs_host[2 * (int64_t)s + 1];
        AMTX_REQUIRE(len >= 1 && len < 0x7fffffffll, "%s: sequence %d: len=%lld: at least one row (and fewer than 2^31)", who, s, (long long)len);
        AMTX_REQUIRE(row0 >= 0, "%s: sequence %d: row0=%lld is negative", who, s, (long long)row0);
        AMTX_REQUIRE(len <= total_rows && row0 <= total_rows - len, "%s: sequence %d: rows [%lld, %lld + %lld) leave the %lld packed rows", who, s,
                     (long long)row0, (long long)row0, (long long)len, (long long)total_rows);
        order[s] = {row0, s};
        longest = std::max(longest, len);
    }
    std::sort(order.begin(), order.end());
    for (int i = 1; i < num_seqs; ++i) {
        const int p = order[i - 1].second, s = order[i].second;
        AMTX_REQUIRE(order[i - 1].first + seqs_host[2 * (int64_t)p + 1] <= order[i].first, "%s: sequence %d: its rows from %lld on overlap sequence %d", who,
                     std::max(p, s), (long long)seqs_host[2 * (int64_t)std::max(p, s)], std::min(p, s));
    }
    if (max_len) *max_len = longest;
    return AMTX_OK;
}

int amtx_launch_rows_gather(const void* src, int batch, int64_t num_frames, int64_t width_bytes, int planes, int64_t src_plane_bytes,
                            const int64_t* table_host, const int64_t* table_dev, void* dst, int64_t total_rows, int64_t dst_plane_bytes,
                            hipStream_t stream) {
    AMTX_REQUIRE(src && table_host && table_dev && dst, "amtx_rows_gather: null argument");
    AMTX_REQUIRE(batch >= 1 && batch < 65536 && num_frames >= 1 && total_rows >= 1, "amtx_rows_gather: batch=%d, num_frames=%lld, total_rows=%lld: at least one each (batch below 65536)",
                 batch, (long long)num_frames, (long long)total_rows);
    AMTX_REQUIRE(width_bytes >= 16 && width_bytes % 16 == 0 && width_bytes < (1ll << 31), "amtx_rows_gather: width_bytes=%lld: rows are copied 16 bytes at a time", (long long)width_bytes);
    AMTX_REQUIRE(planes == 1 || planes == 2, "amtx_rows_gather: planes must be 1 or 2");
    AMTX_REQUIRE(((uintptr_t)src % 16) == 0 && ((uintptr_t)dst % 16) == 0, "amtx_rows_gather: src and dst must be aligned to 16 bytes");
    AMTX_REQUIRE(planes == 1 || (src_plane_bytes % 16 == 0 && dst_plane_bytes % 16 == 0 && src_plane_bytes >= (int64_t)batch * num_frames * width_bytes &&
                                 dst_plane_bytes >= total_rows * width_bytes),
                 "amtx_rows_gather: a plane stride is a multiple of 16 bytes and at least one plane long");
    int64_t most = 0;
    for (int b = 0; b < batch; ++b) {
        const int64_t* d = table_host + 3 * (int64_t)b;
        AMTX_REQUIRE(d[0] >= 0 && d[1] >= 0 && d[2] >= 0, "amtx_rows_gather: clip %d: a negative entry", b);
        AMTX_REQUIRE(d[1] <= num_frames && d[0] <= num_frames - d[1], "amtx_rows_gather: clip %d: rows [%lld, %lld + %lld) leave the clip's %lld frames", b,
                     (long long)d[0], (long long)d[0], (long long)d[1], (long long)num_frames);
        AMTX_REQUIRE(d[1] <= total_rows && d[2] <= total_rows - d[1], "amtx_rows_gather: clip %d: rows [%lld, %lld + %lld) leave the %lld packed rows", b,
                     (long long)d[2], (long long)d[2], (long long)d[1], (long long)total_rows);
        most = std::max(most, d[1]);
    }
    if (most == 0) return AMTX_OK;
    const int w16 = (int)(width_bytes / 16);
    const dim3 grid((unsigned)std::min<int64_t>((most * w16 + 255) / 256, 1024), (unsigned)batch, (unsigned)planes);
    hipLaunchKernelGGL(rows_gather_kernel, grid, dim3(256), 0, stream, (const char*)src, num_frames * width_bytes, w16, planes == 2 ? src_plane_bytes : 0,
                       table_dev, (char*)dst, planes == 2 ? dst_plane_bytes : 0);
    AMTX_CHECK_LAUNCH();
    return AMTX_OK;
}

int amtx_launch_pianoroll_seq(const float* logits, int64_t ld, int col0, const int64_t* seqs_dev, int num_seqs, int64_t max_len, int keys,
                              float threshold, float* out, hipStream_t stream) {
    AMTX_REQUIRE(logits && seqs_dev && out, "pianoroll_seq: null pointer");
    AMTX_REQUIRE(num_seqs > 0 && num_seqs < 65536 && max_len > 0 && keys > 0, "pianoroll_seq: bad sizes");
    const dim3 grid((unsigned)((max_len + 31) / 32), (unsigned)((keys + 31) / 32), (unsigned)num_seqs);
    hipLaunchKernelGGL(pianoroll_seq_kernel, grid, dim3(256), 0, stream, logits, ld, col0, seqs_dev, keys, threshold, out);
    AMTX_CHECK_LAUNCH();
    return AMTX_OK;
}

extern "C" int amtx_rows_gather(const void* src, int batch, int64_t num_frames, int64_t width_bytes, int planes, int64_t src_plane_bytes,
                                const int64_t* table_host, const int64_t* table_dev, void* dst, int64_t total_rows, int64_t dst_plane_bytes,
                                void* stream) {
    return amtx_launch_rows_gather(src, batch, num_frames, width_bytes, planes, src_plane_bytes, table_host, table_dev, dst, total_rows, dst_plane_bytes,
                                   (hipStream_t)stream);
}

extern "C" int amtx_pianoroll_seq(const float* logits, int64_t ld, int col0, const int64_t* seqs_host, const int64_t* seqs_dev, int num_seqs,
                                  int64_t total_rows, int keys, float threshold, float* out, void* stream) {
    int64_t max_len = 0;
    const int rc = amtx_check_seq_table("amtx_pianoroll_seq", seqs_host, num_seqs, total_rows, &max_len);
    if (rc != AMTX_OK) return rc;
    AMTX_REQUIRE(ld >= 1 && col0 >= 0 && keys >= 1 && col0 + (int64_t)keys <= ld, "amtx_pianoroll_seq: columns [%d, %d + %d) of rows of %lld", col0, col0, keys, (long long)ld);
    return amtx_launch_pianoroll_seq(logits, ld, col0, seqs_dev, num_seqs, max_len, keys, threshold, out, (hipStream_t)stream);
}

extern "C" int amtx_bilstm_seq_fwd(const void* xproj, const uint16_t* whh_packed, int hidden, int planes, int elem_type, void* out,
                                   const int64_t* seqs_host, const int64_t* seqs_dev, int num_seqs, int64_t total_rows, int groups, void* stream) {
    AMTX_REQUIRE(xproj && whh_packed && out && seqs_dev, "amtx_bilstm_seq_fwd: null pointer");
    AMTX_REQUIRE(groups >= 1 && (planes == 1 || planes == 2), "amtx_bilstm_seq_fwd: groups=%d, planes=%d", groups, planes);
    const int rc = amtx_check_seq_table("amtx_bilstm_seq_fwd", seqs_host, num_seqs, total_rows, nullptr);
    if (rc != AMTX_OK) return rc;
    LstmSeqArgs a;
    a.l.xproj = xproj; a.l.x_type = elem_type; a.l.whh = whh_packed; a.l.planes = planes; a.l.out = out; a.l.out_type = elem_type;
    a.l.B = num_seqs; a.l.T = 0; a.l.hidden = hidden; a.l.save = nullptr;
    a.l.groups = groups; a.l.x_gs = total_rows * 8 * hidden; a.l.w_gs = (int64_t)amtx_bilstm_wfrag_elems(hidden, planes); a.l.out_gs = total_rows * 2 * hidden;
    a.seqs = seqs_dev; a.S = num_seqs;
    return amtx_launch_bilstm_seq(a, (hipStream_t)stream);
}
