// TEST INFRASTRUCTURE ONLY (tests/test_train_trace.py): which kernels the training step's dense entry points (train.hip) launch, in which grid,
// block and dynamic LDS size, the error they answer, and what their workspace queries return.  A stand-alone program linked with the sanitizer
// build of the library's host halves and tests/san/hip_host_shim.cpp: nothing executes, a launch is recorded by the shim.
//
//   train_trace CASES        one case per line of CASES (tests/san/train_trace.py writes it):
//     matmul     m n k a_trans b_trans bias ldc_pad ws flaw       flaw: ok | null_a | null_c | odd_a | odd_b | lda | ldb
//     linear_fwd m n k bias ldy_pad
//     linear_bwd m n k mask lddy_pad ws flaw                      mask: 1 dx + 2 dw + 4 db;  flaw: ok | null_dy | no_w | no_x
//     conv_fwd   rows T F c_in c_out bias ws
//     conv_bwd   rows T F c_in c_out mask ws flaw                 flaw: ok | no_w | no_x
//   ws, with `need` the answer of the entry point's workspace query: null | exact (need bytes) | exact-N (N bytes short of it, at least 0) |
//     =N (N bytes) | atleast=N (max(need, N)).  ldc_pad / ldy_pad / lddy_pad: what the leading dimension has more than the row length.
//   per case on stdout: "=<tab>return code<tab>error text", "<query><tab>need" where the entry point has a query, then one line per launch.
// Operands are reserved address space the host code only takes addresses of (never touched, never committed).
#include "trace_common.h"

#include <fstream>
#include <sstream>

namespace {

struct Workspace {
    Reserved mem;
    void* p;
    size_t bytes;
    Workspace(size_t have, bool null) : mem(have), p(null ? nullptr : mem.p), bytes(null ? 0 : have) {}
};

size_t ws_bytes(const std::string& mode, size_t need) {
    if (mode == "null") return 0;
    if (mode == "exact") return need;
    if (mode.compare(0, 6, "exact-") == 0) return need - std::min<size_t>(need, std::stoull(mode.substr(6)));
    if (mode.compare(0, 1, "=") == 0) return std::stoull(mode.substr(1));
    if (mode.compare(0, 8, "atleast=") == 0) return std::max<size_t>(need, std::stoull(mode.substr(8)));
    std::cerr << "bad workspace mode " << mode << '\n';
    exit(2);
}

std::string query_line(const char* name, size_t need) { return std::string(name) + '\t' + std::to_string(need) + '\n'; }

void bad(const char* what) { std::cerr << "bad " << what << " case\n"; exit(2); }

void run_case(const std::string& entry, std::istringstream& in) {
    Reserved buf(4096);
    float* const p = (float*)buf.p;
    if (entry == "matmul") {
        long long m, n, k, ldc_pad;
        int at, bt, bias;
        std::string ws, flaw;
        in >> m >> n >> k >> at >> bt >> bias >> ldc_pad >> ws >> flaw;
        if (!in) bad("matmul");
        // the query is asked about problems the entry point takes: at the recorded commit it divided by the tile count of an empty one
        const size_t need = m > 0 && n > 0 && k > 0 ? amtx_matmul_workspace_bytes(m, n, k) : 0;
        Workspace w(ws_bytes(ws, need), ws == "null");
        const float* a = flaw == "null_a" ? nullptr : flaw == "odd_a" ? p + 1 : p;
        const float* b = flaw == "odd_b" ? p + 1 : p;
        // leading dimensions: the contiguous extent rounded up to a multiple of 4 (an extent that is none is refused for itself)
        const int64_t lda = ((at ? m : k) + 3) / 4 * 4 + (flaw == "lda" ? 2 : 0), ldb = ((bt ? n : k) + 3) / 4 * 4 + (flaw == "ldb" ? 2 : 0);
        amtx_san_trace_begin();
        const int rc = amtx_matmul_f32(a, lda, at, b, ldb, bt, bias ? p : nullptr, flaw == "null_c" ? nullptr : p, n + ldc_pad, m, n, k, w.p, w.bytes, nullptr);
        return report(rc, rc != AMTX_OK, query_line("matmul_workspace_bytes", need));
    }
    if (entry == "linear_fwd") {
        long long m, ldy_pad;
        int n, k, bias;
        in >> m >> n >> k >> bias >> ldy_pad;
        if (!in) bad("linear_fwd");
        amtx_san_trace_begin();
        const int rc = amtx_linear_train_fwd(p, k, p, k, bias ? p : nullptr, p, n + ldy_pad, m, n, k, nullptr);
        return report(rc, rc != AMTX_OK);
    }
    if (entry == "linear_bwd") {
        long long m, lddy_pad;
        int n, k, mask;
        std::string ws, flaw;
        in >> m >> n >> k >> mask >> lddy_pad >> ws >> flaw;
        if (!in) bad("linear_bwd");
        const size_t need = amtx_linear_bwd_workspace_bytes(m, n, k);
        Workspace w(ws_bytes(ws, need), ws == "null");
        amtx_san_trace_begin();
        const int rc = amtx_linear_bwd(flaw == "null_dy" ? nullptr : p, n + lddy_pad, flaw == "no_x" ? nullptr : p, k, flaw == "no_w" ? nullptr : p, k, mask & 1 ? p : nullptr, k,
                                       mask & 2 ? p : nullptr, mask & 4 ? p : nullptr, m, n, k, w.p, w.bytes, nullptr);
        return report(rc, rc != AMTX_OK, query_line("linear_bwd_workspace_bytes", need));
    }
    if (entry == "conv_fwd" || entry == "conv_bwd") {
        long long rows;
        int T, F, c_in, c_out, x;                     // x: bias (forward) or mask (backward)
        std::string ws, flaw = "ok";
        in >> rows >> T >> F >> c_in >> c_out >> x >> ws;
        if (entry == "conv_bwd") in >> flaw;
        if (!in) bad("conv");
        const size_t need = amtx_conv3x3_train_workspace_bytes(rows, F, c_in, c_out);
        Workspace w(ws_bytes(ws, need), ws == "null");
        amtx_san_trace_begin();
        const int rc = entry == "conv_fwd" ? amtx_conv3x3_train_fwd(p, p, x ? p : nullptr, p, rows, T, F, c_in, c_out, w.p, w.bytes, nullptr)
                                           : amtx_conv3x3_bwd(p, flaw == "no_x" ? nullptr : p, flaw == "no_w" ? nullptr : p, x & 1 ? p : nullptr, x & 2 ? p : nullptr,
                                                              x & 4 ? p : nullptr, rows, T, F, c_in, c_out, w.p, w.bytes, nullptr);
        return report(rc, rc != AMTX_OK, query_line("conv3x3_train_workspace_bytes", need));
    }
    std::cerr << "bad entry " << entry << '\n';
    exit(2);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { std::cerr << "usage: train_trace CASES\n"; return 2; }
    std::ifstream f(argv[1]);
    if (!f) { std::cerr << "cannot read " << argv[1] << '\n'; return 2; }
    std::string line;
    while (std::getline(f, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string entry;
        in >> entry;
        run_case(entry, in);
    }
    std::cout << "done\n";
    return 0;
}
