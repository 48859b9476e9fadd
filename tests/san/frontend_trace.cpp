// TEST INFRASTRUCTURE ONLY (tests/test_frontend_trace.py): which kernels the front-end's entry points (spec.hip, cqt.hip, cqt_dec.hip and the
// GEMM route of gemm.hip) launch, in which grid, block and dynamic LDS size, or the error they answer.  A stand-alone program linked with the
// sanitizer build of the library's host halves and tests/san/hip_host_shim.cpp: nothing executes, a launch is recorded by the shim.
//
//   frontend_trace CASES        one case per line of CASES (tests/san/frontend_trace.py writes it):
//     spec <entry> sr n_fft hop n_mels center pad_mode batch x          entry: power (x = samples) | power_clips (x = frames) | mel_layout
//     cqt  <entry> lib09 truncate sr hop fmin n_bins bpo gamma nh h.. batch n
//          entry: forward | forward16 | forward16_split | forward_small_ws | track_layout | pyramid_build | power_clips | clips | clips16 |
//                 clips16_split | clips_small_ws | workspace_bytes | clips_workspace_bytes | num_frames
//   per case on stdout: "=<tab>return code<tab>error text", then one line per launch as the shim records it (values an entry point answers
//   through pointers are printed the same way: a name, a tab, numbers).
// Buffers the host code only takes addresses of are reserved address space (never touched, never committed); what it writes -- clip_max, the
// maxima, the workspace's maxima and the host track table -- is real memory.
#include "trace_common.h"
#include "../../include/amtx_pyramid.h"
#include "../../include/amtx_tracks.h"

#include <fstream>
#include <map>
#include <sstream>
#include <vector>

namespace {

std::map<std::string, amtx_spec_plan*> spec_plans;
std::map<std::string, amtx_cqt_plan*> cqt_plans;

void spec_case(std::istringstream& in) {
    std::string entry;
    int sr, n_fft, hop, n_mels, center, pad_mode, batch;
    long long x;
    in >> entry >> sr >> n_fft >> hop >> n_mels >> center >> pad_mode >> batch >> x;
    if (!in) { std::cerr << "bad spec case\n"; exit(2); }
    if (entry == "mel_layout") {
        std::vector<int32_t> row(64 * 8), start(64 * 8), rmax(8);
        amtx_san_trace_begin();
        const int rounds = amtx_spec_mel_layout(sr, n_fft, n_mels, 0, row.data(), start.data(), rmax.data());
        std::ostringstream o;
        if (rounds > 0) {
            int slots = 0;
            for (int r = 0; r < rounds; ++r) slots += rmax[r];
            o << "mel_layout\t" << slots;
            for (int r = 0; r < rounds; ++r) o << ' ' << rmax[r];
            o << '\n';
        }
        return report(rounds, rounds < 0, o.str());
    }
    std::ostringstream key;
    key << sr << ' ' << n_fft << ' ' << hop << ' ' << n_mels << ' ' << center << ' ' << pad_mode;
    amtx_spec_plan*& plan = spec_plans[key.str()];
    if (!plan) {
        amtx_san_trace_begin();
        const int rc = amtx_spec_plan_create(&plan, sr, n_fft, hop, n_fft, n_mels, 0, center, pad_mode);
        if (rc != AMTX_OK) return report(rc, true);
        (void)amtx_san_trace_take();
    }
    std::vector<float> clip_max((size_t)batch);
    Reserved audio(4096), out(4096);
    amtx_san_trace_begin();
    int rc;
    if (entry == "power") rc = amtx_spec_power(plan, (const float*)audio.p, x, x, batch, (float*)out.p, clip_max.data(), nullptr);
    else if (entry == "power_clips") rc = amtx_spec_power_clips(plan, (const float*)audio.p, (const int64_t*)out.p, batch, x, (float*)out.p, clip_max.data(), nullptr);
    else { std::cerr << "bad spec entry " << entry << '\n'; exit(2); }
    report(rc, rc != AMTX_OK);
}

void cqt_case(std::istringstream& in) {
    std::string entry;
    int lib09, truncate, sr, hop, n_bins, bpo, nh, batch;
    double fmin, gamma;
    long long n;
    in >> entry >> lib09 >> truncate >> sr >> hop >> fmin >> n_bins >> bpo >> gamma >> nh;
    std::vector<double> harm((size_t)std::max(nh, 0));
    for (double& h : harm) in >> h;
    in >> batch >> n;
    if (!in) { std::cerr << "bad cqt case\n"; exit(2); }
    std::ostringstream key;
    key.precision(17);
    key << lib09 << ' ' << truncate << ' ' << sr << ' ' << hop << ' ' << fmin << ' ' << n_bins << ' ' << bpo << ' ' << gamma;
    for (double h : harm) key << ' ' << h;
    amtx_cqt_plan*& plan = cqt_plans[key.str()];
    if (!plan) {
        amtx_san_trace_begin();
        const int rc = amtx_cqt_plan_create(&plan, sr, hop, fmin, n_bins, bpo, gamma, harm.data(), nh, truncate, lib09);
        if (rc != AMTX_OK) return report(rc, true);
        (void)amtx_san_trace_take();
    }
    if (entry == "workspace_bytes" || entry == "clips_workspace_bytes" || entry == "num_frames") {
        amtx_san_trace_begin();
        const long long v = entry == "num_frames" ? (long long)amtx_cqt_num_frames(plan, n)
                            : entry == "workspace_bytes" ? (long long)amtx_cqt_workspace_bytes(plan, batch, n) : (long long)amtx_cqt_clips_workspace_bytes(plan, batch, n);
        return report(v, false);
    }
    Reserved audio(4096), out(4096);
    if (entry.compare(0, 7, "forward") == 0) {
        const size_t need = amtx_cqt_workspace_bytes(plan, batch, n), have = entry == "forward_small_ws" ? need - 256 : need;
        Reserved ws(need);
        amtx_san_trace_begin();
        int rc;
        if (entry == "forward" || entry == "forward_small_ws") rc = amtx_cqt_forward(plan, (const float*)audio.p, n, n, batch, 1, ws.p, have, (float*)out.p, nullptr);
        else if (entry == "forward16") rc = amtx_cqt_forward16(plan, (const float*)audio.p, n, n, batch, 1, ws.p, have, out.p, nullptr);
        else if (entry == "forward16_split") rc = amtx_cqt_forward16_split(plan, (const float*)audio.p, n, n, batch, 1, ws.p, have, out.p, 1 << 20, nullptr);
        else { std::cerr << "bad cqt entry " << entry << '\n'; exit(2); }
        return report(rc, rc != AMTX_OK);
    }
    int64_t len[16], stride[16], rows[16], frames = 0;
    if (entry == "track_layout") {
        amtx_san_trace_begin();
        const int nl = amtx_cqt_track_layout(plan, n, len, stride, rows, &frames);
        std::ostringstream o;
        if (nl >= 0) {
            o << "track_layout\t" << frames;
            for (int l = 0; l < nl; ++l) o << ' ' << len[l] << ' ' << stride[l];
            for (int h = 0; h < nh; ++h) o << ' ' << rows[h];
            o << '\n';
        }
        return report(nl, nl < 0, o.str());
    }
    if (entry == "pyramid_build") {
        // `batch` tracks of n, n + hop + 1, n + 2 (hop + 1), n, ... samples (three lengths in turn: the launches of a large bank repeat with a short
        // period, which the golden file folds), laid out one after another the way amt_tools_amd/tracks.py does
        const int cols = amtx_cqt_track_cols(plan);
        std::vector<int64_t> tab((size_t)batch * cols);
        int64_t audio_elems = 0, pyr_elems = 0;
        amtx_san_trace_begin();
        for (int t = 0; t < batch; ++t) {
            const int64_t nt = n + (int64_t)(t % 3) * (hop + 1);
            const int nl = amtx_cqt_track_layout(plan, nt, len, stride, rows, &frames);
            if (nl < 0) return report(nl, true);
            int64_t* tr = tab.data() + (size_t)t * cols;
            tr[0] = audio_elems; tr[1] = nt; tr[3] = frames; tr[2] = 0;
            audio_elems += (nt + 3) / 4 * 4;
            for (int l = 0; l < nl; ++l) {
                tr[4 + 3 * l] = pyr_elems; tr[4 + 3 * l + 1] = len[l]; tr[4 + 3 * l + 2] = stride[l];
                pyr_elems += (stride[l] + 3) / 4 * 4;
            }
            for (int h = 0; h < nh; ++h) { tr[4 + 3 * nl + h] = rows[h]; tr[2] = std::max(tr[2], rows[h]); }
        }
        std::vector<float> maxima((size_t)batch * nh);
        const int rc = amtx_cqt_pyramid_build(plan, (const float*)audio.p, audio_elems, tab.data(), (const int64_t*)out.p, batch, (float*)out.p, std::max<int64_t>(pyr_elems, 1),
                                              maxima.data(), nullptr);
        return report(rc, rc != AMTX_OK);
    }
    // the clip forms: `batch` clips of as many frames as a clip of n samples has
    const int64_t nf = std::max<int64_t>(amtx_cqt_num_frames(plan, n), 1);
    const size_t need = amtx_cqt_clips_workspace_bytes(plan, batch, nf), have = entry == "clips_small_ws" ? need - 256 : need;
    Reserved ws(need);
    const float* a = (const float*)audio.p;
    const int64_t* t = (const int64_t*)out.p;
    amtx_san_trace_begin();
    int rc;
    if (entry == "power_clips") rc = amtx_cqt_power_clips(plan, a, a, t, t, batch, nf, (float*)out.p, nullptr);
    else if (entry == "clips" || entry == "clips_small_ws") rc = amtx_cqt_clips(plan, a, a, t, t, batch, nf, a, 1, ws.p, have, (float*)out.p, nullptr);
    else if (entry == "clips16") rc = amtx_cqt_clips16(plan, a, a, t, t, batch, nf, a, 1, ws.p, have, out.p, nullptr);
    else if (entry == "clips16_split") rc = amtx_cqt_clips16_split(plan, a, a, t, t, batch, nf, a, 1, ws.p, have, out.p, 1 << 20, nullptr);
    else { std::cerr << "bad cqt entry " << entry << '\n'; exit(2); }
    report(rc, rc != AMTX_OK);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { std::cerr << "usage: frontend_trace CASES\n"; return 2; }
    std::ifstream f(argv[1]);
    if (!f) { std::cerr << "cannot read " << argv[1] << '\n'; return 2; }
    std::string line;
    while (std::getline(f, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string family;
        in >> family;
        if (family == "spec") spec_case(in);
        else if (family == "cqt") cqt_case(in);
        else { std::cerr << "bad case: " << line << '\n'; return 2; }
    }
    for (auto& kv : spec_plans) amtx_spec_plan_destroy(kv.second);
    for (auto& kv : cqt_plans) amtx_cqt_plan_destroy(kv.second);
    std::cout << "done\n";
    return 0;
}
