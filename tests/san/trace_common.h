// TEST INFRASTRUCTURE ONLY: what the stand-alone launch-trace programs (frontend_trace.cpp, train_trace.cpp) share.  Each is linked with the
// sanitizer build of the library's host halves and tests/san/hip_host_shim.cpp: nothing executes, a launch is recorded by the shim.
#pragma once
#include "../../include/amtx.h"

#include <sys/mman.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

extern "C" void amtx_san_trace_begin(void);
extern "C" const char* amtx_san_trace_take(void);

namespace {

// address space of `bytes` bytes, 4096-byte aligned; pages exist only where something writes
struct Reserved {
    void* p = nullptr;
    size_t n = 0;
    explicit Reserved(size_t bytes) : n(std::max<size_t>(bytes, 4096)) {
        p = mmap(nullptr, n, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (p == MAP_FAILED) { perror("mmap"); exit(2); }
    }
    ~Reserved() { munmap(p, n); }
    Reserved(const Reserved&) = delete;
    Reserved& operator=(const Reserved&) = delete;
};

// one case's row: "=<tab>return code<tab>error text", the values an entry point answered (`extra`: lines of a name, a tab, numbers), then
// one line per launch as the shim recorded it
void report(long long rc, bool failed, const std::string& extra = std::string()) {
    const std::string trace = amtx_san_trace_take();
    std::cout << "=\t" << rc << '\t' << (failed ? amtx_last_error() : "") << '\n' << extra << trace;
}

}  // namespace
