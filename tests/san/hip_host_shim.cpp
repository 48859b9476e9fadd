// TEST INFRASTRUCTURE ONLY (tests/test_sanitized_host.py): host-memory stand-ins for the handful of HIP runtime entry points that the
// HOST halves of amt_tools_amd/csrc call, linked into the AddressSanitizer / UBSan build of those host halves (libamtx_san.so, CPU only,
// never shipped, never loaded by the product).  "Device" allocations are plain heap blocks -- so every byte the weight packers, plan
// builders and amtx_of_model_finalize upload is written through instrumented code into instrumented memory -- and a kernel launch
// reports hipErrorNoDevice, which the library turns into its ordinary error return.  Between amtx_san_trace_begin and
// amtx_san_trace_take a launch is RECORDED instead (kernel name, grid, block, dynamic LDS bytes) and reports success, so the host code
// behind it runs on: tests/san/driver.py pins with it which kernels a forward pass launches, in which geometry.  Nothing executes.
#include <hip/hip_runtime.h>
#include <cxxabi.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>

// host stub -> kernel name, filled by the objects' registration constructors while the library loads
static std::map<const void*, std::string>& kernel_names() { static std::map<const void*, std::string> m; return m; }
static bool g_tracing = false;
static std::string g_trace, g_trace_taken;

extern "C" {
static hipError_t g_last = hipSuccess;
hipError_t hipMalloc(void** p, size_t n) { *p = malloc(n ? n : 1); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipFree(void* p) { free(p); return hipSuccess; }
// every host -> "device" upload (its length, then its bytes) goes into one FNV-1a hash: tests/san/driver.py pins the packed weights with it
static uint64_t g_up_hash = 0xcbf29ce484222325ull;
static void up_hash(const void* s, size_t n) {
    for (size_t i = 0; i < 8; ++i) g_up_hash = (g_up_hash ^ ((n >> (8 * i)) & 0xff)) * 0x100000001b3ull;
    for (size_t i = 0; i < n; ++i) g_up_hash = (g_up_hash ^ ((const unsigned char*)s)[i]) * 0x100000001b3ull;
}
uint64_t amtx_san_upload_hash_take(void) { const uint64_t h = g_up_hash; g_up_hash = 0xcbf29ce484222325ull; return h; }   // reads and restarts the hash
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind k) {
    if (k == hipMemcpyHostToDevice) up_hash(s, n);
    memcpy(d, s, n);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t) { memcpy(d, s, n); return hipSuccess; }
hipError_t hipMemcpy2DAsync(void* d, size_t dp, const void* s, size_t sp, size_t w, size_t h, hipMemcpyKind, hipStream_t) {
    for (size_t i = 0; i < h; ++i) memcpy((char*)d + i * dp, (const char*)s + i * sp, w);
    return hipSuccess;
}
hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t) { memset(d, v, n); return hipSuccess; }
hipError_t hipGetDevice(int* d) { *d = 0; return hipSuccess; }
hipError_t hipDeviceSynchronize(void) { return hipSuccess; }
hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int) { return hipSuccess; }
hipError_t hipLaunchKernel(const void* f, dim3 g, dim3 b, void**, size_t lds, hipStream_t) {
    if (!g_tracing) { g_last = hipErrorNoDevice; return hipErrorNoDevice; }
    const auto it = kernel_names().find(f);
    g_trace += (it == kernel_names().end() ? std::string("?") : it->second) + '\t' + std::to_string(g.x) + ' ' + std::to_string(g.y) + ' ' + std::to_string(g.z) + ' ' +
               std::to_string(b.x) + ' ' + std::to_string(b.y) + ' ' + std::to_string(b.z) + ' ' + std::to_string(lds) + '\n';
    return hipSuccess;
}
// launch recording: begin; take = the launches since begin, one line each (name, tab, grid x y z, block x y z, LDS bytes), and end
void amtx_san_trace_begin(void) { g_tracing = true; g_trace.clear(); }
const char* amtx_san_trace_take(void) { g_tracing = false; g_trace_taken.swap(g_trace); g_trace.clear(); return g_trace_taken.c_str(); }
hipError_t hipGetLastError(void) { hipError_t e = g_last; g_last = hipSuccess; return e; }
const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "success" : "no device (sanitizer build: host halves only)"; }
hipError_t hipEventCreate(hipEvent_t*) { return hipErrorNoDevice; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipErrorNoDevice; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipErrorNoDevice; }
hipError_t hipEventElapsedTime(float*, hipEvent_t, hipEvent_t) { return hipErrorNoDevice; }
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
// kernel registration of the host-only objects: only the names are kept
void** __hipRegisterFatBinary(const void*) { static void* h; return &h; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* stub, char*, const char* name, unsigned, void*, void*, void*, void*, int*) {
    int st = 1;
    char* d = abi::__cxa_demangle(name, nullptr, nullptr, &st);
    kernel_names()[stub] = st == 0 ? d : name;
    free(d);
}
void __hipRegisterVar(void**, void*, char*, const char*, int, size_t, int, int) {}
static dim3 g_grid, g_block; static size_t g_shmem; static hipStream_t g_stream;
hipError_t __hipPushCallConfiguration(dim3 g, dim3 b, size_t sh, hipStream_t s) { g_grid = g; g_block = b; g_shmem = sh; g_stream = s; return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3* g, dim3* b, size_t* sh, hipStream_t* s) { *g = g_grid; *b = g_block; *sh = g_shmem; *s = g_stream; return hipSuccess; }
}
