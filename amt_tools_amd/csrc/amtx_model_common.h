// Host-side plumbing shared by the model engines (ofmodel.hip, tab.hip): device buffers that survive a weight re-sync, the
// state_dict tensor store, the wait before a re-sync, workspace carving.  Host only.
#pragma once
#include "amtx_common.h"

#include <map>
#include <string>
#include <utility>
#include <vector>

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    int upload(const void* host, size_t n) {
        if (!p || bytes != n) {        // a weight re-sync (validate() inside train()) keeps its allocations: same model, same sizes
            if (p) (void)hipFree(p);
            p = nullptr; bytes = n;
            AMTX_CHECK_HIP(hipMalloc(&p, n));
        }
        AMTX_CHECK_HIP(hipMemcpy(p, host, n, hipMemcpyHostToDevice));
        return AMTX_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; }
};

// Tensors handed over under their state_dict names: host copies (set) and borrowed device pointers (set_device, for a re-sync that does
// not leave the GPU).  need / need_device look one up and check its element count; `who` and `absent` word the engine's error texts.
struct TensorStore {
    const char* who;       // "<who>: tensor '<name>' <absent>"
    const char* absent;
    std::map<std::string, std::vector<float>> host;
    std::map<std::string, std::pair<const float*, int64_t>> device;

    void set(const char* name, const float* data, int64_t numel) { host[name].assign(data, data + numel); }
    void set_device(const char* name, const float* data, int64_t numel) { device[name] = std::make_pair(data, numel); }
    int need(const std::string& name, size_t numel, const float** out) const {
        auto it = host.find(name);
        if (it == host.end()) return missing("", name);
        if (it->second.size() != numel) return mis_sized("", name, it->second.size(), numel);
        *out = it->second.data();
        return AMTX_OK;
    }
    int need_device(const std::string& name, size_t numel, const float** out) const {
        auto it = device.find(name);
        if (it == device.end()) return missing("device ", name);
        if ((size_t)it->second.second != numel) return mis_sized("device ", name, (size_t)it->second.second, numel);
        *out = it->second.first;
        return AMTX_OK;
    }

private:
    int missing(const char* kind, const std::string& name) const {
        amtx_set_error("%s: %stensor '%s' %s", who, kind, name.c_str(), absent);
        return AMTX_ERR_ARG;
    }
    int mis_sized(const char* kind, const std::string& name, size_t has, size_t numel) const {
        amtx_set_error("%s: %stensor '%s' has %zu elements, expected %zu", who, kind, name.c_str(), has, numel);
        return AMTX_ERR_ARG;
    }
};

// A RE-sync overwrites the packed buffers in place (DevBuf::upload keeps its allocation; the device packers write on the caller's
// stream).  A forward pass of the previous weight version may still be in flight on ANOTHER stream (PyTorch side streams do not
// synchronise with the null stream), so every re-sync entry point first waits for everything the device has been given.
inline int amtx_quiesce_before_resync(bool packed_once) {
    if (packed_once) AMTX_CHECK_HIP(hipDeviceSynchronize());
    return AMTX_OK;
}

// Hands out 256-byte aligned pieces of a workspace one after the other; with a null base it only adds up the sizes.
struct WorkspaceCarver {
    char* base;
    size_t off = 0;
    char* take(size_t bytes) {
        char* p = base ? base + off : nullptr;
        off += align256(bytes);
        return p;
    }
};
