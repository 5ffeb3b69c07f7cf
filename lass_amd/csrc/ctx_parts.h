// ctx_parts.h - the host plumbing the three contexts (lass_ctx in api.hip, lass_text_ctx in text.hip, lass_audioq_ctx in
// audio_clap.hip) are built from: opening the device, error reporting, the parameter store and the pinned staging of small
// per-call uploads.  Host-only.  The context structs hold these parts as members; what a part needs of its owner (HIP_TRY, fail,
// ParamStore::put) is an `err` string.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "../../include/lass_hip.h"

namespace {

#define HIP_TRY(ctx, expr)                                                      \
    do {                                                                        \
        hipError_t _e = (expr);                                                 \
        if (_e != hipSuccess) {                                                 \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(_e);     \
            return LASS_ERR_HIP;                                                \
        }                                                                       \
    } while (0)

template <class Ctx>
int fail(Ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}

inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

// What every *_create asks of device_id before it allocates anything: a HIP device, in range, and a gfx950.  LASS_OK, or the
// code with the message in `err` (the entry's thread-local create error: there is no context yet).
inline int open_device(int device_id, std::string& err) {
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        err = std::string("no HIP device available: ") + hipGetErrorString(e) + " (liblass_hip has no CPU fallback)";
        return LASS_ERR_HIP;
    }
    if (device_id < 0 || device_id >= ndev) {
        err = "device_id out of range";
        return LASS_ERR_ARG;
    }
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device_id);
    if (e != hipSuccess) {
        err = std::string("hipGetDeviceProperties: ") + hipGetErrorString(e);
        return LASS_ERR_HIP;
    }
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0) {
        err = std::string("device is ") + prop.gcnArchName + "; liblass_hip is built for gfx950 only";
        return LASS_ERR_HIP;
    }
    return LASS_OK;
}

struct Param {
    float* d = nullptr;
    std::vector<int64_t> shape;
    size_t n = 0;  // elements
};

// name -> float32 tensor on the device.  The owner validates names and shapes in front of put and selects its device.
struct ParamStore {
    std::map<std::string, Param> by_name;

    // a synchronous copy of `data` (host or device) under `name`; a tensor whose shape changed is reallocated
    template <class Ctx>
    int put(Ctx* c, const std::string& name, const void* data, const int64_t* shape, int ndim) {
        size_t n = 1;
        for (int i = 0; i < ndim; ++i) n *= (size_t)shape[i];
        Param& r = by_name[name];
        if (r.d && r.shape != std::vector<int64_t>(shape, shape + ndim)) {
            (void)hipFree(r.d);
            r.d = nullptr;
        }
        if (!r.d) HIP_TRY(c, hipMalloc(&r.d, n * sizeof(float)));
        r.shape.assign(shape, shape + ndim);
        r.n = n;
        HIP_TRY(c, hipMemcpy(r.d, data, n * sizeof(float), hipMemcpyDefault));
        return LASS_OK;
    }
    const Param* find(const std::string& name) const {
        auto it = by_name.find(name);
        return it == by_name.end() ? nullptr : &it->second;
    }
    const float* get(const std::string& name) const {
        const Param* p = find(name);
        return p ? p->d : nullptr;
    }
    void free_all() {
        for (auto& kv : by_name) (void)hipFree(kv.second.d);
        by_name.clear();
    }
};

// Pinned host ints behind one asynchronous upload per call: reserve (which waits until the previous call's upload has read
// them), fill, hipMemcpyAsync from `host` on the stream, record on the same stream.
struct PinnedInts {
    int* host = nullptr;
    size_t cap = 0;  // ints
    hipEvent_t ev = nullptr;
    bool pending = false;

    hipError_t create() { return hipEventCreateWithFlags(&ev, hipEventDisableTiming); }
    template <class Ctx>
    int reserve(Ctx* c, size_t n) {
        if (pending) HIP_TRY(c, hipEventSynchronize(ev));  // the previous call's upload has read the staging
        pending = false;
        if (n > cap) {
            if (host) (void)hipHostFree(host);
            host = nullptr;
            cap = 0;
            HIP_TRY(c, hipHostMalloc((void**)&host, n * sizeof(int), hipHostMallocDefault));
            cap = n;
        }
        return LASS_OK;
    }
    template <class Ctx>
    int record(Ctx* c, hipStream_t st) {
        HIP_TRY(c, hipEventRecord(ev, st));
        pending = true;
        return LASS_OK;
    }
    void destroy() {
        if (host) (void)hipHostFree(host);
        if (ev) (void)hipEventDestroy(ev);
    }
};

}  // namespace
