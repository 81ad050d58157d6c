// fm_ops_util.h -- what every per-op hook (fm_ops.cpp, fm_codec_ops.cpp) stands on: its own stream,
// device buffers freed with the hook, fp32 host arrays up and down in the precision's storage type.
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>

#include <vector>

#include "fm_kernels.h"
#include "fm_runtime.h"

// (fm_ops_util: the hook files pull it in with a using-directive)
namespace fm_ops_util {

// Every fill, copy and launch of a hook goes to the hook's own non-blocking stream, in order. (A
// non-blocking stream does not wait for the null stream, so a null-stream hipMemset of a buffer
// could land after a kernel on `s` has written it.)
struct DevBufs {
    hipStream_t s;
    std::vector<void*> ptrs;
    explicit DevBufs(hipStream_t st) : s(st) {}
    ~DevBufs() {
        (void)hipStreamSynchronize(s);
        for (void* p : ptrs) (void)hipFree(p);
    }
    void* alloc(size_t bytes) {
        void* p = nullptr;
        HIPCHK(hipMalloc(&p, bytes ? bytes : 16));
        HIPCHK(hipMemsetAsync(p, 0, bytes ? bytes : 16, s));
        ptrs.push_back(p);
        return p;
    }
    void put(void* d, const void* h, size_t bytes) {
        HIPCHK(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));  // the host array may be a temporary
    }
    // fp32 host -> device storage type T
    template <typename T> T* upload(const float* h, size_t n) {
        float* tmp = (float*)alloc(n * 4);
        put(tmp, h, n * 4);
        T* d = (T*)alloc(n * sizeof(T));
        launch_convert<T>(s, tmp, 0, (int64_t)n, d);
        HIPCHK(hipGetLastError());
        return d;
    }
};

template <typename T> void download(const T* d, size_t n, float* out, hipStream_t s) {
    std::vector<T> h(n);
    HIPCHK(hipMemcpyAsync(h.data(), d, n * sizeof(T), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (size_t i = 0; i < n; ++i) {
        if constexpr (sizeof(T) == 2) {
            const uint32_t u = (uint32_t)h[i] << 16;
            memcpy(&out[i], &u, 4);
        } else {
            out[i] = h[i];
        }
    }
}

struct StreamGuard {
    hipStream_t s = nullptr;
    explicit StreamGuard(int device) {
        int n = 0;
        FMCHECK(hipGetDeviceCount(&n) == hipSuccess && n > 0, "no HIP device visible");
        FMCHECK(device >= 0 && device < n, "bad device index");
        HIPCHK(hipSetDevice(device));
        HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    }
    ~StreamGuard() {
        if (s) (void)hipStreamDestroy(s);
    }
};

// A caller output array, in/out: uploaded before the launches (the caller's sentinel fill lands in
// the padding columns and rows the kernel must not touch) and downloaded after them.
template <typename T> struct InOut {
    T* d;
    float* h;
    size_t n;
    InOut(DevBufs& b, float* host, size_t count)
        : d(count ? b.upload<T>(host, count) : (T*)b.alloc(16)), h(host), n(count) {}  // (count 0: not in use)
    void get(hipStream_t s) {
        if (n) download<T>(d, n, h, s);
    }
    // the caller's values again (an in-place kernel's input before a repeated launch)
    void refill(DevBufs& b) {
        if (n) HIPCHK(hipMemcpyAsync(d, b.upload<T>(h, n), n * sizeof(T), hipMemcpyDeviceToDevice, b.s));
    }
};

}  // namespace fm_ops_util
