// Host-side scope of one call that owns device buffers and times launches for its own duration (dev_harness.hip: the single-kernel development
// entry points of include/duodiff_dev.h; capi.hip: dd_bench_gemm), and the one function through which every host unit reports an error on the
// context (dd_ctx itself: engine_state.h, which includes this header).  Not included by any kernel translation unit.
#pragma once
#include "../../include/duodiff.h"
#include "host_arena.h"

#include <hip/hip_runtime.h>
#include <string>
#include <vector>

struct dd_ctx;

namespace dd {

int ctx_fail(dd_ctx* c, int code, const std::string& msg);   // sets the context's error string, returns code (model.hip)

#pragma GCC visibility push(hidden)   // what follows stays out of the library's dynamic symbol table

inline int fail_hip(dd_ctx* c, hipError_t e, const char* what) {
    return ctx_fail(c, DD_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// The device buffers of one call, freed when it returns, and its error: the first failing operation is kept with its text and every later
// member does nothing (a buffer asked for after a failure is null).  status() is the one place where that becomes DD_ERR_HIP and the
// context's error string, "<operation>: <hipGetErrorString>".
class DevScope {
public:
    explicit DevScope(dd_ctx* c) : c_(c) {}
    ~DevScope() { for (void* p : bufs_) (void)hipFree(p); }
    DevScope(const DevScope&) = delete;
    DevScope& operator=(const DevScope&) = delete;

    bool ok() const { return err_ == hipSuccess; }
    bool ok(hipError_t e, const char* what) {
        if (ok() && e != hipSuccess) { err_ = e; what_ = what; }
        return ok();
    }
    int status() const { return ok() ? DD_OK : fail_hip(c_, err_, what_); }

    template <typename T = void> T* alloc(size_t bytes) {                        // uninitialised
        void* p = nullptr;
        if (ok() && ok(hipMalloc(&p, bytes), "hipMalloc")) bufs_.push_back(p);
        return static_cast<T*>(p);
    }
    template <typename T = void> T* filled(size_t bytes, int byte_value) {       // every byte = byte_value
        T* d = alloc<T>(bytes);
        if (ok()) ok(hipMemset(d, byte_value, bytes), "hipMemset");
        return d;
    }
    template <typename T> T* upload(const T* host, size_t bytes) {               // the host bytes
        T* d = alloc<T>(bytes);
        if (ok()) ok(hipMemcpy(d, host, bytes, hipMemcpyHostToDevice), "hipMemcpy to the device");
        return d;
    }
    void download(void* host, const void* dev, size_t bytes) {
        if (ok()) ok(hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost), "hipMemcpy from the device");
    }

private:
    dd_ctx* c_;
    std::vector<void*> bufs_;
    hipError_t err_ = hipSuccess;
    const char* what_ = "";
};
// a HIP call of the scope's function (a launch, a synchronise), skipped once anything has failed; a failure returns status()
#define DEV_HIP(dev, expr) \
    do { if (!(dev).ok() || !(dev).ok((expr), #expr)) return (dev).status(); } while (0)

// *ms_out = the mean time of `iters` calls of once() on s, between two events (nothing when iters <= 0 or ms_out is null); the first failing
// once() ends the loop
template <typename F>
hipError_t time_launches(hipStream_t s, int iters, F&& once, float* ms_out) {
    if (iters <= 0 || !ms_out) return hipSuccess;
    struct Events {
        hipEvent_t e[2] = {nullptr, nullptr};
        ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    } ev;
    hipError_t err = hipSuccess;
    for (hipEvent_t& x : ev.e) if ((err = hipEventCreate(&x)) != hipSuccess) return err;
    if ((err = hipEventRecord(ev.e[0], s)) != hipSuccess) return err;
    for (int i = 0; i < iters; ++i) if ((err = once()) != hipSuccess) return err;
    if ((err = hipEventRecord(ev.e[1], s)) != hipSuccess) return err;
    if ((err = hipEventSynchronize(ev.e[1])) != hipSuccess) return err;
    float ms = 0.f;
    if ((err = hipEventElapsedTime(&ms, ev.e[0], ev.e[1])) != hipSuccess) return err;
    *ms_out = ms / (float)iters;
    return hipSuccess;
}

// float rows [rows, cols] as bf16 rows [alloc_rows, cols]: the rows past `rows` hold fill_byte in every byte (0xFF: NaN, a row read past the
// end shows up as one)
inline std::vector<unsigned short> bf16_rows(const float* src, size_t rows, size_t cols, size_t alloc_rows, unsigned char fill_byte) {
    std::vector<unsigned short> v(alloc_rows * cols, (unsigned short)(fill_byte * 0x0101u));
    for (size_t i = 0; i < rows * cols; ++i) v[i] = host_f2bf(src[i]);
    return v;
}
#pragma GCC visibility pop

}  // namespace dd
