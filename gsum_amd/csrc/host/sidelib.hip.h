// The host scaffold of the side libraries (gsum_vario.hip, gsum_refdist.hip; not part of libgsum_hip.so): the per-thread error
// string, checked HIP calls, device buffers, and the handle's device / stream with its create and free.  Everything has internal
// linkage, so each library carries its own copy and exports only what its version script names.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <string>

namespace {

thread_local std::string g_error;                  // what <library>_last_error() returns

struct Error : std::runtime_error {
    using std::runtime_error::runtime_error;
};

void check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw Error(std::string(what) + ": " + hipGetErrorString(e));
}
#define SL_CHECK(call) check((call), #call)
#define SL_LAUNCHED(name) check(hipGetLastError(), name)

// The body of every entry point that returns a code: 0, or 1 with the message in g_error.
template <class F>
int guarded(F&& f) {
    try {
        f();
        return 0;
    } catch (const std::exception& e) {
        g_error = e.what();
    } catch (...) {
        g_error = "unknown error";
    }
    return 1;
}

// Device memory of `n` elements.  reserve() only grows: to exactly the count asked for, or with Slack to at least half as much
// again as it holds (buffers that grow call after call).
template <class T, bool Slack = false>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    void alloc(size_t count) {
        release();
        if (count) SL_CHECK(hipMalloc(&p, count * sizeof(T)));
        n = count;
    }
    void reserve(size_t count) {
        if (count > n) alloc(Slack ? std::max(count, n + n / 2) : count);
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    ~DevBuf() { release(); }
};

// What every handle starts with.  The stream is destroyed after the derived handle's members (its buffers) are.
struct Handle {
    int device = 0;
    hipStream_t stream = nullptr;
    void open(int device) {
        this->device = device;
        SL_CHECK(hipSetDevice(device));
        SL_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    }
    ~Handle() {
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// *out = a new H opened on `device` and filled by init(h); when either throws the handle is deleted and *out stays nullptr.
template <class H, class F>
void create(H** out, int device, F&& init) {
    *out = nullptr;
    H* h = new H();
    try {
        h->open(device);
        init(h);
    } catch (...) {
        delete h;
        throw;
    }
    *out = h;
}

template <class H>
void destroy(H* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    delete h;
}

}  // namespace
