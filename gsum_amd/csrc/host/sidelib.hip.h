// The host scaffold of the side libraries (gsum_vario.hip, gsum_refdist.hip, gsum_pointwise.hip, gsum_loo.hip, gsum_toep.hip; not
// part of libgsum_hip.so): the per-thread error string, checked HIP calls, device buffers, the handle's device / stream with its
// create and free, and the phase clock of the handles that report per-phase times.  Everything has internal linkage, so each
// library carries its own copy and exports only what its version script names.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

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

// What every handle starts with.  The stream is destroyed after the derived handle's members (its buffers) are, and after the
// events a TimedHandle still holds: members first, then the clock's events, then the stream.
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

// A handle with a phase clock: ms[] are the device milliseconds of N phases, summed over the calls so far.
template <int N>
struct TimedHandle : Handle {
    double ms[N] = {};
    std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> pending;    // (phase, start, stop) of the call in flight
    ~TimedHandle() {
        for (auto& e : pending) {
            (void)hipEventDestroy(e.second.first);
            (void)hipEventDestroy(e.second.second);
        }
    }
};

// Run f (enqueues on h->stream) between two events charged to a phase; settle() turns them into milliseconds after the sync.
template <class H, class F>
void timed(H* h, int ph, F&& f) {
    hipEvent_t a = nullptr, b = nullptr;
    SL_CHECK(hipEventCreate(&a));
    if (hipEventCreate(&b) != hipSuccess) {
        (void)hipEventDestroy(a);
        throw Error("hipEventCreate failed");
    }
    h->pending.push_back({ph, {a, b}});
    SL_CHECK(hipEventRecord(a, h->stream));
    f();
    SL_CHECK(hipEventRecord(b, h->stream));
}

// Elapsed times are added only after a sync that succeeded; every event is destroyed either way, and only then is the sync's
// error reported.
template <class H>
void settle(H* h) {
    const hipError_t e = hipStreamSynchronize(h->stream);
    for (auto& p : h->pending) {
        float t = 0.f;
        if (e == hipSuccess && hipEventElapsedTime(&t, p.second.first, p.second.second) == hipSuccess) h->ms[p.first] += t;
        (void)hipEventDestroy(p.second.first);
        (void)hipEventDestroy(p.second.second);
    }
    h->pending.clear();
    check(e, "hipStreamSynchronize");
}

// A call that throws between timed() and settle() must still drain the stream before its buffers can be touched again.
template <class H, class F>
void run(H* h, F&& f) {
    SL_CHECK(hipSetDevice(h->device));
    try {
        f();
        settle(h);
    } catch (...) {
        try {
            settle(h);
        } catch (...) {
        }
        throw;
    }
}

// The body of every <library>_*_times: ms[0 .. count) = the clocks of the phases first .. first + count, zeroed after if reset.
template <int N>
void read_times(TimedHandle<N>* h, int first, int count, double* ms, int32_t reset) {
    for (int k = 0; k < count; ++k) {
        ms[k] = h->ms[first + k];
        if (reset) h->ms[first + k] = 0;
    }
}

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
