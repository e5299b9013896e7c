// libgsum_loo.so: the C ABI of include/gsum_loo.h (leave-one-out diagnostics).  Kernels: kernels/loo.hip.h.
#include <utility>
#include <vector>

#include "gsum_loo.h"
#include "host/sidelib.hip.h"
#include "kernels/loo.hip.h"

#define GL_API extern "C" __attribute__((visibility("default")))

namespace {

enum Phase { kUpload = 0, kInverse, kReduce, kH2D, kSolve, kD2H, kPhases };
constexpr int64_t kMaxN = (int64_t)1 << 20;        // keeps every byte count below far inside int64; no device holds such a matrix
constexpr int64_t kChunk = 512;                    // the columns of R one pair of solve launches takes

}  // namespace

struct gsum_loo : Handle {
    int64_t n = 0, N = 0;                          // the order of L, and n rounded up to loo::kBlock
    DevBuf<double> W;                              // N x N: the inverse of the padded factor
    DevBuf<double, true> R, Y;                     // N x ldr each: a chunk of right-hand sides and its forward product
    std::vector<double> p;                         // n
    double sum_log_diag = 0;
    double ms[kPhases] = {0, 0, 0, 0, 0, 0};
    std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> pending;    // (phase, start, stop) of the call in flight
    ~gsum_loo() {
        for (auto& e : pending) {
            (void)hipEventDestroy(e.second.first);
            (void)hipEventDestroy(e.second.second);
        }
    }
};

namespace {

// Run f (enqueues on h->stream) between two events charged to a phase; settle() turns them into milliseconds after the sync.
template <class F>
void timed(gsum_loo* h, Phase ph, F&& f) {
    hipEvent_t a = nullptr, b = nullptr;
    SL_CHECK(hipEventCreate(&a));
    if (hipEventCreate(&b) != hipSuccess) {
        (void)hipEventDestroy(a);
        throw Error("hipEventCreate failed");
    }
    h->pending.push_back({(int)ph, {a, b}});
    SL_CHECK(hipEventRecord(a, h->stream));
    f();
    SL_CHECK(hipEventRecord(b, h->stream));
}

void settle(gsum_loo* h) {
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
template <class F>
void run(gsum_loo* h, F&& f) {
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

// W = L^-1 for the padded factor Ld (both N x N); T is N x N scratch.  The diagonal check of level 0 is read back before the merges.
void invert(gsum_loo* h, const double* Ld, double* T, std::vector<double>& logdiag) {
    const int64_t N = h->N, nb = N / loo::kBlock;
    hipStream_t st = h->stream;
    DevBuf<int> info;
    DevBuf<double> logs;
    info.alloc((size_t)nb);
    logs.alloc((size_t)nb);
    std::vector<int> bad((size_t)nb);
    logdiag.resize((size_t)nb);
    SL_CHECK(hipFuncSetAttribute((const void*)loo::k_invert_diag, hipFuncAttributeMaxDynamicSharedMemorySize, (int)loo::kInvertLds));
    run(h, [&] {
        timed(h, kInverse, [&] {
            loo::k_invert_diag<<<(unsigned)nb, loo::kBlock, loo::kInvertLds, st>>>(Ld, h->W.p, N, h->n, info.p, logs.p);
            SL_LAUNCHED("k_invert_diag");
        });
        SL_CHECK(hipMemcpyAsync(bad.data(), info.p, sizeof(int) * nb, hipMemcpyDeviceToHost, st));
        SL_CHECK(hipMemcpyAsync(logdiag.data(), logs.p, sizeof(double) * nb, hipMemcpyDeviceToHost, st));
    });
    for (int64_t b = 0; b < nb; ++b)
        if (bad[(size_t)b])
            throw Error("gsum_loo_open: the factor's diagonal entry " + std::to_string(b * loo::kBlock + bad[(size_t)b] - 1) +
                        " is not a finite positive number");
    run(h, [&] {
        timed(h, kInverse, [&] {
            for (int64_t g = 2 * loo::kBlock; g / 2 < N; g *= 2) {
                const int64_t pairs = (N - g / 2 + g - 1) / g, tiles = (g / 2 / loo::kTile) * (g / 2 / loo::kTile);
                const dim3 grid((unsigned)tiles, (unsigned)pairs);
                loo::k_merge<0><<<grid, 256, 0, st>>>(Ld, h->W.p, T, N, g);
                loo::k_merge<1><<<grid, 256, 0, st>>>(Ld, h->W.p, T, N, g);
                loo::k_merge<2><<<grid, 256, 0, st>>>(Ld, h->W.p, T, N, g);
                loo::k_merge<3><<<grid, 256, 0, st>>>(Ld, h->W.p, T, N, g);
                SL_LAUNCHED("k_merge");
            }
        });
    });
}

}  // namespace

GL_API const char* gsum_loo_last_error(void) { return g_error.c_str(); }

GL_API int gsum_loo_open(const double* L, int64_t n, int device, gsum_loo** out) {
    return guarded([&] {
        if (!out) throw Error("gsum_loo_open: null pointer argument");
        *out = nullptr;
        if (!L) throw Error("gsum_loo_open: null pointer argument");
        if (n < 1) throw Error("gsum_loo_open: n must be >= 1, got " + std::to_string(n));
        if (n > kMaxN) throw Error("gsum_loo_open: n must be <= " + std::to_string(kMaxN) + ", got " + std::to_string(n));
        create(out, device, [&](gsum_loo* h) {
            const int64_t N = (n + loo::kBlock - 1) / loo::kBlock * loo::kBlock, nb = N / loo::kBlock;
            h->n = n;
            h->N = N;
            size_t free_b = 0, total_b = 0;
            SL_CHECK(hipMemGetInfo(&free_b, &total_b));
            const int64_t need = (3 * N * N + (nb + 1) * N) * (int64_t)sizeof(double) + ((int64_t)64 << 20);    // L, W, T, partials, p; slack
            if ((uint64_t)need > free_b)
                throw Error("gsum_loo_open: n = " + std::to_string(n) + " needs " + std::to_string(need >> 20) + " MiB of device memory, " +
                            std::to_string(free_b >> 20) + " MiB are free");
            DevBuf<double> Ld, T, partial, pd;
            Ld.alloc((size_t)(N * N));
            T.alloc((size_t)(N * N));
            h->W.alloc((size_t)(N * N));
            partial.alloc((size_t)(nb * N));
            pd.alloc((size_t)N);
            hipStream_t st = h->stream;
            run(h, [&] {
                timed(h, kUpload, [&] {
                    if (N > n) SL_CHECK(hipMemsetAsync(Ld.p, 0, sizeof(double) * N * N, st));              // L21 of the identity tail
                    SL_CHECK(hipMemcpy2DAsync(Ld.p, sizeof(double) * N, L, sizeof(double) * n, sizeof(double) * n, (size_t)n,
                                              hipMemcpyHostToDevice, st));
                    loo::k_clean_factor<<<(unsigned)nb, loo::kBlock, 0, st>>>(Ld.p, N, n);
                    SL_LAUNCHED("k_clean_factor");
                });
            });
            std::vector<double> logdiag;
            invert(h, Ld.p, T.p, logdiag);
            h->p.resize((size_t)n);
            run(h, [&] {
                timed(h, kReduce, [&] {
                    loo::k_colsq_partial<<<dim3((unsigned)nb, (unsigned)nb), loo::kBlock, 0, st>>>(h->W.p, N, partial.p);
                    SL_LAUNCHED("k_colsq_partial");
                    loo::k_colsq_total<<<(unsigned)nb, loo::kBlock, 0, st>>>(partial.p, N, pd.p);
                    SL_LAUNCHED("k_colsq_total");
                });
                SL_CHECK(hipMemcpyAsync(h->p.data(), pd.p, sizeof(double) * n, hipMemcpyDeviceToHost, st));
            });
            double s = 0;
            for (double v : logdiag) s += v;
            h->sum_log_diag = s;
        });
    });
}

GL_API int gsum_loo_precision_diag(gsum_loo* h, double* p, double* sum_log_diag) {
    return guarded([&] {
        if (!h || !p || !sum_log_diag) throw Error("gsum_loo_precision_diag: null pointer argument");
        std::copy(h->p.begin(), h->p.end(), p);
        *sum_log_diag = h->sum_log_diag;
    });
}

GL_API int gsum_loo_solve(gsum_loo* h, const double* R, int64_t k, double* alpha) {
    return guarded([&] {
        if (!h || !R || !alpha) throw Error("gsum_loo_solve: null pointer argument");
        if (k < 1) throw Error("gsum_loo_solve: k must be >= 1, got " + std::to_string(k));
        const int64_t n = h->n, N = h->N;
        hipStream_t st = h->stream;
        for (int64_t c0 = 0; c0 < k; c0 += kChunk) {
            const int64_t kc = std::min(kChunk, k - c0), ldr = (kc + loo::kTile - 1) / loo::kTile * loo::kTile;
            const size_t pitch = sizeof(double) * ldr;
            run(h, [&] {
                h->R.reserve((size_t)(N * ldr));
                h->Y.reserve((size_t)(N * ldr));
                timed(h, kH2D, [&] {
                    SL_CHECK(hipMemsetAsync(h->R.p, 0, sizeof(double) * N * ldr, st));                     // the padding rows and columns
                    SL_CHECK(hipMemcpy2DAsync(h->R.p, pitch, R + c0, sizeof(double) * k, sizeof(double) * kc, (size_t)n, hipMemcpyHostToDevice, st));
                });
                timed(h, kSolve, [&] {
                    const dim3 grid((unsigned)(N / loo::kTile), (unsigned)(ldr / loo::kTile));
                    loo::k_solve_forward<<<grid, 256, 0, st>>>(h->W.p, N, h->R.p, h->Y.p, ldr);
                    SL_LAUNCHED("k_solve_forward");
                    loo::k_solve_backward<<<grid, 256, 0, st>>>(h->W.p, N, h->Y.p, h->R.p, ldr);
                    SL_LAUNCHED("k_solve_backward");
                });
                timed(h, kD2H, [&] {
                    SL_CHECK(hipMemcpy2DAsync(alpha + c0, sizeof(double) * k, h->R.p, pitch, sizeof(double) * kc, (size_t)n, hipMemcpyDeviceToHost, st));
                });
            });
        }
    });
}

GL_API int gsum_loo_times(gsum_loo* h, double* ms, int32_t reset) {
    return guarded([&] {
        if (!h || !ms) throw Error("gsum_loo_times: null pointer argument");
        for (int k = 0; k < kPhases; ++k) {
            ms[k] = h->ms[k];
            if (reset) h->ms[k] = 0;
        }
    });
}

GL_API void gsum_loo_free(gsum_loo* h) { destroy(h); }
