// libgsum_toep.so: the C ABI of include/gsum_toep.h (the Toeplitz likelihood path).  Kernels: kernels/toeplitz.hip.h.
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "gsum_toep.h"
#include "host/sidelib.hip.h"
#include "kernels/toeplitz.hip.h"

#define GT_API extern "C" __attribute__((visibility("default")))

static_assert(gt::kMaxN == GSUM_TOEP_MAX_N && gt::kMaxCols == GSUM_TOEP_MAX_COLS, "the header documents the limits");

namespace {

enum Phase { kH2D = 0, kSchur, kGram, kD2H, kPhases };

constexpr size_t kYBudget = (size_t)256 << 20;     // bytes of solved columns (Y) in flight: the first columns go through in chunks

}  // namespace

struct gsum_toep : Handle {
    DevBuf<double, true> t, Z, Y, G, sld;
    DevBuf<int32_t, true> info, ze;
    double ms[kPhases] = {0, 0, 0, 0};
    std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> pending;    // (phase, start, stop) of the call in flight
    ~gsum_toep() {
        for (auto& e : pending) {
            (void)hipEventDestroy(e.second.first);
            (void)hipEventDestroy(e.second.second);
        }
    }
};

namespace {

// Run f (enqueues on h->stream) between two events charged to a phase; settle() turns them into milliseconds after the sync.
template <class F>
void timed(gsum_toep* h, Phase ph, F&& f) {
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

void settle(gsum_toep* h) {
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
void run(gsum_toep* h, F&& f) {
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

// The generator elements per thread (E) and the columns of a chunk (C) follow from n alone: registers hold E * (4 + 1.5 C) doubles
// (a residual and its fp32 correction word per column), or E * (2 + 1.5 C) in the largest class, whose v lives in LDS.
int chunk_cols(int64_t n) { return n <= 512 ? 16 : n <= 2048 ? 12 : n <= 4096 ? 5 : 3; }

void launch_schur(gsum_toep* h, const double* t, int n, int ncols, int64_t m, double* Y, double* sld, int32_t* info) {
    const int C = chunk_cols(n);
    const dim3 grid((unsigned)((ncols + C - 1) / C), (unsigned)m);
    hipStream_t st = h->stream;
    if (n <= gt::kThreads)
        gt::k_schur<1, 16, false><<<grid, gt::kThreads, 0, st>>>(t, n, h->Z.p, h->ze.p, ncols, Y, sld, info);
    else if (n <= 4 * gt::kThreads)
        gt::k_schur<4, 12, false><<<grid, gt::kThreads, 0, st>>>(t, n, h->Z.p, h->ze.p, ncols, Y, sld, info);
    else if (n <= 8 * gt::kThreads)
        gt::k_schur<8, 5, false><<<grid, gt::kThreads, 0, st>>>(t, n, h->Z.p, h->ze.p, ncols, Y, sld, info);
    else
        gt::k_schur<16, 3, true><<<grid, gt::kThreads, 0, st>>>(t, n, h->Z.p, h->ze.p, ncols, Y, sld, info);
    SL_LAUNCHED("k_schur");
}

}  // namespace

GT_API const char* gsum_toep_last_error(void) { return g_error.c_str(); }

GT_API int gsum_toep_open(int32_t device, gsum_toep** out) {
    return guarded([&] {
        if (!out) throw Error("gsum_toep_open: null pointer argument");
        create(out, device, [](gsum_toep*) {});
    });
}

GT_API void gsum_toep_close(gsum_toep* h) { destroy(h); }

GT_API int64_t gsum_toep_max_n(const gsum_toep*) { return gt::kMaxN; }

GT_API int gsum_toep_gram(gsum_toep* h, const double* t, int64_t m, int64_t n, const double* Z, int64_t n_sets, int32_t cols, double* G_out,
                          double* sld_out, int32_t* info_out) {
    return guarded([&] {
        if (!h || !t || !Z || !G_out || !sld_out || !info_out) throw Error("gsum_toep_gram: null pointer argument");
        if (m < 1 || n < 1 || n_sets < 1)
            throw Error("gsum_toep_gram: m, n and n_sets must be >= 1, got " + std::to_string(m) + ", " + std::to_string(n) + ", " + std::to_string(n_sets));
        if (cols < 1 || cols > gt::kMaxCols)
            throw Error("gsum_toep_gram: cols must be between 1 and " + std::to_string(gt::kMaxCols) + ", got " + std::to_string(cols));
        if (n > gt::kMaxN)
            throw Error("gsum_toep_gram: n must be <= " + std::to_string(gt::kMaxN) + " (one workgroup holds the generator), got " + std::to_string(n));
        if (n_sets > 65535) throw Error("gsum_toep_gram: n_sets must be <= 65535, got " + std::to_string(n_sets));
        if (n_sets * cols > (((int64_t)1 << 31) - 1) / n)
            throw Error("gsum_toep_gram: n * n_sets * cols must be < 2^31, got " + std::to_string(n) + " x " + std::to_string(n_sets) + " x " + std::to_string(cols));
        // The right-hand sides are normalised on the device (k_colexp); the scale of T reaches the fp32 correction word through
        // lo(L) ~ 2^-53 sqrt(t0) and y ~ 1 / sqrt(t0), which stay far inside fp32's range for t0 within 2^-64 .. 2^64.
        for (int64_t i = 0; i < m; ++i) {
            const double t0 = t[i * n];
            if (t0 > 0.0 && t0 < INFINITY && (t0 < 0x1p-64 || t0 > 0x1p64)) {
                char got[32];
                snprintf(got, sizeof got, "%g", t0);
                throw Error("gsum_toep_gram: t[0] must lie within 2^-64 .. 2^64 (scale t by a power of 4 and G and sum_log_diag with it), got " +
                            std::string(got) + " in first column " + std::to_string(i));
            }
        }
        const int ncols = (int)(n_sets * cols);
        const size_t per_theta = (size_t)n * ncols;                            // doubles of Y per first column
        const int64_t step = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(m, 65535), (int64_t)(kYBudget / (per_theta * sizeof(double)))));
        const size_t gsz = (size_t)n_sets * cols * cols;
        run(h, [&] {
            h->t.reserve((size_t)m * n);
            h->Z.reserve(per_theta);
            h->Y.reserve(per_theta * step);
            h->G.reserve(gsz * m);
            h->sld.reserve((size_t)m);
            h->info.reserve((size_t)m);
            h->ze.reserve((size_t)ncols);
            hipStream_t st = h->stream;
            timed(h, kH2D, [&] {
                SL_CHECK(hipMemcpyAsync(h->t.p, t, sizeof(double) * m * n, hipMemcpyHostToDevice, st));
                SL_CHECK(hipMemcpyAsync(h->Z.p, Z, sizeof(double) * per_theta, hipMemcpyHostToDevice, st));
            });
            timed(h, kSchur, [&] {
                gt::k_colexp<<<(unsigned)ncols, gt::kWave, 0, st>>>(h->Z.p, (int)n, h->ze.p);
                SL_LAUNCHED("k_colexp");
            });
            for (int64_t lo = 0; lo < m; lo += step) {
                const int64_t cnt = std::min(step, m - lo);
                timed(h, kSchur, [&] { launch_schur(h, h->t.p + lo * n, (int)n, ncols, cnt, h->Y.p, h->sld.p + lo, h->info.p + lo); });
                timed(h, kGram, [&] {
                    gt::k_gram<<<dim3((unsigned)cols, (unsigned)n_sets, (unsigned)cnt), gt::kWave, 0, st>>>(h->Y.p, (int)n, cols, (int)n_sets,
                                                                                                         h->ze.p, h->info.p + lo, h->G.p + gsz * lo);
                    SL_LAUNCHED("k_gram");
                });
            }
            timed(h, kD2H, [&] {
                SL_CHECK(hipMemcpyAsync(G_out, h->G.p, sizeof(double) * gsz * m, hipMemcpyDeviceToHost, st));
                SL_CHECK(hipMemcpyAsync(sld_out, h->sld.p, sizeof(double) * m, hipMemcpyDeviceToHost, st));
                SL_CHECK(hipMemcpyAsync(info_out, h->info.p, sizeof(int32_t) * m, hipMemcpyDeviceToHost, st));
            });
        });
    });
}

GT_API int gsum_toep_times(gsum_toep* h, double* ms, int32_t reset) {
    return guarded([&] {
        if (!h || !ms) throw Error("gsum_toep_times: null pointer argument");
        for (int k = 0; k < kPhases; ++k) {
            ms[k] = h->ms[k];
            if (reset) h->ms[k] = 0;
        }
    });
}
