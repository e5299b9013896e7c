// libgsum_refdist.so: the C ABI of include/gsum_refdist.h (reference distributions).  Kernels: kernels/refdist.hip.h.
#include <cmath>
#include <utility>
#include <vector>

#include "gsum_refdist.h"
#include "host/sidelib.hip.h"
#include "kernels/refdist.hip.h"

#define GR_API extern "C" __attribute__((visibility("default")))

static_assert(gr::kSortLds == GSUM_REFDIST_LDS_SORT_MAX, "the header documents the LDS sort limit");

namespace {

enum Phase { kH2D = 0, kTranspose, kColSort, kPercentiles, kCoverage, kD2H, kPhases };

}  // namespace

struct gsum_refdist : TimedHandle<kPhases> {
    int64_t n = 0, m = 0;
    DevBuf<double> D, T;                           // the matrix (n x m) and the scratch matrix of the same size
    DevBuf<uint64_t> k0, k1;                       // long segments: the keys of every padded segment, ping and pong
    DevBuf<double> lower, upper, gamma, out;
    DevBuf<int64_t> idx;
    DevBuf<unsigned long long> counts;
    bool lds_attr = false;
};

namespace {

void transpose(gsum_refdist* h, const double* in, int64_t rows, int64_t cols, double* out) {
    const int64_t tiles = ((rows + gr::kTile - 1) / gr::kTile) * ((cols + gr::kTile - 1) / gr::kTile);
    gr::k_transpose<<<(unsigned)tiles, gr::kThreads, 0, h->stream>>>(in, rows, cols, out);
    SL_LAUNCHED("k_transpose");
}

int pow2_at_least(int64_t v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

// Device memory a sort of nseg segments of len needs beyond src / dst: none up to kSortLds, two key buffers above.
void reserve_sort(gsum_refdist* h, int64_t nseg, int64_t len) {
    if (len <= gr::kSortLds) return;
    const int64_t chunks = (len + gr::kSortLds - 1) / gr::kSortLds;
    const int64_t total = nseg * chunks * gr::kSortLds;
    h->k0.reserve((size_t)total);
    h->k1.reserve((size_t)total);
}

// dst segment s (dst + s * len) = src segment s sorted ascending, s < nseg; dst may be src.  reserve_sort() first.
void sort_segments(gsum_refdist* h, const double* src, double* dst, int64_t nseg, int64_t len) {
    if (!h->lds_attr) {
        SL_CHECK(hipFuncSetAttribute((const void*)gr::k_sort_lds<false>, hipFuncAttributeMaxDynamicSharedMemorySize, gr::kSortLds * 8));
        SL_CHECK(hipFuncSetAttribute((const void*)gr::k_sort_lds<true>, hipFuncAttributeMaxDynamicSharedMemorySize, gr::kSortLds * 8));
        h->lds_attr = true;
    }
    hipStream_t st = h->stream;
    if (len <= gr::kSortLds) {                                               // THE switch: one workgroup's LDS holds the segment
        const int P = pow2_at_least(len);
        const int threads = std::min(gr::kSortThreads, std::max(64, P / 2));
        gr::k_sort_lds<false><<<(unsigned)nseg, threads, (size_t)P * 8, st>>>(src, len, len, 1, P, dst, nullptr);
        SL_LAUNCHED("k_sort_lds");
        return;
    }
    const int P = gr::kSortLds;
    const int64_t chunks = (len + P - 1) / P, Lp = chunks * P, total = nseg * Lp;
    if (nseg * chunks >= ((int64_t)1 << 31)) throw Error("gsum_refdist: too many sort chunks");
    gr::k_sort_lds<true><<<(unsigned)(nseg * chunks), gr::kSortThreads, (size_t)P * 8, st>>>(src, len, len, (int)chunks, P, nullptr, h->k0.p);
    SL_LAUNCHED("k_sort_lds");
    uint64_t *in = h->k0.p, *out = h->k1.p;
    const int64_t blocks = (total + gr::kThreads - 1) / gr::kThreads;
    for (int64_t w = P; w < Lp; w *= 2) {
        gr::k_merge_pass<<<(unsigned)blocks, gr::kThreads, 0, st>>>(in, out, Lp, w, total);
        SL_LAUNCHED("k_merge_pass");
        std::swap(in, out);
    }
    const int64_t vals = nseg * len;
    gr::k_keys_to_double<<<(unsigned)((vals + gr::kThreads - 1) / gr::kThreads), gr::kThreads, 0, st>>>(in, Lp, len, len, vals, dst);
    SL_LAUNCHED("k_keys_to_double");
}

void enqueue_sort_columns(gsum_refdist* h, double* sorted) {
    const int64_t n = h->n, m = h->m;
    reserve_sort(h, m, n);
    timed(h, kTranspose, [&] { transpose(h, h->D.p, n, m, h->T.p); });
    timed(h, kColSort, [&] { sort_segments(h, h->T.p, h->T.p, m, n); });
    timed(h, kTranspose, [&] { transpose(h, h->T.p, m, n, h->D.p); });
    if (sorted) timed(h, kD2H, [&] { SL_CHECK(hipMemcpyAsync(sorted, h->D.p, sizeof(double) * n * m, hipMemcpyDeviceToHost, h->stream)); });
}

// Everything the percentile stage allocates; called before the first launch of the call.
void reserve_percentiles(gsum_refdist* h, int nq) {
    reserve_sort(h, h->n, h->m);
    h->idx.reserve(nq);
    h->gamma.reserve(nq);
    h->out.reserve((size_t)nq * h->n);
}

// idx / gamma staging lives in the caller until settle(); reserve_percentiles() first
void enqueue_row_percentiles(gsum_refdist* h, const std::vector<int64_t>& idx, const std::vector<double>& gamma, double* out) {
    const int64_t n = h->n, m = h->m;
    const int nq = (int)idx.size();
    hipStream_t st = h->stream;
    timed(h, kH2D, [&] {
        SL_CHECK(hipMemcpyAsync(h->idx.p, idx.data(), sizeof(int64_t) * nq, hipMemcpyHostToDevice, st));
        SL_CHECK(hipMemcpyAsync(h->gamma.p, gamma.data(), sizeof(double) * nq, hipMemcpyHostToDevice, st));
    });
    timed(h, kPercentiles, [&] {
        sort_segments(h, h->D.p, h->T.p, n, m);
        gr::k_pick<<<(unsigned)((n + gr::kThreads - 1) / gr::kThreads), gr::kThreads, 0, st>>>(h->T.p, n, m, h->idx.p, h->gamma.p, nq, h->out.p);
        SL_LAUNCHED("k_pick");
    });
    timed(h, kD2H, [&] { SL_CHECK(hipMemcpyAsync(out, h->out.p, sizeof(double) * nq * n, hipMemcpyDeviceToHost, st)); });
}

// numpy's virtual index of the 'linear' method, (m - 1) * (q / 100), its floor and the remainder
void percentile_ranks(const char* who, const double* q, int32_t nq, int64_t m, std::vector<int64_t>& idx, std::vector<double>& gamma) {
    if (nq < 1) throw Error(std::string(who) + ": nq must be >= 1");
    idx.resize(nq);
    gamma.resize(nq);
    for (int k = 0; k < nq; ++k) {
        if (!(q[k] >= 0.0 && q[k] <= 100.0)) throw Error(std::string(who) + ": percentiles must be in [0, 100]");
        const double quant = q[k] / 100.0;
        const double v = (double)(m - 1) * quant;
        const double fl = std::floor(v);
        idx[k] = std::min<int64_t>((int64_t)fl, m - 1);
        gamma[k] = v - fl;
    }
}

}  // namespace

GR_API const char* gsum_refdist_last_error(void) { return g_error.c_str(); }

GR_API int gsum_refdist_create(int32_t device, const double* A, int64_t n, int64_t m, gsum_refdist** out) {
    return guarded([&] {
        if (!out) throw Error("gsum_refdist_create: null pointer argument");
        *out = nullptr;
        if (!A) throw Error("gsum_refdist_create: null pointer argument");
        if (n < 1 || m < 1) throw Error("gsum_refdist_create: n and m must be >= 1, got " + std::to_string(n) + " x " + std::to_string(m));
        if (n > (((int64_t)1 << 31) - 1) / m) throw Error("gsum_refdist_create: n * m must be < 2^31, got " + std::to_string(n) + " x " + std::to_string(m));
        create(out, device, [&](gsum_refdist* h) {
            h->n = n;
            h->m = m;
            h->D.reserve((size_t)(n * m));
            h->T.reserve((size_t)(n * m));
            run(h, [&] { timed(h, kH2D, [&] { SL_CHECK(hipMemcpyAsync(h->D.p, A, sizeof(double) * n * m, hipMemcpyHostToDevice, h->stream)); }); });
        });
    });
}

GR_API int gsum_refdist_sort_columns(gsum_refdist* h, double* sorted) {
    return guarded([&] {
        if (!h) throw Error("gsum_refdist_sort_columns: null pointer argument");
        run(h, [&] { enqueue_sort_columns(h, sorted); });
    });
}

GR_API int gsum_refdist_row_percentiles(gsum_refdist* h, const double* q, int32_t nq, double* out) {
    return guarded([&] {
        if (!h || !q || !out) throw Error("gsum_refdist_row_percentiles: null pointer argument");
        std::vector<int64_t> idx;
        std::vector<double> gamma;
        percentile_ranks("gsum_refdist_row_percentiles", q, nq, h->m, idx, gamma);
        run(h, [&] {
            reserve_percentiles(h, nq);
            enqueue_row_percentiles(h, idx, gamma, out);
        });
    });
}

GR_API int gsum_refdist_qq_bands(gsum_refdist* h, const double* q, int32_t nq, double* bands, double* sorted) {
    return guarded([&] {
        if (!h || !q || !bands) throw Error("gsum_refdist_qq_bands: null pointer argument");
        std::vector<int64_t> idx;
        std::vector<double> gamma;
        percentile_ranks("gsum_refdist_qq_bands", q, nq, h->m, idx, gamma);
        run(h, [&] {
            reserve_sort(h, h->m, h->n);                                       // every buffer of both stages before the first launch
            reserve_percentiles(h, nq);
            enqueue_sort_columns(h, sorted);
            enqueue_row_percentiles(h, idx, gamma, bands);
        });
    });
}

GR_API int gsum_refdist_coverage(gsum_refdist* h, const double* lower, const double* upper, int32_t K, int64_t* counts) {
    return guarded([&] {
        if (!h || !lower || !upper || !counts) throw Error("gsum_refdist_coverage: null pointer argument");
        if (K < 1 || K > 65535 * gr::kCovK) throw Error("gsum_refdist_coverage: K must be in [1, 524280], got " + std::to_string(K));
        const int64_t n = h->n, m = h->m;
        static_assert(sizeof(unsigned long long) == sizeof(int64_t), "counts are copied out as int64");
        run(h, [&] {
            h->lower.reserve((size_t)K * n);
            h->upper.reserve((size_t)K * n);
            h->counts.reserve((size_t)m * K);
            hipStream_t st = h->stream;
            timed(h, kH2D, [&] {
                SL_CHECK(hipMemcpyAsync(h->lower.p, lower, sizeof(double) * K * n, hipMemcpyHostToDevice, st));
                SL_CHECK(hipMemcpyAsync(h->upper.p, upper, sizeof(double) * K * n, hipMemcpyHostToDevice, st));
            });
            timed(h, kCoverage, [&] {
                SL_CHECK(hipMemsetAsync(h->counts.p, 0, sizeof(unsigned long long) * m * K, st));
                // slices of the points so that about 1024 workgroups exist; a slice is a whole number of LDS stages
                const int64_t jb = (m + gr::kThreads - 1) / gr::kThreads, kb = (K + gr::kCovK - 1) / gr::kCovK;
                const int64_t stages = (n + gr::kCovI - 1) / gr::kCovI;
                const int64_t want = std::max<int64_t>(1, std::min<int64_t>({stages, (1024 + jb * kb - 1) / (jb * kb), 65535}));
                const int64_t slice = (stages + want - 1) / want * gr::kCovI;
                const int64_t slices = (n + slice - 1) / slice;
                if (jb >= ((int64_t)1 << 31)) throw Error("gsum_refdist_coverage: too many curves");
                gr::k_coverage<<<dim3((unsigned)jb, (unsigned)kb, (unsigned)slices), gr::kThreads, 0, st>>>(h->D.p, n, m, h->lower.p, h->upper.p, K,
                                                                                                             slice, h->counts.p);
                SL_LAUNCHED("k_coverage");
            });
            timed(h, kD2H, [&] { SL_CHECK(hipMemcpyAsync(counts, h->counts.p, sizeof(int64_t) * m * K, hipMemcpyDeviceToHost, st)); });
        });
    });
}

GR_API int gsum_refdist_times(gsum_refdist* h, double* ms, int32_t reset) {
    return guarded([&] {
        if (!h || !ms) throw Error("gsum_refdist_times: null pointer argument");
        read_times(h, 0, kPhases, ms, reset);
    });
}

GR_API void gsum_refdist_free(gsum_refdist* h) { destroy(h); }
