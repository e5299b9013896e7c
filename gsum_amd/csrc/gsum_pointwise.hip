// libgsum_pointwise.so: the C ABI of include/gsum_pointwise.h (TruncationPointwise).  Kernels: kernels/pointwise.hip.h.
#include <utility>
#include <vector>

#include "gsum_pointwise.h"
#include "host/sidelib.hip.h"
#include "kernels/pointwise.hip.h"

#define GP_API extern "C" __attribute__((visibility("default")))

static_assert(gp::kMaxOrders == GSUM_POINTWISE_MAX_ORDERS, "the header documents the limit on the kept orders");
static_assert(gp::kRefScalar == GSUM_POINTWISE_REF_SCALAR && gp::kRefPoints == GSUM_POINTWISE_REF_POINTS &&
                  gp::kRefRowScalar == GSUM_POINTWISE_REF_ROW_SCALAR && gp::kRefRowPoints == GSUM_POINTWISE_REF_ROW_POINTS,
              "the header documents the reference modes");

namespace {

enum Phase { kH2D = 0, kDiff, kLogLike, kCoverage, kD2H, kPhases };

}  // namespace

struct gsum_pointwise : TimedHandle<kPhases> {
    int64_t n = 0;
    int k = 0, kp = 0;
    double order_sum = 0;                          // the sum of the kept orders
    DevBuf<double> dy;                             // kp x n: the first differences of the kept columns, order-major
    DevBuf<int> orders;                            // kp: the kept orders
    DevBuf<double, true> ratios, refs, partial, out, loc, scale, data, t;
    DevBuf<unsigned long long> counts;
};

namespace {

void upload(gsum_pointwise* h, double* dst, const double* src, size_t count) {
    SL_CHECK(hipMemcpyAsync(dst, src, sizeof(double) * count, hipMemcpyHostToDevice, h->stream));
}

}  // namespace

GP_API const char* gsum_pointwise_last_error(void) { return g_error.c_str(); }

GP_API int gsum_pointwise_create(int32_t device, const double* y, const int32_t* orders, const int32_t* mask, int64_t n, int32_t k,
                                 gsum_pointwise** out) {
    return guarded([&] {
        if (!out) throw Error("gsum_pointwise_create: null pointer argument");
        *out = nullptr;
        if (!y || !orders || !mask) throw Error("gsum_pointwise_create: null pointer argument");
        if (n < 1 || k < 1) throw Error("gsum_pointwise_create: n and k must be >= 1, got " + std::to_string(n) + " x " + std::to_string(k));
        if (n > (((int64_t)1 << 31) - 1) / k) throw Error("gsum_pointwise_create: n * k must be < 2^31, got " + std::to_string(n) + " x " + std::to_string(k));
        std::vector<int> cols, kept;
        double order_sum = 0;
        for (int j = 0; j < k; ++j)
            if (mask[j]) {
                cols.push_back(j);
                kept.push_back(orders[j]);
                order_sum += orders[j];
            }
        const int kp = (int)cols.size();
        if (kp < 1 || kp > gp::kMaxOrders)
            throw Error("gsum_pointwise_create: between 1 and " + std::to_string(gp::kMaxOrders) + " orders must be kept, got " + std::to_string(kp));
        create(out, device, [&](gsum_pointwise* h) {
            h->n = n;
            h->k = k;
            h->kp = kp;
            h->order_sum = order_sum;
            DevBuf<double> yd;                                                    // the partial sums: needed for the differences only
            DevBuf<int> cd;
            yd.alloc((size_t)(n * k));
            cd.alloc(kp);
            h->dy.alloc((size_t)n * kp);
            h->orders.alloc(kp);
            run(h, [&] {
                timed(h, kH2D, [&] {
                    upload(h, yd.p, y, (size_t)(n * k));
                    SL_CHECK(hipMemcpyAsync(cd.p, cols.data(), sizeof(int) * kp, hipMemcpyHostToDevice, h->stream));
                    SL_CHECK(hipMemcpyAsync(h->orders.p, kept.data(), sizeof(int) * kp, hipMemcpyHostToDevice, h->stream));
                });
                timed(h, kDiff, [&] {
                    const int64_t blocks = (n * kp + gp::kThreads - 1) / gp::kThreads;
                    gp::k_differences<<<(unsigned)blocks, gp::kThreads, 0, h->stream>>>(yd.p, n, k, cd.p, kp, h->dy.p);
                    SL_LAUNCHED("k_differences");
                });
            });
        });
    });
}

GP_API int gsum_pointwise_loglike_grid(gsum_pointwise* h, const double* ratios, int32_t ratio_is_row, const double* refs, int32_t ref_mode,
                                       int64_t G, double df0, double scale0, double* out) {
    return guarded([&] {
        if (!h || !ratios || !refs || !out) throw Error("gsum_pointwise_loglike_grid: null pointer argument");
        if (G < 1) throw Error("gsum_pointwise_loglike_grid: G must be >= 1, got " + std::to_string(G));
        if (ref_mode < gp::kRefScalar || ref_mode > gp::kRefRowPoints)
            throw Error("gsum_pointwise_loglike_grid: ref_mode must be 0, 1, 2 or 3, got " + std::to_string(ref_mode));
        const int64_t n = h->n, nb = (n + gp::kSegment - 1) / gp::kSegment;
        const size_t nratio = (size_t)G * (ratio_is_row ? n : 1);
        const size_t nref = ref_mode == gp::kRefScalar ? 1 : ref_mode == gp::kRefPoints ? (size_t)n : ref_mode == gp::kRefRowScalar ? (size_t)G : (size_t)G * n;
        const int jac_points = ratio_is_row || ref_mode == gp::kRefPoints || ref_mode == gp::kRefRowPoints;
        const double prior = df0 * (scale0 * scale0), df = df0 + h->kp;
        run(h, [&] {
            h->ratios.reserve(nratio);
            h->refs.reserve(nref);
            h->partial.reserve((size_t)G * nb);
            h->out.reserve((size_t)G);
            hipStream_t st = h->stream;
            timed(h, kH2D, [&] {
                upload(h, h->ratios.p, ratios, nratio);
                upload(h, h->refs.p, refs, nref);
            });
            timed(h, kLogLike, [&] {
                const int64_t rows_per_launch = std::max<int64_t>(1, (((int64_t)1 << 31) - 1) / nb);     // blockIdx.x = row * nb + segment
                for (int64_t g0 = 0; g0 < G; g0 += rows_per_launch) {
                    const int64_t rows = std::min(rows_per_launch, G - g0);
                    gp::k_loglike<<<(unsigned)(rows * nb), gp::kThreads, 0, st>>>(h->dy.p, h->orders.p, h->kp, n, h->ratios.p, ratio_is_row ? 1 : 0,
                                                                                   h->refs.p, ref_mode, g0, nb, prior, df, h->order_sum, jac_points,
                                                                                   h->partial.p);
                    SL_LAUNCHED("k_loglike");
                    gp::k_loglike_rows<<<(unsigned)rows, gp::kWave, 0, st>>>(h->partial.p, nb, g0, h->ratios.p, h->refs.p, ref_mode, h->order_sum,
                                                                             jac_points, h->out.p);
                    SL_LAUNCHED("k_loglike_rows");
                }
            });
            timed(h, kD2H, [&] { SL_CHECK(hipMemcpyAsync(out, h->out.p, sizeof(double) * G, hipMemcpyDeviceToHost, st)); });
        });
    });
}

GP_API int gsum_pointwise_coverage(gsum_pointwise* h, const double* loc, const double* scale, const double* data, int32_t data_cols,
                                   const double* t_lo, const double* t_hi, int32_t D, int64_t* counts) {
    return guarded([&] {
        if (!h || !loc || !scale || !data || !t_lo || !t_hi || !counts) throw Error("gsum_pointwise_coverage: null pointer argument");
        if (D < 1) throw Error("gsum_pointwise_coverage: D must be >= 1, got " + std::to_string(D));
        const int64_t n = h->n;
        const int kp = h->kp;
        if (data_cols != 1 && data_cols != kp)
            throw Error("gsum_pointwise_coverage: data_cols must be 1 or " + std::to_string(kp) + ", got " + std::to_string(data_cols));
        static_assert(sizeof(unsigned long long) == sizeof(int64_t), "counts are copied out as int64");
        run(h, [&] {
            const size_t nk = (size_t)n * kp;
            h->loc.reserve(nk);
            h->scale.reserve(nk);
            h->data.reserve((size_t)n * data_cols);
            h->t.reserve((size_t)2 * D);
            h->counts.reserve((size_t)D * kp);
            hipStream_t st = h->stream;
            timed(h, kH2D, [&] {
                upload(h, h->loc.p, loc, nk);
                upload(h, h->scale.p, scale, nk);
                upload(h, h->data.p, data, (size_t)n * data_cols);
                upload(h, h->t.p, t_lo, D);
                upload(h, h->t.p + D, t_hi, D);
            });
            timed(h, kCoverage, [&] {
                SL_CHECK(hipMemsetAsync(h->counts.p, 0, sizeof(unsigned long long) * D * kp, st));
                const int64_t tiles = (n + gp::kThreads - 1) / gp::kThreads, db = (D + gp::kCovD - 1) / gp::kCovD;
                if (db > 65535) throw Error("gsum_pointwise_coverage: D must be <= " + std::to_string(65535 * gp::kCovD));
                const int64_t blocks = std::min<int64_t>(tiles, 2048);            // tiles are strided over them
                gp::k_coverage<<<dim3((unsigned)blocks, (unsigned)db), gp::kThreads, 0, st>>>(h->loc.p, h->scale.p, h->data.p, data_cols, n, kp, h->t.p,
                                                                                             h->t.p + D, D, h->counts.p);
                SL_LAUNCHED("k_coverage");
            });
            timed(h, kD2H, [&] { SL_CHECK(hipMemcpyAsync(counts, h->counts.p, sizeof(int64_t) * D * kp, hipMemcpyDeviceToHost, st)); });
        });
    });
}

GP_API int gsum_pointwise_times(gsum_pointwise* h, double* ms, int32_t reset) {
    return guarded([&] {
        if (!h || !ms) throw Error("gsum_pointwise_times: null pointer argument");
        read_times(h, 0, kPhases, ms, reset);
    });
}

GP_API void gsum_pointwise_free(gsum_pointwise* h) { destroy(h); }
