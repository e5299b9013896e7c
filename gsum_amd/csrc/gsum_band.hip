// libgsum_band.so: the C ABI of include/gsum_band.h (the banded likelihood path).  Kernels: kernels/band.hip.h.
#include <cstdio>
#include <string>
#include <vector>

#include "gsum_band.h"
#include "host/sidelib.hip.h"
#include "kernels/band.hip.h"

#define GB_API extern "C" __attribute__((visibility("default")))

static_assert(gb::kMaxB == GSUM_BAND_MAX_HALFWIDTH && gb::kBlock == GSUM_BAND_BLOCK, "the header documents the limits");
static_assert(GSUM_BAND_MAX_COLS == GSUM_MAX_RHS && GSUM_BAND_MAX_COLS == 16, "a set is one 16-column tile");

namespace {

enum Phase { kH2D = 0, kBuild, kFactor, kForward, kGram, kD2H, kPhases };

constexpr int64_t kLaunchLimit = (int64_t)1 << 31;         // elements a launch chunk must stay below
constexpr int64_t kYLimit = (int64_t)1 << 27;              // doubles of solved columns in flight (1 GiB) unless one (matrix, set) needs more
constexpr int64_t kGridYZ = 65535;

}  // namespace

struct gsum_band : TimedHandle<kPhases> {
    DevBuf<double, true> AB, L, Z, Y, G, sld, X;
    DevBuf<int32_t, true> info, flags;
    DevBuf<gsum_kernel_desc, true> descs;
    int64_t chunk = kLaunchLimit - 1;                      // gsum_band_set_chunk
    int64_t res_m = 0, res_n = 0, res_b = -1;              // what AB holds (gsum_band_build)
};

namespace {

std::string s(int64_t v) { return std::to_string(v); }

void check_mn(const char* fn, int64_t m, int64_t n) {
    if (m < 1 || n < 1) throw Error(std::string(fn) + ": m and n must be >= 1, got " + s(m) + ", " + s(n));
}

void check_b(const char* fn, int64_t n, int64_t b) {
    if (b < 0 || b > gb::kMaxB) throw Error(std::string(fn) + ": b must be between 0 and " + s(gb::kMaxB) + " (gsum_band_max_halfwidth), got " + s(b));
    if (n * (b + 1) >= kLaunchLimit) throw Error(std::string(fn) + ": n * (b + 1) must be below 2^31 per matrix, got " + s(n) + " * " + s(b + 1));
}

void check_descs(const char* fn, const gsum_kernel_desc* descs, int64_t m) {
    for (int64_t i = 0; i < m; ++i) {
        const gsum_kernel_desc& d = descs[i];
        bool many = d.n_ops == 0 && d.anisotropic != 0;
        if (d.n_ops < 0 || d.n_ops > GSUM_MAX_OPS || d.n_leaves < 0 || d.n_leaves > GSUM_MAX_LEAVES)
            throw Error(std::string(fn) + ": descs[" + s(i) + "] is not a kernel descriptor");
        for (int l = 0; l < d.n_leaves; ++l) many = many || d.leaf[l].anisotropic != 0;
        if (many)
            throw Error(std::string(fn) + ": descs[" + s(i) + "] has a length scale per feature: the banded path takes descriptors of one feature");
    }
}

// matrices per launch chunk: their bands, and with per_y > 0 their solved columns, stay below the limits
int64_t matrices_per_chunk(const gsum_band* h, int64_t m, int64_t per_band, int64_t per_y) {
    int64_t c = std::min<int64_t>(m, kGridYZ);
    c = std::min(c, std::max<int64_t>(1, h->chunk / per_band));
    if (per_y > 0) c = std::min(c, std::max<int64_t>(1, std::min(h->chunk, kYLimit) / per_y));
    return c;
}

void upload_points(gsum_band* h, const gsum_kernel_desc* descs, int64_t m, const double* X, int64_t n) {
    h->descs.reserve((size_t)m);
    h->X.reserve((size_t)n);
    timed(h, kH2D, [&] {
        SL_CHECK(hipMemcpyAsync(h->descs.p, descs, sizeof(gsum_kernel_desc) * m, hipMemcpyHostToDevice, h->stream));
        SL_CHECK(hipMemcpyAsync(h->X.p, X, sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
    });
}

// factor the cnt bands at Lp in place, info and sld at ip / sp
void launch_factor(gsum_band* h, double* Lp, int n, int b, int64_t cnt, int32_t* ip, double* sp) {
    hipLaunchKernelGGL(gb::k_band_factor, dim3((unsigned)cnt), dim3(gb::kThreads), 0, h->stream, Lp, n, b, ip);
    SL_LAUNCHED("k_band_factor");
    hipLaunchKernelGGL(gb::k_band_sld, dim3((unsigned)cnt), dim3(gb::kThreads), 0, h->stream, Lp, n, b, ip, sp);
    SL_LAUNCHED("k_band_sld");
}

void launch_forward(gsum_band* h, const double* Lp, int n, int b, const double* Zp, int ncols, int64_t cnt, double* Yp, const int32_t* ip) {
    const dim3 grid((unsigned)((ncols + 15) / 16), (unsigned)cnt);
    hipLaunchKernelGGL(gb::k_band_forward, grid, dim3(gb::kThreads), gb::forward_lds_bytes(b), h->stream, Lp, n, b, Zp, ncols, Yp, ip);
    SL_LAUNCHED("k_band_forward");
}

}  // namespace

GB_API const char* gsum_band_last_error(void) { return g_error.c_str(); }

GB_API int gsum_band_open(int32_t device, gsum_band** out) {
    return guarded([&] {
        if (!out) throw Error("gsum_band_open: null pointer argument");
        create(out, device, [](gsum_band*) {});
    });
}

GB_API void gsum_band_close(gsum_band* h) { destroy(h); }

GB_API int32_t gsum_band_max_halfwidth(const gsum_band*) { return gb::kMaxB; }

GB_API int32_t gsum_band_block(const gsum_band*) { return gb::kBlock; }

GB_API int gsum_band_set_chunk(gsum_band* h, int64_t max_elements) {
    return guarded([&] {
        if (!h) throw Error("gsum_band_set_chunk: null pointer argument");
        h->chunk = (max_elements < 1 || max_elements >= kLaunchLimit) ? kLaunchLimit - 1 : max_elements;
    });
}

GB_API int gsum_band_width(gsum_band* h, const gsum_kernel_desc* descs, int64_t m, const double* X, int64_t n, double nugget, int32_t* width_out) {
    (void)nugget;                                          // the nugget sits on the diagonal and moves no width
    return guarded([&] {
        if (!h || !descs || !X || !width_out) throw Error("gsum_band_width: null pointer argument");
        check_mn("gsum_band_width", m, n);
        check_b("gsum_band_width", n, gb::kMaxB);
        check_descs("gsum_band_width", descs, m);
        const int kmax = gb::kMaxB + 1;
        std::vector<int32_t> flags((size_t)m * kmax);
        run(h, [&] {
            upload_points(h, descs, m, X, n);
            h->flags.reserve(flags.size());
            timed(h, kBuild, [&] {
                SL_CHECK(hipMemsetAsync(h->flags.p, 0, sizeof(int32_t) * flags.size(), h->stream));
                for (int64_t lo = 0; lo < m; lo += kGridYZ) {
                    const int64_t cnt = std::min(kGridYZ, m - lo);
                    const dim3 grid((unsigned)((n + gb::kThreads - 1) / gb::kThreads), (unsigned)kmax, (unsigned)cnt);
                    hipLaunchKernelGGL(gb::k_band_width, grid, dim3(gb::kThreads), 0, h->stream, h->descs.p + lo, h->X.p, (int)n, kmax,
                                       h->flags.p + lo * kmax);
                    SL_LAUNCHED("k_band_width");
                }
            });
            timed(h, kD2H, [&] { SL_CHECK(hipMemcpyAsync(flags.data(), h->flags.p, sizeof(int32_t) * flags.size(), hipMemcpyDeviceToHost, h->stream)); });
        });
        for (int64_t i = 0; i < m; ++i) {
            int32_t w = 0;
            for (int k = 1; k <= kmax; ++k)
                if (flags[(size_t)i * kmax + k - 1]) w = k;
            width_out[i] = w;
        }
    });
}

GB_API int gsum_band_build(gsum_band* h, const gsum_kernel_desc* descs, int64_t m, const double* X, int64_t n, double nugget, int32_t b,
                           double* AB_out) {
    return guarded([&] {
        if (!h || !descs || !X) throw Error("gsum_band_build: null pointer argument");
        check_mn("gsum_band_build", m, n);
        check_b("gsum_band_build", n, b);
        check_descs("gsum_band_build", descs, m);
        const int64_t per = n * (b + 1);
        h->res_b = -1;
        run(h, [&] {
            upload_points(h, descs, m, X, n);
            h->AB.reserve((size_t)m * per);
            const int64_t step = matrices_per_chunk(h, m, per, 0);
            timed(h, kBuild, [&] {
                for (int64_t lo = 0; lo < m; lo += step) {
                    const int64_t cnt = std::min(step, m - lo);
                    const dim3 grid((unsigned)((n + gb::kThreads - 1) / gb::kThreads), (unsigned)(b + 1), (unsigned)cnt);
                    hipLaunchKernelGGL(gb::k_band_build, grid, dim3(gb::kThreads), 0, h->stream, h->descs.p + lo, h->X.p, (int)n, (int)b, nugget,
                                       h->AB.p + lo * per);
                    SL_LAUNCHED("k_band_build");
                }
            });
            if (AB_out)
                timed(h, kD2H, [&] { SL_CHECK(hipMemcpyAsync(AB_out, h->AB.p, sizeof(double) * m * per, hipMemcpyDeviceToHost, h->stream)); });
        });
        h->res_m = m;
        h->res_n = n;
        h->res_b = b;
    });
}

GB_API int gsum_band_gram(gsum_band* h, const double* AB, int64_t m, int64_t n, int32_t b, const double* Z, int64_t n_sets, int32_t cols,
                          double* G_out, double* sld_out, int32_t* info_out, double* L_out) {
    return guarded([&] {
        if (!h || !Z || !G_out || !sld_out || !info_out) throw Error("gsum_band_gram: null pointer argument");
        check_mn("gsum_band_gram", m, n);
        if (n_sets < 1) throw Error("gsum_band_gram: n_sets must be >= 1, got " + s(n_sets));
        check_b("gsum_band_gram", n, b);
        if (cols < 1 || cols > GSUM_BAND_MAX_COLS) throw Error("gsum_band_gram: cols must be between 1 and " + s(GSUM_BAND_MAX_COLS) + ", got " + s(cols));
        if (n * cols >= kLaunchLimit) throw Error("gsum_band_gram: n * cols must be below 2^31, got " + s(n) + " * " + s(cols));
        if (n_sets * cols >= kLaunchLimit) throw Error("gsum_band_gram: n_sets * cols must be below 2^31, got " + s(n_sets) + " * " + s(cols));
        if (!AB && !(h->res_b == b && h->res_m == m && h->res_n == n))
            throw Error("gsum_band_gram: AB is null and the handle holds no bands of this m, n and b (gsum_band_build)");
        const int64_t per = n * (b + 1);
        // sets per launch: the solved columns of one matrix stay below the limits
        const int64_t ylimit = std::min(h->chunk, std::max<int64_t>(kYLimit, n * cols));
        const int64_t sstep = std::min<int64_t>(std::min<int64_t>(n_sets, std::max<int64_t>(1, ylimit / (n * cols))), kLaunchLimit / 32);
        const int64_t step = matrices_per_chunk(h, m, per, n * cols * sstep);
        const size_t gsz = (size_t)n_sets * cols * cols;
        run(h, [&] {
            hipStream_t st = h->stream;
            h->L.reserve((size_t)step * per);
            h->Z.reserve((size_t)n * n_sets * cols);
            h->Y.reserve((size_t)step * n * cols * sstep);
            h->G.reserve(gsz * m);
            h->sld.reserve((size_t)m);
            h->info.reserve((size_t)m);
            timed(h, kH2D, [&] { SL_CHECK(hipMemcpyAsync(h->Z.p, Z, sizeof(double) * n * n_sets * cols, hipMemcpyHostToDevice, st)); });
            for (int64_t lo = 0; lo < m; lo += step) {
                const int64_t cnt = std::min(step, m - lo);
                if (AB) timed(h, kH2D, [&] { SL_CHECK(hipMemcpyAsync(h->L.p, AB + lo * per, sizeof(double) * cnt * per, hipMemcpyHostToDevice, st)); });
                else timed(h, kFactor, [&] { SL_CHECK(hipMemcpyAsync(h->L.p, h->AB.p + lo * per, sizeof(double) * cnt * per, hipMemcpyDeviceToDevice, st)); });
                timed(h, kFactor, [&] { launch_factor(h, h->L.p, (int)n, b, cnt, h->info.p + lo, h->sld.p + lo); });
                for (int64_t s0 = 0; s0 < n_sets; s0 += sstep) {
                    const int64_t sc = std::min(sstep, n_sets - s0);
                    timed(h, kForward, [&] {
                        launch_forward(h, h->L.p, (int)n, b, h->Z.p + s0 * cols * n, (int)(sc * cols), cnt, h->Y.p, h->info.p + lo);
                    });
                    timed(h, kGram, [&] {
                        hipLaunchKernelGGL(gb::k_band_gram, dim3((unsigned)sc, (unsigned)cnt), dim3(64), 0, st, h->Y.p, (int)n, (int)cols, (int)sc, n_sets,
                                           s0, h->info.p + lo, h->G.p + gsz * lo);
                        SL_LAUNCHED("k_band_gram");
                    });
                }
                if (L_out)
                    timed(h, kD2H, [&] { SL_CHECK(hipMemcpyAsync(L_out + lo * per, h->L.p, sizeof(double) * cnt * per, hipMemcpyDeviceToHost, st)); });
            }
            timed(h, kD2H, [&] {
                SL_CHECK(hipMemcpyAsync(G_out, h->G.p, sizeof(double) * gsz * m, hipMemcpyDeviceToHost, st));
                SL_CHECK(hipMemcpyAsync(sld_out, h->sld.p, sizeof(double) * m, hipMemcpyDeviceToHost, st));
                SL_CHECK(hipMemcpyAsync(info_out, h->info.p, sizeof(int32_t) * m, hipMemcpyDeviceToHost, st));
            });
        });
    });
}

GB_API int gsum_band_forward(gsum_band* h, const double* L, int64_t m, int64_t n, int32_t b, const double* Z, int64_t ncols, double* Y_out) {
    return guarded([&] {
        if (!h || !L || !Z || !Y_out) throw Error("gsum_band_forward: null pointer argument");
        check_mn("gsum_band_forward", m, n);
        if (ncols < 1) throw Error("gsum_band_forward: ncols must be >= 1, got " + s(ncols));
        check_b("gsum_band_forward", n, b);
        if (n * ncols >= kLaunchLimit) throw Error("gsum_band_forward: n * ncols must be below 2^31, got " + s(n) + " * " + s(ncols));
        const int64_t per = n * (b + 1);
        const int64_t step = matrices_per_chunk(h, m, per, n * ncols);
        run(h, [&] {
            hipStream_t st = h->stream;
            h->L.reserve((size_t)step * per);
            h->Z.reserve((size_t)n * ncols);
            h->Y.reserve((size_t)step * n * ncols);
            timed(h, kH2D, [&] { SL_CHECK(hipMemcpyAsync(h->Z.p, Z, sizeof(double) * n * ncols, hipMemcpyHostToDevice, st)); });
            for (int64_t lo = 0; lo < m; lo += step) {
                const int64_t cnt = std::min(step, m - lo);
                timed(h, kH2D, [&] { SL_CHECK(hipMemcpyAsync(h->L.p, L + lo * per, sizeof(double) * cnt * per, hipMemcpyHostToDevice, st)); });
                timed(h, kForward, [&] { launch_forward(h, h->L.p, (int)n, b, h->Z.p, (int)ncols, cnt, h->Y.p, nullptr); });
                timed(h, kD2H, [&] {
                    SL_CHECK(hipMemcpyAsync(Y_out + lo * n * ncols, h->Y.p, sizeof(double) * cnt * n * ncols, hipMemcpyDeviceToHost, st));
                });
            }
        });
    });
}

GB_API int gsum_band_times(gsum_band* h, double* ms, int32_t reset) {
    return guarded([&] {
        if (!h || !ms) throw Error("gsum_band_times: null pointer argument");
        read_times(h, 0, kPhases, ms, reset);
    });
}
