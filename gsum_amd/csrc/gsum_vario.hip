// libgsum_vario.so: the C ABI of include/gsum_vario.h (the empirical variogram).  Kernels: kernels/variogram.hip.h.
#include <cmath>
#include <cstring>
#include <vector>

#include "gsum_vario.h"
#include "host/sidelib.hip.h"
#include "kernels/variogram.hip.h"

#define GV_API extern "C" __attribute__((visibility("default")))

template <class T>
using GrowBuf = DevBuf<T, true>;                    // the cov stage's buffers: reserve() grows them by at least half

struct gsum_vario : Handle {
    int n = 0, d = 0, nc = 0, nbin = 0;
    int64_t P = 0;
    std::vector<int64_t> counts;
    std::vector<int32_t> start;                    // Nb + 1 list offsets
    DevBuf<int16_t> T;                              // n x n bins
    DevBuf<uint32_t> pairs;                         // (i << 16) | j, grouped by bin, tril order within a bin
    // cov-stage buffers
    GrowBuf<gv::Tile> tiles;
    GrowBuf<int32_t> order, tstart;
    GrowBuf<double> gam, den, sq, slab, out;
    std::vector<int32_t> last_b1, last_b2;         // the request list whose tiles, order and tstart are on the device
    int last_ntiles = 0;
};

GV_API const char* gsum_vario_last_error(void) { return g_error.c_str(); }

GV_API int gsum_vario_create(int32_t device, const double* X, int64_t n, int32_t d, const double* Z, int32_t n_curves,
                             const double* bounds, int32_t n_bounds, gsum_vario** out, int64_t* counts, double* h_sum, double* dij_sum) {
    return guarded([&] {
        if (!out || !X || !Z || !bounds || !counts || !h_sum || !dij_sum) throw Error("gsum_vario_create: null pointer argument");
        *out = nullptr;
        if (n < 1 || n > 65535) throw Error("gsum_vario_create: n must be in [1, 65535] (pairs are stored as 16-bit indices), got " + std::to_string(n));
        if (d < 1 || d > 64) throw Error("gsum_vario_create: d must be in [1, 64], got " + std::to_string(d));
        if (n_curves < 1) throw Error("gsum_vario_create: n_curves must be >= 1");
        if (n_bounds < 1 || n_bounds > 32766) throw Error("gsum_vario_create: the number of bins (bounds + 1) must be in [2, 32767], got " + std::to_string(n_bounds + 1));
        for (int64_t k = 0; k < n * d; ++k)
            if (!std::isfinite(X[k])) throw Error("gsum_vario_create: X must be finite");
        for (int k = 0; k < n_bounds; ++k) {
            if (!std::isfinite(bounds[k])) throw Error("gsum_vario_create: bin bounds must be finite");
            if (k && bounds[k] < bounds[k - 1]) throw Error("gsum_vario_create: bin bounds must be non-decreasing");
        }
        create(out, device, [&](gsum_vario* v) {
            v->n = (int)n;
            v->d = d;
            v->nc = n_curves;
            v->nbin = n_bounds + 1;
            v->P = n * (n - 1) / 2;
            hipStream_t st = v->stream;
            const int nbin = v->nbin;
            DevBuf<double> dX, dZ, dB, dh, ddij;
            DevBuf<int> dcnt, dstart;
            dX.alloc(n * d);
            dZ.alloc((size_t)n_curves * n);
            dB.alloc(n_bounds);
            v->T.alloc((size_t)n * n);
            dh.alloc(nbin);
            ddij.alloc((size_t)nbin * n_curves);
            dstart.alloc(nbin + 1);
            const int64_t P = v->P;
            // chunks of the tril order for the stable compaction: about 4096 pairs each, at most 2^24 per-chunk counters
            const int64_t max_chunks = std::max<int64_t>(1, ((int64_t)1 << 24) / nbin);
            const int64_t chunks = std::max<int64_t>(1, std::min<int64_t>((P + 4095) / 4096, max_chunks));
            const int64_t chunk = ((P + chunks - 1) / chunks + gv::kThreads - 1) / gv::kThreads * gv::kThreads;
            const int64_t nchunks = P ? (P + chunk - 1) / chunk : 0;
            dcnt.alloc((size_t)std::max<int64_t>(nchunks, 1) * nbin);
            v->pairs.alloc((size_t)std::max<int64_t>(P, 1));
            SL_CHECK(hipMemcpyAsync(dX.p, X, sizeof(double) * n * d, hipMemcpyHostToDevice, st));
            SL_CHECK(hipMemcpyAsync(dZ.p, Z, sizeof(double) * n_curves * n, hipMemcpyHostToDevice, st));
            SL_CHECK(hipMemcpyAsync(dB.p, bounds, sizeof(double) * n_bounds, hipMemcpyHostToDevice, st));
            gv::k_bin_table<<<dim3((unsigned)((n + 63) / 64), (unsigned)((n + 3) / 4)), gv::kThreads, 0, st>>>(dX.p, (int)n, d, dB.p, n_bounds, v->T.p);
            SL_LAUNCHED("k_bin_table");
            v->counts.assign(nbin, 0);
            v->start.assign(nbin + 1, 0);
            std::vector<int> cnt;                               // host staging of the compaction: outlives the stream's last copy
            if (P) {
                SL_CHECK(hipMemsetAsync(dcnt.p, 0, sizeof(int) * nchunks * nbin, st));
                gv::k_pair_count<<<(unsigned)nchunks, gv::kThreads, 0, st>>>(v->T.p, (int)n, P, chunk, nbin, dcnt.p);
                SL_LAUNCHED("k_pair_count");
                cnt.resize((size_t)nchunks * nbin);
                SL_CHECK(hipMemcpyAsync(cnt.data(), dcnt.p, sizeof(int) * cnt.size(), hipMemcpyDeviceToHost, st));
                SL_CHECK(hipStreamSynchronize(st));
                for (int64_t c = 0; c < nchunks; ++c)
                    for (int b = 0; b < nbin; ++b) v->counts[b] += cnt[(size_t)c * nbin + b];
                for (int b = 0; b < nbin; ++b) v->start[b + 1] = (int32_t)(v->start[b] + v->counts[b]);
                const std::vector<int> start0(v->start.begin(), v->start.end() - 1);
                std::vector<int> run(start0);
                for (int64_t c = 0; c < nchunks; ++c)                   // cursor of (chunk, bin) = bin start + earlier chunks' pairs
                    for (int b = 0; b < nbin; ++b) {
                        const int k = cnt[(size_t)c * nbin + b];
                        cnt[(size_t)c * nbin + b] = run[b];
                        run[b] += k;
                    }
                SL_CHECK(hipMemcpyAsync(dcnt.p, cnt.data(), sizeof(int) * cnt.size(), hipMemcpyHostToDevice, st));
                SL_CHECK(hipMemcpyAsync(dstart.p, v->start.data(), sizeof(int) * (nbin + 1), hipMemcpyHostToDevice, st));
                gv::k_pair_scatter<<<(unsigned)nchunks, gv::kThreads, 0, st>>>(v->T.p, (int)n, P, chunk, nbin, dcnt.p, v->pairs.p);
                SL_LAUNCHED("k_pair_scatter");
                gv::k_bin_sums<<<(unsigned)nbin, gv::kThreads, 0, st>>>(dX.p, (int)n, d, dZ.p, n_curves, v->pairs.p, dstart.p, dh.p, ddij.p);
                SL_LAUNCHED("k_bin_sums");
                SL_CHECK(hipMemcpyAsync(h_sum, dh.p, sizeof(double) * nbin, hipMemcpyDeviceToHost, st));
                SL_CHECK(hipMemcpyAsync(dij_sum, ddij.p, sizeof(double) * nbin * n_curves, hipMemcpyDeviceToHost, st));
            } else {
                std::fill(h_sum, h_sum + nbin, 0.0);
                std::fill(dij_sum, dij_sum + (size_t)nbin * n_curves, 0.0);
            }
            SL_CHECK(hipStreamSynchronize(st));
            std::copy(v->counts.begin(), v->counts.end(), counts);
            // the cov stage's buffers, sized for one request per bin (compute()) with up to 4 curves per group
            int64_t tiles = 0;
            for (int b = 0; b < nbin; ++b) {
                const int64_t t = (v->counts[b] + gv::kTile - 1) / gv::kTile;
                tiles += t * (t + 1) / 2;
            }
            const int ncp = (n_curves + 3) / 4 * 4;
            v->tiles.reserve(std::max<int64_t>(tiles, 1));
            v->order.reserve(std::max<int64_t>(tiles, 1));
            v->slab.reserve((size_t)std::max<int64_t>(tiles, 1) * ncp);
            v->tstart.reserve(nbin + 1);
            v->gam.reserve((size_t)nbin * ncp);
            v->den.reserve((size_t)nbin * ncp);
            v->sq.reserve((size_t)nbin * ncp);
            v->out.reserve((size_t)nbin * n_curves);
        });
    });
}

namespace {

template <int CG>
void launch_cov(gsum_vario* v, int ntiles, int groups, int ncp, double corr_factor) {
    const size_t lds = (size_t)v->nbin * CG <= (size_t)gv::kGammaLds ? sizeof(double) * v->nbin * CG : 0;   // gamma~ in LDS when it fits
    gv::k_cov<CG><<<dim3((unsigned)ntiles, (unsigned)groups), gv::kThreads, lds, v->stream>>>(
        v->tiles.p, v->order.p, v->pairs.p, v->T.p, v->n, v->gam.p, v->nbin, v->den.p, v->sq.p, ncp, corr_factor, v->slab.p);
    SL_LAUNCHED("k_cov");
}

}  // namespace

GV_API int gsum_vario_cov(gsum_vario* v, const double* gamma_tilde, double var_factor, double corr_factor, const int32_t* bin1,
                          const int32_t* bin2, int32_t n_pairs, double* sums) {
    return guarded([&] {
        if (!v || !gamma_tilde || (n_pairs > 0 && (!bin1 || !bin2 || !sums))) throw Error("gsum_vario_cov: null pointer argument");
        if (n_pairs < 0) throw Error("gsum_vario_cov: n_pairs must be >= 0");
        const int nbin = v->nbin, nc = v->nc;
        for (int r = 0; r < n_pairs; ++r)
            if (bin1[r] < 0 || bin1[r] >= nbin || bin2[r] < 0 || bin2[r] >= nbin)
                throw Error("gsum_vario_cov: bin index out of range [0, " + std::to_string(nbin) + ")");
        if (n_pairs == 0) return;
        SL_CHECK(hipSetDevice(v->device));
        const int CG = nc < 4 ? nc : 4;
        const int ncp = (nc + CG - 1) / CG * CG, groups = ncp / CG;
        auto gt = [&](int b, int c) { return gamma_tilde[(size_t)b * nc + (c < nc ? c : 0)]; };   // padded curves repeat curve 0
        // gamma~ as [group][bin][CG]; per request: den = 2 sqrt(gt1 gt2), sq = sqrt(var1 var2), var = var_factor sqrt(gt)
        std::vector<double> gam((size_t)groups * nbin * CG), den((size_t)n_pairs * ncp), sq((size_t)n_pairs * ncp);
        for (int gi = 0; gi < groups; ++gi)
            for (int b = 0; b < nbin; ++b)
                for (int c = 0; c < CG; ++c) gam[((size_t)gi * nbin + b) * CG + c] = gt(b, gi * CG + c);
        for (int r = 0; r < n_pairs; ++r)
            for (int c = 0; c < ncp; ++c) {
                const double g1 = gt(bin1[r], c), g2 = gt(bin2[r], c);
                den[(size_t)r * ncp + c] = 2 * std::sqrt(g1 * g2);
                const double v1 = var_factor * std::sqrt(g1), v2 = var_factor * std::sqrt(g2);
                sq[(size_t)r * ncp + c] = std::sqrt(v1 * v2);
            }
        // the tile list depends only on the requests and the bin counts: built and uploaded once per distinct request list
        const bool cached = (int)v->last_b1.size() == n_pairs && std::equal(bin1, bin1 + n_pairs, v->last_b1.begin()) &&
                            std::equal(bin2, bin2 + n_pairs, v->last_b2.begin());
        std::vector<gv::Tile> tiles;
        std::vector<int32_t> tstart(n_pairs + 1, 0), order;
        for (int r = 0; r < n_pairs && !cached; ++r) {
            int b1 = bin1[r], b2 = bin2[r];
            if (v->counts[b1] < v->counts[b2]) std::swap(b1, b2);     // the larger bin on the lanes: the sum is symmetric in p, q
            const int64_t m1 = v->counts[b1], m2 = v->counts[b2];
            if (m1 && m2) {
                const int t1 = (int)((m1 + gv::kTile - 1) / gv::kTile), t2 = (int)((m2 + gv::kTile - 1) / gv::kTile);
                for (int a = 0; a < t1; ++a)
                    for (int b = 0; b < (b1 == b2 ? a + 1 : t2); ++b) {
                        gv::Tile t;
                        t.req = r;
                        t.p0 = v->start[b1] + a * gv::kTile;
                        t.np = (int)std::min<int64_t>(gv::kTile, m1 - (int64_t)a * gv::kTile);
                        t.q0 = v->start[b2] + b * gv::kTile;
                        t.nq = (int)std::min<int64_t>(gv::kTile, m2 - (int64_t)b * gv::kTile);
                        t.kind = b1 != b2 ? 0 : a == b ? 2 : 1;
                        tiles.push_back(t);
                    }
            }
            tstart[r + 1] = (int32_t)tiles.size();
        }
        const int ntiles = cached ? v->last_ntiles : (int)tiles.size();
        if (!cached) {
            order.resize(ntiles);
            for (int k = 0; k < ntiles; ++k) order[k] = k;
            auto work = [&](const gv::Tile& t) { return t.kind == 2 ? (int64_t)t.np * (t.np + 1) / 2 : (int64_t)t.np * t.nq; };
            std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return work(tiles[a]) > work(tiles[b]); });
            v->last_b1.clear();
            v->last_b2.clear();
        }
        // grow (not inside the launch sequence: everything is allocated before the first copy)
        v->tiles.reserve(std::max(ntiles, 1));
        v->order.reserve(std::max(ntiles, 1));
        v->slab.reserve((size_t)std::max(ntiles, 1) * ncp);
        v->tstart.reserve(n_pairs + 1);
        v->gam.reserve(gam.size());
        v->den.reserve(den.size());
        v->sq.reserve(sq.size());
        v->out.reserve((size_t)n_pairs * nc);
        hipStream_t st = v->stream;
        if (!cached) {
            if (ntiles) {
                SL_CHECK(hipMemcpyAsync(v->tiles.p, tiles.data(), sizeof(gv::Tile) * ntiles, hipMemcpyHostToDevice, st));
                SL_CHECK(hipMemcpyAsync(v->order.p, order.data(), sizeof(int32_t) * ntiles, hipMemcpyHostToDevice, st));
            }
            SL_CHECK(hipMemcpyAsync(v->tstart.p, tstart.data(), sizeof(int32_t) * (n_pairs + 1), hipMemcpyHostToDevice, st));
        }
        SL_CHECK(hipMemcpyAsync(v->gam.p, gam.data(), sizeof(double) * gam.size(), hipMemcpyHostToDevice, st));
        SL_CHECK(hipMemcpyAsync(v->den.p, den.data(), sizeof(double) * den.size(), hipMemcpyHostToDevice, st));
        SL_CHECK(hipMemcpyAsync(v->sq.p, sq.data(), sizeof(double) * sq.size(), hipMemcpyHostToDevice, st));
        if (ntiles) {
            if (CG == 1) launch_cov<1>(v, ntiles, groups, ncp, corr_factor);
            else if (CG == 2) launch_cov<2>(v, ntiles, groups, ncp, corr_factor);
            else if (CG == 3) launch_cov<3>(v, ntiles, groups, ncp, corr_factor);
            else launch_cov<4>(v, ntiles, groups, ncp, corr_factor);
        }
        const int nout = n_pairs * nc;
        gv::k_cov_reduce<<<(unsigned)((nout + gv::kThreads - 1) / gv::kThreads), gv::kThreads, 0, st>>>(v->slab.p, v->tstart.p, n_pairs, nc, ncp, v->out.p);
        SL_LAUNCHED("k_cov_reduce");
        SL_CHECK(hipMemcpyAsync(sums, v->out.p, sizeof(double) * nout, hipMemcpyDeviceToHost, st));
        SL_CHECK(hipStreamSynchronize(st));
        if (!cached) {
            v->last_b1.assign(bin1, bin1 + n_pairs);
            v->last_b2.assign(bin2, bin2 + n_pairs);
            v->last_ntiles = ntiles;
        }
    });
}

GV_API int gsum_vario_corr(int32_t device, const double* rho, int64_t m, double corr_factor, double* out) {
    return guarded([&] {
        if (m < 0 || (m && (!rho || !out))) throw Error("gsum_vario_corr: bad arguments");
        if (!m) return;
        SL_CHECK(hipSetDevice(device));
        DevBuf<double> dr, dout;
        dr.alloc(m);
        dout.alloc(m);
        SL_CHECK(hipMemcpy(dr.p, rho, sizeof(double) * m, hipMemcpyHostToDevice));
        gv::k_corr<<<(unsigned)((m + gv::kThreads - 1) / gv::kThreads), gv::kThreads>>>(dr.p, m, corr_factor, dout.p);
        SL_LAUNCHED("k_corr");
        SL_CHECK(hipMemcpy(out, dout.p, sizeof(double) * m, hipMemcpyDeviceToHost));
        SL_CHECK(hipDeviceSynchronize());
    });
}

GV_API void gsum_vario_free(gsum_vario* v) { destroy(v); }
