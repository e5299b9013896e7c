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
// the phases of gsum_toep_grad and gsum_toep_solve (gsum_toep_grad_times), after those of gsum_toep_gram in one array
enum GradPhase { kGH2D = kPhases, kGSchur, kGLevinson, kGGram, kGDiag, kGSolve, kGContract, kGD2H, kAllPhases };
// the phases of gsum_toep_predict and gsum_toep_loo (gsum_toep_post_times), after those
enum PostPhase { kPH2D = kAllPhases, kPSchur, kPLevinson, kPSums, kPCov, kPSolve, kPD2H, kEveryPhase };
// the phases of gsum_toep_gram_panel and gsum_toep_predict_panel (gsum_toep_panel_times), after those
enum PanelPhase { kNH2D = kEveryPhase, kNRecursion, kNDiag, kNUpdate, kNSums, kNCov, kND2H, kTotalPhases };
// the phases of gsum_toep_gram_blocked and gsum_toep_predict_blocked (gsum_toep_blocked_times), after those
enum BlockedPhase { kBH2D = kTotalPhases, kBLead, kBTiles, kBDiag, kBUpdate, kBSums, kBCov, kBD2H, kGrandPhases };
// the phases of gsum_toep_grad_blocked, gsum_toep_solve_blocked and gsum_toep_loo_blocked (gsum_toep_levinson_times), after those
enum LevinsonPhase { kLH2D = kGrandPhases, kLLead, kLTiles, kLDiag, kLUpdate, kLLevinson, kLGram, kLDiagsums, kLSolve, kLContract, kLD2H, kUltimatePhases };

static_assert((GSUM_TOEP_BLOCKED_MAX_N - gt::kPanelB + 15) / 16 <= 65535 && (GSUM_TOEP_BLOCKED_MAX_N + 31) / 32 <= 65535,
              "k_panel_update's and k_panel_load's grid y at the blocked route's limit");
constexpr int kBlockedSettle = 256;                // panels of the blocked route between two settlements of the phase clock's events

constexpr size_t kYBudget = (size_t)256 << 20;     // bytes of solved columns (Y) in flight: the first columns go through in chunks
// the panel route's: the solved columns with their correction words, the panel and the generator state of the first columns in flight
constexpr size_t kPanelBudget = (size_t)1 << 30;

}  // namespace

struct gsum_toep : TimedHandle<kUltimatePhases> {
    DevBuf<double, true> t, Z, Y, G, sld;
    DevBuf<int32_t, true> info, ze;
    DevBuf<double, true> dt, steps, xd, xf, sd, trace, W, As, Aout, Q, H;      // the gradient path's
    DevBuf<double, true> Yz, quad, cross, cov, pd;                             // the posterior's
    DevBuf<double, true> Ph, Pst;                                              // the panel route's: a panel's high words, the generator state
    DevBuf<float, true> Pl, Zc;                                                // ... its low words, the correction words beside Y
    DevBuf<double, true> Bst, Bco, Bdg;                                        // the blocked route's: two generator states, a panel's coefficients, diag(L)
    DevBuf<double, true> Lst;                                                  // the tiled replay's: the two states of A and B
};

namespace {

// THE size classes, written here and nowhere else.  The generator elements per thread (E) and the columns of a chunk (C) follow from
// n alone: registers hold E * (4 + 1.5 C) doubles (a residual and its fp32 correction word per column), or E * (2 + 1.5 C) in the
// largest class, whose v lives in LDS (VL).
template <int E_, int C_, bool VL_>
struct SizeClass {
    static constexpr int E = E_, C = C_;
    static constexpr bool VL = VL_;
};

// f(SizeClass of n): what a launch instantiates its kernel from.
template <class F>
void with_size_class(int n, F&& f) {
    if (n <= gt::kThreads)
        f(SizeClass<1, 16, false>{});
    else if (n <= 4 * gt::kThreads)
        f(SizeClass<4, 12, false>{});
    else if (n <= 8 * gt::kThreads)
        f(SizeClass<8, 5, false>{});
    else
        f(SizeClass<16, 3, true>{});
}

// E of n: the generator elements a k_schur thread holds and sums log L_jj over; beyond the size classes ceil(n / kThreads).
int generator_elements(int64_t n) {
    int E = (int)((n + gt::kThreads - 1) / gt::kThreads);
    if (n <= gt::kMaxN) with_size_class((int)n, [&](auto k) { E = decltype(k)::E; });
    return E;
}

// The Schur recursion of m first columns with the forward substitution of the ncols columns Z / ze beside it.  R: it also hands out
// its reflection coefficients and rotations (steps, (m, n, 4)), which launch_levinson replays.
template <bool R>
void launch_schur(gsum_toep* h, const double* t, int n, const double* Z, const int32_t* ze, int ncols, int64_t m, double* Y, double* sld,
                  int32_t* info, double* steps) {
    with_size_class(n, [&](auto k) {
        using K = decltype(k);
        const dim3 grid((unsigned)((ncols + K::C - 1) / K::C), (unsigned)m);       // the chunks of the C the kernel is made for
        gt::k_schur<K::E, K::C, K::VL, R><<<grid, gt::kThreads, 0, h->stream>>>(t, n, Z, ze, ncols, Y, sld, info, steps);
    });
    SL_LAUNCHED("k_schur");
}

// The recursion that replays the steps into x = T^-1 e_0 (xd both words, xf rounded).
void launch_levinson(gsum_toep* h, const double* t, int n, int64_t m, double* steps, double* xd, double* xf, double* sld, int32_t* info) {
    hipStream_t st = h->stream;
    gt::k_coeffs<<<dim3((unsigned)((n + 255) / 256), (unsigned)m), 256, 0, st>>>(steps, n, info);
    SL_LAUNCHED("k_coeffs");
    with_size_class(n, [&](auto k) { gt::k_levinson<decltype(k)::E><<<(unsigned)m, gt::kThreads, 0, st>>>(t, n, steps, xd, xf, sld, info); });
    SL_LAUNCHED("k_levinson");
}

// The exponents ze of the ncols columns of h->Z, which the kernels normalise by.
void launch_colexp(gsum_toep* h, int n, int ncols) {
    gt::k_colexp<<<(unsigned)ncols, gt::kWave, 0, h->stream>>>(h->Z.p, n, h->ze.p);
    SL_LAUNCHED("k_colexp");
}

// G of cnt first columns from their solved columns h->Y.
void launch_gram(gsum_toep* h, int n, int cols, int n_sets, int64_t cnt, const int32_t* info, double* G) {
    gt::k_gram<<<dim3((unsigned)cols, (unsigned)n_sets, (unsigned)cnt), gt::kWave, 0, h->stream>>>(h->Y.p, n, cols, n_sets, h->ze.p, info, G);
    SL_LAUNCHED("k_gram");
}

// G (gsz doubles per first column), sum_log_diag and info of m first columns to the host.
void read_back(gsum_toep* h, int64_t m, size_t gsz, double* G_out, double* sld_out, int32_t* info_out) {
    SL_CHECK(hipMemcpyAsync(G_out, h->G.p, sizeof(double) * gsz * m, hipMemcpyDeviceToHost, h->stream));
    SL_CHECK(hipMemcpyAsync(sld_out, h->sld.p, sizeof(double) * m, hipMemcpyDeviceToHost, h->stream));
    SL_CHECK(hipMemcpyAsync(info_out, h->info.p, sizeof(int32_t) * m, hipMemcpyDeviceToHost, h->stream));
}

// The first columns of one launch: as many as keep `bytes` each within kYBudget, a grid dimension's 65535 at most, one at least.
int64_t columns_per_launch(int64_t m, size_t bytes, size_t budget = kYBudget) {
    return std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(m, 65535), (int64_t)(budget / bytes)));
}

// What the entry point `who` refuses about the first columns: their order n ...
void check_order(const char* who, int64_t n, int64_t limit = gt::kMaxN, const char* why = "one workgroup holds the generator") {
    if (n > limit) throw Error(std::string(who) + ": n must be <= " + std::to_string(limit) + " (" + why + "), got " + std::to_string(n));
}

// ... and their scale (`with`: what else the hint says to scale).  The right-hand sides are normalised on the device (k_colexp); the
// scale of T reaches the fp32 correction word through lo(L) ~ 2^-53 sqrt(t0) and y ~ 1 / sqrt(t0), which stay far inside fp32's
// range for t0 within 2^-64 .. 2^64.
void check_scale(const char* who, const double* t, int64_t m, int64_t n, const char* with = "") {
    for (int64_t i = 0; i < m; ++i) {
        const double t0 = t[i * n];
        if (t0 > 0.0 && t0 < INFINITY && (t0 < 0x1p-64 || t0 > 0x1p64)) {
            char got[32];
            snprintf(got, sizeof got, "%g", t0);
            throw Error(std::string(who) + ": t[0] must lie within 2^-64 .. 2^64 (scale t by a power of 4" + with + "), got " + std::string(got) +
                        " in first column " + std::to_string(i));
        }
    }
}

// Both, after the counts, for grad and solve.  gram runs the two with its set checks between them, in the order it always refused in.
void check_first_columns(const char* who, const double* t, int64_t m, int64_t n, bool blocked = false) {
    if (m < 1 || n < 1) throw Error(std::string(who) + ": m and n must be >= 1, got " + std::to_string(m) + ", " + std::to_string(n));
    if (blocked)
        check_order(who, n, GSUM_TOEP_BLOCKED_MAX_N, "the grids of the panel kernels");
    else
        check_order(who, n);
    check_scale(who, t, m, n);
}

void check_cols(const char* who, int32_t cols) {
    if (cols < 1 || cols > gt::kMaxCols)
        throw Error(std::string(who) + ": cols must be between 1 and " + std::to_string(gt::kMaxCols) + ", got " + std::to_string(cols));
}

// What gram and grad refuse about the n_sets sets of cols columns (n >= 1): a grid dimension and the int indices of the kernels.
void check_sets(const char* who, int64_t n, int64_t n_sets, int32_t cols) {
    if (n_sets > 65535) throw Error(std::string(who) + ": n_sets must be <= 65535, got " + std::to_string(n_sets));
    if (n_sets * cols > (((int64_t)1 << 31) - 1) / n)
        throw Error(std::string(who) + ": n * n_sets * cols must be < 2^31, got " + std::to_string(n) + " x " + std::to_string(n_sets) + " x " + std::to_string(cols));
}

// alpha of cnt first columns from their xd: As (scaled columns) and, if not null, alpha_out (cnt, n, ncols).
void launch_solve(gsum_toep* h, int n, int ncols, int64_t cnt, const double* xd, const int32_t* info, double* alpha_out) {
    const dim3 grid((unsigned)(n * ncols), (unsigned)cnt);
    gt::k_gs_first<<<grid, gt::kWave, 0, h->stream>>>(xd, n, h->Z.p, h->ze.p, ncols, info, h->W.p);
    SL_LAUNCHED("k_gs_first");
    gt::k_gs_second<<<grid, gt::kWave, 0, h->stream>>>(xd, n, h->W.p, h->ze.p, ncols, info, h->As.p, alpha_out);
    SL_LAUNCHED("k_gs_second");
}

// ---- the panel route ----

// What both routes keep on the device per first column, Y with its correction words and one panel: the bytes, and the buffers of
// `step` first columns in flight.
size_t shared_bytes(int64_t n, int64_t ncols) {
    return (size_t)n * ncols * (sizeof(double) + sizeof(float)) + (size_t)n * gt::kPanelB * (sizeof(double) + sizeof(float));
}
void reserve_shared(gsum_toep* h, int64_t n, int64_t ncols, int64_t step) {
    h->Y.reserve((size_t)n * ncols * step);
    h->Zc.reserve((size_t)n * ncols * step);
    h->Ph.reserve((size_t)n * gt::kPanelB * step);
    h->Pl.reserve((size_t)n * gt::kPanelB * step);
}

// The panel route adds the generator state, four planes of every thread's elements.
size_t panel_state(int64_t n) { return (size_t)4 * gt::kThreads * generator_elements(n); }
size_t panel_bytes(int64_t n, int64_t ncols) { return shared_bytes(n, ncols) + panel_state(n) * sizeof(double); }
void reserve_panel(gsum_toep* h, int64_t n, int64_t ncols, int64_t step) {
    reserve_shared(h, n, ncols, step);
    h->Pst.reserve(panel_state(n) * step);
}

// The scaled right-hand sides h->Z / h->ze into the working residuals h->Y of cnt first columns, their correction words zeroed.
void load_residuals(gsum_toep* h, int n, int ncols, int64_t cnt, int phase) {
    hipStream_t st = h->stream;
    timed(h, phase, [&] {
        gt::k_panel_load<<<dim3((unsigned)((ncols + 31) / 32), (unsigned)((n + 31) / 32)), dim3(32, 8), 0, st>>>(h->Z.p, h->ze.p, n, ncols, (int)cnt, h->Y.p);
        SL_LAUNCHED("k_panel_load");
        SL_CHECK(hipMemsetAsync(h->Zc.p, 0, sizeof(float) * (size_t)n * ncols * cnt, st));
    });
}

// The panel h->Ph / h->Pl of the columns k0 .. of L against every right-hand side: its triangular block, then the rows below it.
void apply_panel(gsum_toep* h, int n, int k0, int ncols, int64_t cnt, const int32_t* info, int phase_diag, int phase_update) {
    hipStream_t st = h->stream;
    timed(h, phase_diag, [&] {
        const dim3 grid((unsigned)((ncols + gt::kDiagThreads - 1) / gt::kDiagThreads), (unsigned)cnt);
        gt::k_panel_diag<<<grid, gt::kDiagThreads, 0, st>>>(h->Ph.p, h->Pl.p, n, k0, ncols, h->Y.p, h->Zc.p, info);
        SL_LAUNCHED("k_panel_diag");
    });
    const int below = n - k0 - gt::kPanelB;                                    // rows under the panel
    if (below > 0)
        timed(h, phase_update, [&] {
            const int wide = 16 * gt::kUpdateTiles;
            const dim3 grid((unsigned)((ncols + wide - 1) / wide), (unsigned)((below + 15) / 16), (unsigned)cnt);
            gt::k_panel_update<<<grid, gt::kWave, 0, st>>>(h->Ph.p, h->Pl.p, n, k0, ncols, h->Y.p, h->Zc.p, info);
            SL_LAUNCHED("k_panel_update");
        });
}

// Y = L^-1 Z of cnt first columns t (device) and the ncols columns h->Z / h->ze, with sum_log_diag and info: per panel of kPanelB
// columns of L the recursion, the triangular block and the trailing update, one after the other on the handle's stream.
void panel_solve(gsum_toep* h, const double* t, int n, int ncols, int64_t cnt, double* sld, int32_t* info) {
    hipStream_t st = h->stream;
    load_residuals(h, n, ncols, cnt, kNUpdate);
    for (int k0 = 0; k0 < n; k0 += gt::kPanelB) {
        timed(h, kNRecursion, [&] {
            with_size_class(n, [&](auto k) {
                using K = decltype(k);
                gt::k_schur_panel<K::E, K::VL><<<(unsigned)cnt, gt::kThreads, 0, st>>>(t, n, k0, h->Pst.p, h->Ph.p, h->Pl.p, sld, info);
            });
            SL_LAUNCHED("k_schur_panel");
        });
        apply_panel(h, n, k0, ncols, cnt, info, kNDiag, kNUpdate);
    }
}

// ---- the blocked route ----

// The blocked route adds the two generator states, the panel's coefficients and the diagonal of L.
size_t blocked_bytes(int64_t n, int64_t ncols) { return shared_bytes(n, ncols) + ((size_t)2 * 4 * n + 4 * gt::kPanelB + n) * sizeof(double); }
void reserve_blocked(gsum_toep* h, int64_t n, int64_t ncols, int64_t step) {
    reserve_shared(h, n, ncols, step);
    h->Bst.reserve((size_t)2 * 4 * n * step);
    h->Bco.reserve((size_t)4 * gt::kPanelB * step);
    h->Bdg.reserve((size_t)n * step);
}

// The phases the blocked recursion charges: the blocked clock's, or the tiled replay's for the entry points that go on to x.
struct BlockedPhases {
    int lead, tiles, diag, update;
};
constexpr BlockedPhases kBlockedClock = {kBLead, kBTiles, kBDiag, kBUpdate};
constexpr BlockedPhases kLevinsonClock = {kLLead, kLTiles, kLDiag, kLUpdate};

// panel_solve with the recursion of a panel split into its lead and its tiles: per panel k_schur_lead, k_schur_tiles (from one state
// buffer into the other), then the panel route's triangular block and trailing update on the panel the tiles stored.  ncols == 0:
// the recursion alone.  keep, (cnt, n, 4), if not null receives what the replay needs in k_coeffs' layout: the lead overwrites its
// panel's (rho, 1 / c) at the next panel, so each panel's rows are moved there after its lead, and row n - 1 takes both words of
// u[n-1] = L[n-1, n-1] from the final state.  A call without keep pays for no copy.
void blocked_recursion(gsum_toep* h, const BlockedPhases& ph, const double* t, int n, int ncols, int64_t cnt, double* sld, int32_t* info, double* keep) {
    hipStream_t st = h->stream;
    const size_t row = sizeof(double) * 4 * n;                                 // of a first column in keep, and of a plane quadruple of the state
    if (ncols) load_residuals(h, n, ncols, cnt, ph.update);
    double* cur = h->Bst.p;
    double* nxt = cur + (size_t)4 * n * cnt;
    timed(h, ph.tiles, [&] {
        gt::k_blocked_init<<<dim3((unsigned)((n + 255) / 256), (unsigned)cnt), 256, 0, st>>>(t, n, cur, info);
        SL_LAUNCHED("k_blocked_init");
    });
    int panels = 0;
    for (int k0 = 0; k0 < n; k0 += gt::kPanelB) {
        timed(h, ph.lead, [&] {
            gt::k_schur_lead<<<(unsigned)cnt, gt::kWave, 0, st>>>(n, k0, cur, h->Bco.p, info);
            SL_LAUNCHED("k_schur_lead");
            const int lead_steps = std::min(k0 + gt::kPanelB, n - 1) - k0;     // the rows k0 .. of keep
            if (keep && lead_steps > 0)
                SL_CHECK(hipMemcpy2DAsync(keep + (size_t)4 * k0, row, h->Bco.p, sizeof(double) * 4 * gt::kPanelB, sizeof(double) * 4 * lead_steps,
                                          (size_t)cnt, hipMemcpyDeviceToDevice, st));
        });
        timed(h, ph.tiles, [&] {
            const dim3 grid((unsigned)((n - 1) / gt::kTileR - k0 / gt::kTileR + 1), (unsigned)cnt);      // the tiles from the pivot's on
            gt::k_schur_tiles<<<grid, gt::kWave, 0, st>>>(n, k0, cur, nxt, h->Bco.p, h->Ph.p, h->Pl.p, h->Bdg.p, info);
            SL_LAUNCHED("k_schur_tiles");
        });
        // both buffers are required: a tile's halo is its upper neighbour's own rows, and nothing orders the tiles of one launch, so a
        // tile may load after its neighbour has stored.  No test sees a single buffer fail (the hardware starts neighbours together).
        std::swap(cur, nxt);
        if (ncols) apply_panel(h, n, k0, ncols, cnt, info, ph.diag, ph.update);
        // a large n has thousands of panels with four event pairs each: settle them every kBlockedSettle panels, which costs one
        // stream synchronisation each time (64 of them at n = 2^20, none before the last panel at n <= 16384)
        if (++panels % kBlockedSettle == 0) settle(h);
    }
    timed(h, ph.tiles, [&] {
        gt::k_blocked_sld<<<(unsigned)cnt, gt::kThreads, 0, st>>>(h->Bdg.p, n, generator_elements(n), sld, info);
        SL_LAUNCHED("k_blocked_sld");
        if (keep)                                                              // the state keeps L_ii in u at and above the pivot: planes 0 and 1, row n - 1
            SL_CHECK(hipMemcpy2DAsync(keep + (size_t)4 * (n - 1), row, cur + (n - 1), row, sizeof(double), (size_t)cnt, hipMemcpyDeviceToDevice, st));
        if (keep)
            SL_CHECK(hipMemcpy2DAsync(keep + (size_t)4 * (n - 1) + 1, row, cur + (size_t)n + (n - 1), row, sizeof(double), (size_t)cnt, hipMemcpyDeviceToDevice, st));
    });
}

void blocked_solve(gsum_toep* h, const double* t, int n, int ncols, int64_t cnt, double* sld, int32_t* info) {
    blocked_recursion(h, kBlockedClock, t, n, ncols, cnt, sld, info, nullptr);
}

// ---- the tiled replay ----

// What the entry points that go on to x keep per first column beside the blocked route's: steps, the two states of A and B, xd, xf
// and the diagonal sums; per right-hand side W, As, with P derivative columns Q, and for the host alpha.
size_t levinson_bytes(int64_t n, int64_t ncols, int64_t P, bool alpha_out) {
    return ((size_t)(4 + 2 * 4 + 2 + 1 + 2) * n + (size_t)n * ncols * (4 + 1 + 2 * P + (alpha_out ? 1 : 0))) * sizeof(double);
}

// launch_levinson on tiles: the rows of steps the blocked recursion kept are (rho, 1 / c) already.  Per panel of kPanelB steps the
// tiles 0 .. (its last step) / kTileR, from one state into the other; both are zero-filled first, and the first panel always runs
// (it sets A[0] = B[0], which is all of n = 1).  Both states are required for the reason blocked_recursion gives.
void tiled_levinson(gsum_toep* h, const double* t, int n, int64_t cnt, const double* steps, double* xd, double* xf, double* sld, int32_t* info) {
    hipStream_t st = h->stream;
    double* cur = h->Lst.p;
    double* nxt = cur + (size_t)4 * n * cnt;
    timed(h, kLLevinson, [&] { SL_CHECK(hipMemsetAsync(cur, 0, sizeof(double) * 2 * 4 * n * cnt, st)); });
    int panels = 0, k0 = 0;
    do {
        timed(h, kLLevinson, [&] {
            const dim3 grid((unsigned)(std::min(k0 + gt::kPanelB, n - 1) / gt::kTileR + 1), (unsigned)cnt);
            gt::k_levinson_tiles<<<grid, gt::kWave, 0, st>>>(t, n, k0, cur, nxt, steps, info);
            SL_LAUNCHED("k_levinson_tiles");
        });
        std::swap(cur, nxt);
        if (++panels % kBlockedSettle == 0) settle(h);
    } while ((k0 += gt::kPanelB) < n - 1);
    timed(h, kLLevinson, [&] {
        gt::k_levinson_finish<<<(unsigned)cnt, gt::kThreads, 0, st>>>(cur, n, steps, xd, xf, sld, info);
        SL_LAUNCHED("k_levinson_finish");
    });
}

// The phases a call of solve_columns is charged to: gsum_toep_solve's are the gradient path's, gsum_toep_loo's the posterior's, and
// those of the two blocked entry points the tiled replay's, with the phases of the blocked recursion (null: the column route).
struct SolvePhases {
    int h2d, schur, levinson, solve, d2h;
    const BlockedPhases* blocked = nullptr;
};

// The body of gsum_toep_solve, gsum_toep_loo and their blocked namesakes (`who`): x = T^-1 e_0 of m first columns by the recursion
// and Levinson's replay, then alpha = T^-1 Z (alpha_out not null) and p = diag(T^-1) (p_out not null) from it.  The recursion needs
// no right-hand side: the column route runs it on one column of zeros, the blocked route without columns.
void solve_columns(const char* who, const SolvePhases& ph, gsum_toep* h, const double* t, int64_t m, int64_t n, const double* Z, int64_t ncols64,
                   double* x_out, double* alpha_out, double* p_out, int32_t* info_out) {
    const std::string name(who);
    const bool blocked = ph.blocked != nullptr;
    if (alpha_out && ncols64 < 1) throw Error(name + ": ncols must be >= 1, got " + std::to_string(ncols64));
    check_first_columns(who, t, m, n, blocked);
    const int64_t nc = alpha_out ? ncols64 : 0;
    if (nc > (((int64_t)1 << 31) - 1) / n) throw Error(name + ": n * ncols must be < 2^31, got " + std::to_string(n) + " x " + std::to_string(nc));
    const int ncols = (int)nc;
    const size_t per_theta = (size_t)n * std::max(ncols, 1);
    const int64_t step = blocked ? columns_per_launch(m, blocked_bytes(n, 0) + levinson_bytes(n, ncols, 0, true), kPanelBudget)
                                 : columns_per_launch(m, 2 * per_theta * sizeof(double));
    run(h, [&] {
        h->t.reserve((size_t)m * n);
        h->Z.reserve(per_theta + n);                                       // the right-hand sides, then one column of zeros
        h->ze.reserve((size_t)ncols + 1);
        if (blocked) {
            reserve_blocked(h, n, 0, step);
            h->Lst.reserve((size_t)2 * 4 * n * step);
        } else {
            h->Y.reserve((size_t)n * step);
        }
        h->steps.reserve((size_t)4 * n * step);
        h->xd.reserve((size_t)2 * n * step);
        h->xf.reserve((size_t)n * m);
        h->sld.reserve((size_t)m);
        h->info.reserve((size_t)m);
        if (p_out) h->pd.reserve((size_t)n * m);
        if (ncols) {
            h->As.reserve(per_theta * step);
            h->Aout.reserve(per_theta * step);
            h->W.reserve(4 * per_theta * step);
        }
        hipStream_t st = h->stream;
        // the column route's recursion runs on one column of zeros, kept after the ncols of Z
        double* zero = h->Z.p + (size_t)n * ncols;
        int32_t* zero_e = h->ze.p + ncols;
        timed(h, ph.h2d, [&] {
            SL_CHECK(hipMemcpyAsync(h->t.p, t, sizeof(double) * m * n, hipMemcpyHostToDevice, st));
            if (ncols) SL_CHECK(hipMemcpyAsync(h->Z.p, Z, sizeof(double) * n * ncols, hipMemcpyHostToDevice, st));
            if (!blocked) {
                SL_CHECK(hipMemsetAsync(zero, 0, sizeof(double) * n, st));
                SL_CHECK(hipMemsetAsync(zero_e, 0, sizeof(int32_t), st));
            }
        });
        if (ncols) timed(h, ph.schur, [&] { launch_colexp(h, (int)n, ncols); });
        for (int64_t lo = 0; lo < m; lo += step) {
            const int64_t cnt = std::min(step, m - lo);
            const double* tl = h->t.p + lo * n;
            int32_t* il = h->info.p + lo;
            if (blocked) {
                blocked_recursion(h, *ph.blocked, tl, (int)n, 0, cnt, h->sld.p + lo, il, h->steps.p);
                tiled_levinson(h, tl, (int)n, cnt, h->steps.p, h->xd.p, h->xf.p + lo * n, h->sld.p + lo, il);
            } else {
                timed(h, ph.schur, [&] { launch_schur<true>(h, tl, (int)n, zero, zero_e, 1, cnt, h->Y.p, h->sld.p + lo, il, h->steps.p); });
                timed(h, ph.levinson, [&] { launch_levinson(h, tl, (int)n, cnt, h->steps.p, h->xd.p, h->xf.p + lo * n, h->sld.p + lo, il); });
            }
            if (p_out)
                timed(h, ph.solve, [&] {
                    if (blocked)
                        gt::k_invdiag_n<<<(unsigned)cnt, gt::kThreads, 0, st>>>(h->xd.p, (int)n, generator_elements(n), il, h->pd.p + lo * n);
                    else
                        with_size_class((int)n, [&](auto k) {
                            gt::k_invdiag<decltype(k)::E><<<(unsigned)cnt, gt::kThreads, 0, st>>>(h->xd.p, (int)n, il, h->pd.p + lo * n);
                        });
                    SL_LAUNCHED("k_invdiag");
                });
            if (ncols) {
                timed(h, ph.solve, [&] { launch_solve(h, (int)n, ncols, cnt, h->xd.p, il, h->Aout.p); });
                timed(h, ph.d2h, [&] {
                    SL_CHECK(hipMemcpyAsync(alpha_out + (size_t)lo * per_theta, h->Aout.p, sizeof(double) * per_theta * cnt, hipMemcpyDeviceToHost, st));
                });
            }
        }
        timed(h, ph.d2h, [&] {
            if (x_out) SL_CHECK(hipMemcpyAsync(x_out, h->xf.p, sizeof(double) * m * n, hipMemcpyDeviceToHost, st));
            if (p_out) SL_CHECK(hipMemcpyAsync(p_out, h->pd.p, sizeof(double) * m * n, hipMemcpyDeviceToHost, st));
            SL_CHECK(hipMemcpyAsync(info_out, h->info.p, sizeof(int32_t) * m, hipMemcpyDeviceToHost, st));
        });
    });
}

// The phases a call of grad_route is charged to: gsum_toep_grad's are the gradient path's, gsum_toep_grad_blocked's the tiled
// replay's, with the phases of the blocked recursion (null: the column route).
struct GradPhases {
    int h2d, schur, levinson, gram, diag, solve, contract, d2h;
    const BlockedPhases* blocked = nullptr;
};

// The body of gsum_toep_grad and gsum_toep_grad_blocked (`who`).  They differ in the recursion that leaves Y, sum_log_diag, info and
// the coefficients, in the replay that leaves x, and in the limit and the memory that come with those; the kernels from x on are one.
void grad_route(const char* who, const GradPhases& ph, gsum_toep* h, const double* t, int64_t m, int64_t n, const double* dt, int64_t P, const double* Z,
                int64_t n_sets, int32_t cols, double* G_out, double* sld_out, int32_t* info_out, double* trace_out, double* H_out) {
    const std::string name(who);
    const bool blocked = ph.blocked != nullptr;
    if (!h || !t || !dt || !Z || !G_out || !sld_out || !info_out || !trace_out || !H_out) throw Error(name + ": null pointer argument");
    if (n_sets < 1) throw Error(name + ": n_sets must be >= 1, got " + std::to_string(n_sets));
    if (P < 1 || P > 65535) throw Error(name + ": P must be between 1 and 65535, got " + std::to_string(P));
    check_cols(who, cols);
    check_first_columns(who, t, m, n, blocked);
    check_sets(who, n, n_sets, cols);
    if ((int64_t)cols * cols * P > ((int64_t)1 << 31) - 1) throw Error(name + ": cols * cols * P must be < 2^31");
    const int ncols = (int)(n_sets * cols);
    const size_t per_theta = (size_t)n * ncols;                                // doubles of Y, and of alpha, per first column
    const int64_t step = blocked ? columns_per_launch(m, blocked_bytes(n, ncols) + levinson_bytes(n, ncols, P, false), kPanelBudget)
                                 : columns_per_launch(m, 2 * per_theta * sizeof(double));
    const size_t gsz = (size_t)n_sets * cols * cols, hsz = gsz * (size_t)P;
    run(h, [&] {
        h->t.reserve((size_t)m * n);
        h->dt.reserve((size_t)m * P * n);
        h->Z.reserve(per_theta);
        if (blocked) {
            reserve_blocked(h, n, ncols, step);
            h->Lst.reserve((size_t)2 * 4 * n * step);
        } else {
            h->Y.reserve(per_theta * step);
        }
        h->As.reserve(per_theta * step);
        h->W.reserve(4 * per_theta * step);
        h->Q.reserve(2 * per_theta * step * P);
        h->steps.reserve((size_t)4 * n * step);
        h->xd.reserve((size_t)2 * n * step);
        h->xf.reserve((size_t)n * step);
        h->sd.reserve((size_t)2 * n * step);
        h->G.reserve(gsz * m);
        h->H.reserve(hsz * m);
        h->trace.reserve((size_t)m * P);
        h->sld.reserve((size_t)m);
        h->info.reserve((size_t)m);
        h->ze.reserve((size_t)ncols);
        hipStream_t st = h->stream;
        timed(h, ph.h2d, [&] {
            SL_CHECK(hipMemcpyAsync(h->t.p, t, sizeof(double) * m * n, hipMemcpyHostToDevice, st));
            SL_CHECK(hipMemcpyAsync(h->dt.p, dt, sizeof(double) * m * P * n, hipMemcpyHostToDevice, st));
            SL_CHECK(hipMemcpyAsync(h->Z.p, Z, sizeof(double) * per_theta, hipMemcpyHostToDevice, st));
        });
        timed(h, ph.schur, [&] { launch_colexp(h, (int)n, ncols); });
        for (int64_t lo = 0; lo < m; lo += step) {
            const int64_t cnt = std::min(step, m - lo);
            const double* tl = h->t.p + lo * n;
            int32_t* il = h->info.p + lo;
            if (blocked) {
                blocked_recursion(h, *ph.blocked, tl, (int)n, ncols, cnt, h->sld.p + lo, il, h->steps.p);
                tiled_levinson(h, tl, (int)n, cnt, h->steps.p, h->xd.p, h->xf.p, h->sld.p + lo, il);
            } else {
                timed(h, ph.schur, [&] { launch_schur<true>(h, tl, (int)n, h->Z.p, h->ze.p, ncols, cnt, h->Y.p, h->sld.p + lo, il, h->steps.p); });
                timed(h, ph.levinson, [&] { launch_levinson(h, tl, (int)n, cnt, h->steps.p, h->xd.p, h->xf.p, h->sld.p + lo, il); });
            }
            timed(h, ph.gram, [&] { launch_gram(h, (int)n, cols, (int)n_sets, cnt, il, h->G.p + gsz * lo); });
            timed(h, ph.diag, [&] {
                gt::k_diagsums<<<dim3((unsigned)n, (unsigned)cnt), gt::kWave, 0, st>>>(h->xd.p, (int)n, il, h->sd.p);
                SL_LAUNCHED("k_diagsums");
                gt::k_traces<<<dim3((unsigned)P, (unsigned)cnt), gt::kWave, 0, st>>>(h->sd.p, h->dt.p + lo * P * n, (int)n, (int)P, il,
                                                                                     h->trace.p + lo * P);
                SL_LAUNCHED("k_traces");
            });
            timed(h, ph.solve, [&] { launch_solve(h, (int)n, ncols, cnt, h->xd.p, il, nullptr); });
            timed(h, ph.contract, [&] {
                gt::k_tprod<<<dim3((unsigned)(n * ncols), (unsigned)P, (unsigned)cnt), gt::kWave, 0, st>>>(h->dt.p + lo * P * n, (int)n, (int)P,
                                                                                                        h->As.p, ncols, il, h->Q.p);
                SL_LAUNCHED("k_tprod");
                gt::k_hdot<<<dim3((unsigned)(cols * cols * P), (unsigned)n_sets, (unsigned)cnt), gt::kWave, 0, st>>>(
                    h->As.p, h->Q.p, (int)n, (int)P, cols, (int)n_sets, h->ze.p, il, h->H.p + hsz * lo);
                SL_LAUNCHED("k_hdot");
            });
        }
        timed(h, ph.d2h, [&] {
            read_back(h, m, gsz, G_out, sld_out, info_out);
            SL_CHECK(hipMemcpyAsync(H_out, h->H.p, sizeof(double) * hsz * m, hipMemcpyDeviceToHost, st));
            SL_CHECK(hipMemcpyAsync(trace_out, h->trace.p, sizeof(double) * m * P, hipMemcpyDeviceToHost, st));
        });
    });
}

// What the panel and the blocked entry points differ in: the limit on n, the phases they charge, the device memory of a first
// column, and the solve.  Everything around the solve is one code (gram_route, predict_route).
struct Route {
    int64_t max_n;
    const char* why;                                                           // what bounds n, for the refusal
    int h2d, prepare, sums, cov, d2h;
    size_t (*bytes)(int64_t, int64_t);
    void (*reserve)(gsum_toep*, int64_t, int64_t, int64_t);
    void (*solve)(gsum_toep*, const double*, int, int, int64_t, double*, int32_t*);
};
const Route kPanelRoute = {gt::kMaxN, "one workgroup holds the generator", kNH2D, kNUpdate, kNSums, kNCov, kND2H, panel_bytes, reserve_panel, panel_solve};
const Route kBlockedRoute = {GSUM_TOEP_BLOCKED_MAX_N, "the grids of the panel kernels", kBH2D, kBUpdate, kBSums, kBCov, kBD2H, blocked_bytes, reserve_blocked,
                             blocked_solve};

// The body of gsum_toep_gram_panel and gsum_toep_gram_blocked (`who`).
void gram_route(const char* who, const Route& r, gsum_toep* h, const double* t, int64_t m, int64_t n, const double* Z, int64_t n_sets, int32_t cols,
                double* G_out, double* sld_out, int32_t* info_out) {
    const std::string name(who);
    if (!h || !t || !Z || !G_out || !sld_out || !info_out) throw Error(name + ": null pointer argument");
    if (m < 1 || n < 1 || n_sets < 1)
        throw Error(name + ": m, n and n_sets must be >= 1, got " + std::to_string(m) + ", " + std::to_string(n) + ", " + std::to_string(n_sets));
    check_cols(who, cols);
    check_order(who, n, r.max_n, r.why);
    check_sets(who, n, n_sets, cols);
    check_scale(who, t, m, n, " and G and sum_log_diag with it");
    const int ncols = (int)(n_sets * cols);
    const size_t per_theta = (size_t)n * ncols;
    const int64_t step = columns_per_launch(m, r.bytes(n, ncols), kPanelBudget);
    const size_t gsz = (size_t)n_sets * cols * cols;
    run(h, [&] {
        h->t.reserve((size_t)m * n);
        h->Z.reserve(per_theta);
        r.reserve(h, n, ncols, step);
        h->G.reserve(gsz * m);
        h->sld.reserve((size_t)m);
        h->info.reserve((size_t)m);
        h->ze.reserve((size_t)ncols);
        hipStream_t st = h->stream;
        timed(h, r.h2d, [&] {
            SL_CHECK(hipMemcpyAsync(h->t.p, t, sizeof(double) * m * n, hipMemcpyHostToDevice, st));
            SL_CHECK(hipMemcpyAsync(h->Z.p, Z, sizeof(double) * per_theta, hipMemcpyHostToDevice, st));
        });
        timed(h, r.prepare, [&] { launch_colexp(h, (int)n, ncols); });
        for (int64_t lo = 0; lo < m; lo += step) {
            const int64_t cnt = std::min(step, m - lo);
            int32_t* il = h->info.p + lo;
            r.solve(h, h->t.p + lo * n, (int)n, ncols, cnt, h->sld.p + lo, il);
            timed(h, r.sums, [&] { launch_gram(h, (int)n, cols, (int)n_sets, cnt, il, h->G.p + gsz * lo); });
        }
        timed(h, r.d2h, [&] { read_back(h, m, gsz, G_out, sld_out, info_out); });
    });
}

// The body of gsum_toep_predict_panel and gsum_toep_predict_blocked (`who`).
void predict_route(const char* who, const Route& r, gsum_toep* h, const double* t, int64_t n, const double* K, int64_t q, const double* Z, int32_t c,
                   double* quad_out, double* cross_out, double* cov_out, double* G_out, double* sld_out, int32_t* info_out) {
    const std::string name(who);
    if (!h || !t || !K || !quad_out || !sld_out || !info_out) throw Error(name + ": null pointer argument");
    if (q < 1 || n < 1) throw Error(name + ": n and q must be >= 1, got " + std::to_string(n) + ", " + std::to_string(q));
    if (c < 0 || c > gt::kMaxCols) throw Error(name + ": c must be between 0 and " + std::to_string(gt::kMaxCols) + ", got " + std::to_string(c));
    if (c > 0 && (!Z || !cross_out || !G_out)) throw Error(name + ": null pointer argument (Z, cross_out and G_out with c > 0)");
    check_order(who, n, r.max_n, r.why);
    if (q > (((int64_t)1 << 31) - 1) / n - c)
        throw Error(name + ": n * (q + c) must be < 2^31, got " + std::to_string(n) + " x (" + std::to_string(q) + " + " + std::to_string(c) + ")");
    if (cov_out && q > 16 * 65535) throw Error(name + ": cov_out takes q <= 1048560, got " + std::to_string(q));
    check_scale(who, t, 1, n, " and the outputs with it");
    const int ncols = (int)(q + c), qi = (int)q;
    const size_t ny = (size_t)n * ncols;
    run(h, [&] {
        h->t.reserve((size_t)n);
        h->Z.reserve(ny);
        r.reserve(h, n, ncols, 1);
        h->ze.reserve((size_t)ncols);
        h->sld.reserve(1);
        h->info.reserve(1);
        h->quad.reserve((size_t)q);
        if (c) {
            h->cross.reserve((size_t)q * c);
            h->Yz.reserve((size_t)n * c);
            h->G.reserve((size_t)c * c);
        }
        if (cov_out) h->cov.reserve((size_t)q * q);
        hipStream_t st = h->stream;
        timed(h, r.h2d, [&] {
            SL_CHECK(hipMemcpyAsync(h->t.p, t, sizeof(double) * n, hipMemcpyHostToDevice, st));
            SL_CHECK(hipMemcpyAsync(h->Z.p, K, sizeof(double) * n * q, hipMemcpyHostToDevice, st));
            if (c) SL_CHECK(hipMemcpyAsync(h->Z.p + (size_t)n * q, Z, sizeof(double) * n * c, hipMemcpyHostToDevice, st));
        });
        timed(h, r.prepare, [&] { launch_colexp(h, (int)n, ncols); });
        r.solve(h, h->t.p, (int)n, ncols, 1, h->sld.p, h->info.p);
        timed(h, r.sums, [&] {
            gt::k_pred_sums<<<dim3((unsigned)q, (unsigned)(1 + c)), gt::kWave, 0, st>>>(h->Y.p, (int)n, qi, c, h->ze.p, h->info.p, h->quad.p, h->cross.p);
            SL_LAUNCHED("k_pred_sums");
            if (c) {                                                           // the residual columns alone, as one set of k_gram's
                SL_CHECK(hipMemcpy2DAsync(h->Yz.p, sizeof(double) * c, h->Y.p + q, sizeof(double) * ncols, sizeof(double) * c, (size_t)n,
                                          hipMemcpyDeviceToDevice, st));
                gt::k_gram<<<dim3((unsigned)c, 1, 1), gt::kWave, 0, st>>>(h->Yz.p, (int)n, c, 1, h->ze.p + q, h->info.p, h->G.p);
                SL_LAUNCHED("k_gram");
            }
        });
        if (cov_out)
            timed(h, r.cov, [&] {
                const unsigned tiles = (unsigned)((q + 15) / 16);
                gt::k_pred_cov<<<dim3(tiles, tiles), gt::kWave, 0, st>>>(h->Y.p, (int)n, qi, c, h->ze.p, h->info.p, h->cov.p);
                SL_LAUNCHED("k_pred_cov");
            });
        timed(h, r.d2h, [&] {
            SL_CHECK(hipMemcpyAsync(quad_out, h->quad.p, sizeof(double) * q, hipMemcpyDeviceToHost, st));
            if (c) {
                SL_CHECK(hipMemcpyAsync(cross_out, h->cross.p, sizeof(double) * q * c, hipMemcpyDeviceToHost, st));
                SL_CHECK(hipMemcpyAsync(G_out, h->G.p, sizeof(double) * c * c, hipMemcpyDeviceToHost, st));
            }
            if (cov_out) SL_CHECK(hipMemcpyAsync(cov_out, h->cov.p, sizeof(double) * q * q, hipMemcpyDeviceToHost, st));
            SL_CHECK(hipMemcpyAsync(sld_out, h->sld.p, sizeof(double), hipMemcpyDeviceToHost, st));
            SL_CHECK(hipMemcpyAsync(info_out, h->info.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        });
    });
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
        check_cols("gsum_toep_gram", cols);
        check_order("gsum_toep_gram", n);
        check_sets("gsum_toep_gram", n, n_sets, cols);
        check_scale("gsum_toep_gram", t, m, n, " and G and sum_log_diag with it");
        const int ncols = (int)(n_sets * cols);
        const size_t per_theta = (size_t)n * ncols;                            // doubles of Y per first column
        const int64_t step = columns_per_launch(m, per_theta * sizeof(double));
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
            timed(h, kSchur, [&] { launch_colexp(h, (int)n, ncols); });
            for (int64_t lo = 0; lo < m; lo += step) {
                const int64_t cnt = std::min(step, m - lo);
                int32_t* il = h->info.p + lo;
                timed(h, kSchur, [&] {
                    launch_schur<false>(h, h->t.p + lo * n, (int)n, h->Z.p, h->ze.p, ncols, cnt, h->Y.p, h->sld.p + lo, il, nullptr);
                });
                timed(h, kGram, [&] { launch_gram(h, (int)n, cols, (int)n_sets, cnt, il, h->G.p + gsz * lo); });
            }
            timed(h, kD2H, [&] { read_back(h, m, gsz, G_out, sld_out, info_out); });
        });
    });
}

GT_API int gsum_toep_times(gsum_toep* h, double* ms, int32_t reset) {
    return guarded([&] {
        if (!h || !ms) throw Error("gsum_toep_times: null pointer argument");
        read_times(h, 0, kPhases, ms, reset);
    });
}

GT_API int gsum_toep_grad(gsum_toep* h, const double* t, int64_t m, int64_t n, const double* dt, int64_t P, const double* Z, int64_t n_sets,
                          int32_t cols, double* G_out, double* sld_out, int32_t* info_out, double* trace_out, double* H_out) {
    return guarded([&] {
        grad_route("gsum_toep_grad", {kGH2D, kGSchur, kGLevinson, kGGram, kGDiag, kGSolve, kGContract, kGD2H}, h, t, m, n, dt, P, Z, n_sets, cols, G_out,
                   sld_out, info_out, trace_out, H_out);
    });
}

GT_API int gsum_toep_solve(gsum_toep* h, const double* t, int64_t m, int64_t n, const double* Z, int64_t ncols64, double* x_out,
                           double* alpha_out, int32_t* info_out) {
    return guarded([&] {
        if (!h || !t || !info_out || (!x_out && !alpha_out) || (alpha_out && !Z)) throw Error("gsum_toep_solve: null pointer argument");
        solve_columns("gsum_toep_solve", {kGH2D, kGSchur, kGLevinson, kGSolve, kGD2H}, h, t, m, n, Z, ncols64, x_out, alpha_out, nullptr, info_out);
    });
}

GT_API int gsum_toep_grad_times(gsum_toep* h, double* ms, int32_t reset) {
    return guarded([&] {
        if (!h || !ms) throw Error("gsum_toep_grad_times: null pointer argument");
        read_times(h, kPhases, kAllPhases - kPhases, ms, reset);
    });
}

GT_API int gsum_toep_loo(gsum_toep* h, const double* t, int64_t m, int64_t n, const double* Z, int64_t ncols, double* p_out, double* alpha_out,
                         int32_t* info_out) {
    return guarded([&] {
        if (!h || !t || !p_out || !info_out || (alpha_out && !Z)) throw Error("gsum_toep_loo: null pointer argument");
        solve_columns("gsum_toep_loo", {kPH2D, kPSchur, kPLevinson, kPSolve, kPD2H}, h, t, m, n, Z, ncols, nullptr, alpha_out, p_out, info_out);
    });
}

GT_API int gsum_toep_predict(gsum_toep* h, const double* t, int64_t n, const double* K, int64_t q, const double* Z, int32_t c, double* quad_out,
                             double* cross_out, double* cov_out, double* G_out, double* sld_out, int32_t* info_out) {
    return guarded([&] {
        if (!h || !t || !K || !quad_out || !sld_out || !info_out) throw Error("gsum_toep_predict: null pointer argument");
        if (q < 1 || n < 1) throw Error("gsum_toep_predict: n and q must be >= 1, got " + std::to_string(n) + ", " + std::to_string(q));
        if (c < 0 || c > gt::kMaxCols)
            throw Error("gsum_toep_predict: c must be between 0 and " + std::to_string(gt::kMaxCols) + ", got " + std::to_string(c));
        if (c > 0 && (!Z || !cross_out || !G_out)) throw Error("gsum_toep_predict: null pointer argument (Z, cross_out and G_out with c > 0)");
        check_order("gsum_toep_predict", n);
        if (q > (((int64_t)1 << 31) - 1) / n - c)
            throw Error("gsum_toep_predict: n * (q + c) must be < 2^31, got " + std::to_string(n) + " x (" + std::to_string(q) + " + " + std::to_string(c) + ")");
        if (cov_out && q > 16 * 65535) throw Error("gsum_toep_predict: cov_out takes q <= 1048560, got " + std::to_string(q));
        check_scale("gsum_toep_predict", t, 1, n, " and the outputs with it");
        const int ncols = (int)(q + c), qi = (int)q;
        const size_t ny = (size_t)n * ncols;
        run(h, [&] {
            h->t.reserve((size_t)n);
            h->Z.reserve(ny);
            h->Y.reserve(ny);
            h->ze.reserve((size_t)ncols);
            h->sld.reserve(1);
            h->info.reserve(1);
            h->quad.reserve((size_t)q);
            if (c) {
                h->cross.reserve((size_t)q * c);
                h->Yz.reserve((size_t)n * c);
                h->G.reserve((size_t)c * c);
            }
            if (cov_out) h->cov.reserve((size_t)q * q);
            hipStream_t st = h->stream;
            timed(h, kPH2D, [&] {
                SL_CHECK(hipMemcpyAsync(h->t.p, t, sizeof(double) * n, hipMemcpyHostToDevice, st));
                SL_CHECK(hipMemcpyAsync(h->Z.p, K, sizeof(double) * n * q, hipMemcpyHostToDevice, st));
                if (c) SL_CHECK(hipMemcpyAsync(h->Z.p + (size_t)n * q, Z, sizeof(double) * n * c, hipMemcpyHostToDevice, st));
            });
            timed(h, kPSchur, [&] {
                launch_colexp(h, (int)n, ncols);
                launch_schur<false>(h, h->t.p, (int)n, h->Z.p, h->ze.p, ncols, 1, h->Y.p, h->sld.p, h->info.p, nullptr);
            });
            timed(h, kPSums, [&] {
                gt::k_pred_sums<<<dim3((unsigned)q, (unsigned)(1 + c)), gt::kWave, 0, st>>>(h->Y.p, (int)n, qi, c, h->ze.p, h->info.p, h->quad.p,
                                                                                          h->cross.p);
                SL_LAUNCHED("k_pred_sums");
                if (c) {                                                       // the residual columns alone, as one set of k_gram's
                    SL_CHECK(hipMemcpy2DAsync(h->Yz.p, sizeof(double) * c, h->Y.p + q, sizeof(double) * ncols, sizeof(double) * c, (size_t)n,
                                              hipMemcpyDeviceToDevice, st));
                    gt::k_gram<<<dim3((unsigned)c, 1, 1), gt::kWave, 0, st>>>(h->Yz.p, (int)n, c, 1, h->ze.p + q, h->info.p, h->G.p);
                    SL_LAUNCHED("k_gram");
                }
            });
            if (cov_out)
                timed(h, kPCov, [&] {
                    const unsigned tiles = (unsigned)((q + 15) / 16);
                    gt::k_pred_cov<<<dim3(tiles, tiles), gt::kWave, 0, st>>>(h->Y.p, (int)n, qi, c, h->ze.p, h->info.p, h->cov.p);
                    SL_LAUNCHED("k_pred_cov");
                });
            timed(h, kPD2H, [&] {
                SL_CHECK(hipMemcpyAsync(quad_out, h->quad.p, sizeof(double) * q, hipMemcpyDeviceToHost, st));
                if (c) {
                    SL_CHECK(hipMemcpyAsync(cross_out, h->cross.p, sizeof(double) * q * c, hipMemcpyDeviceToHost, st));
                    SL_CHECK(hipMemcpyAsync(G_out, h->G.p, sizeof(double) * c * c, hipMemcpyDeviceToHost, st));
                }
                if (cov_out) SL_CHECK(hipMemcpyAsync(cov_out, h->cov.p, sizeof(double) * q * q, hipMemcpyDeviceToHost, st));
                SL_CHECK(hipMemcpyAsync(sld_out, h->sld.p, sizeof(double), hipMemcpyDeviceToHost, st));
                SL_CHECK(hipMemcpyAsync(info_out, h->info.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
            });
        });
    });
}

GT_API int gsum_toep_post_times(gsum_toep* h, double* ms, int32_t reset) {
    return guarded([&] {
        if (!h || !ms) throw Error("gsum_toep_post_times: null pointer argument");
        read_times(h, kAllPhases, kEveryPhase - kAllPhases, ms, reset);
    });
}

GT_API int32_t gsum_toep_panel_width(const gsum_toep*) { return gt::kPanelB; }

GT_API int gsum_toep_gram_panel(gsum_toep* h, const double* t, int64_t m, int64_t n, const double* Z, int64_t n_sets, int32_t cols, double* G_out,
                                double* sld_out, int32_t* info_out) {
    return guarded([&] { gram_route("gsum_toep_gram_panel", kPanelRoute, h, t, m, n, Z, n_sets, cols, G_out, sld_out, info_out); });
}

GT_API int gsum_toep_predict_panel(gsum_toep* h, const double* t, int64_t n, const double* K, int64_t q, const double* Z, int32_t c,
                                   double* quad_out, double* cross_out, double* cov_out, double* G_out, double* sld_out, int32_t* info_out) {
    return guarded([&] {
        predict_route("gsum_toep_predict_panel", kPanelRoute, h, t, n, K, q, Z, c, quad_out, cross_out, cov_out, G_out, sld_out, info_out);
    });
}

GT_API int gsum_toep_panel_times(gsum_toep* h, double* ms, int32_t reset) {
    return guarded([&] {
        if (!h || !ms) throw Error("gsum_toep_panel_times: null pointer argument");
        read_times(h, kEveryPhase, kTotalPhases - kEveryPhase, ms, reset);
    });
}

GT_API int64_t gsum_toep_blocked_max_n(const gsum_toep*) { return GSUM_TOEP_BLOCKED_MAX_N; }

GT_API int32_t gsum_toep_blocked_tile_rows(const gsum_toep*) { return gt::kTileR; }

GT_API int gsum_toep_gram_blocked(gsum_toep* h, const double* t, int64_t m, int64_t n, const double* Z, int64_t n_sets, int32_t cols, double* G_out,
                                  double* sld_out, int32_t* info_out) {
    return guarded([&] { gram_route("gsum_toep_gram_blocked", kBlockedRoute, h, t, m, n, Z, n_sets, cols, G_out, sld_out, info_out); });
}

GT_API int gsum_toep_predict_blocked(gsum_toep* h, const double* t, int64_t n, const double* K, int64_t q, const double* Z, int32_t c,
                                     double* quad_out, double* cross_out, double* cov_out, double* G_out, double* sld_out, int32_t* info_out) {
    return guarded([&] {
        predict_route("gsum_toep_predict_blocked", kBlockedRoute, h, t, n, K, q, Z, c, quad_out, cross_out, cov_out, G_out, sld_out, info_out);
    });
}

GT_API int gsum_toep_blocked_times(gsum_toep* h, double* ms, int32_t reset) {
    return guarded([&] {
        if (!h || !ms) throw Error("gsum_toep_blocked_times: null pointer argument");
        read_times(h, kTotalPhases, kGrandPhases - kTotalPhases, ms, reset);
    });
}

GT_API int gsum_toep_grad_blocked(gsum_toep* h, const double* t, int64_t m, int64_t n, const double* dt, int64_t P, const double* Z, int64_t n_sets,
                                  int32_t cols, double* G_out, double* sld_out, int32_t* info_out, double* trace_out, double* H_out) {
    return guarded([&] {
        grad_route("gsum_toep_grad_blocked", {kLH2D, kLUpdate, kLLevinson, kLGram, kLDiagsums, kLSolve, kLContract, kLD2H, &kLevinsonClock}, h, t, m, n, dt,
                   P, Z, n_sets, cols, G_out, sld_out, info_out, trace_out, H_out);
    });
}

GT_API int gsum_toep_solve_blocked(gsum_toep* h, const double* t, int64_t m, int64_t n, const double* Z, int64_t ncols64, double* x_out,
                                   double* alpha_out, int32_t* info_out) {
    return guarded([&] {
        if (!h || !t || !info_out || (!x_out && !alpha_out) || (alpha_out && !Z)) throw Error("gsum_toep_solve_blocked: null pointer argument");
        solve_columns("gsum_toep_solve_blocked", {kLH2D, kLUpdate, kLLevinson, kLSolve, kLD2H, &kLevinsonClock}, h, t, m, n, Z, ncols64, x_out, alpha_out,
                      nullptr, info_out);
    });
}

GT_API int gsum_toep_loo_blocked(gsum_toep* h, const double* t, int64_t m, int64_t n, const double* Z, int64_t ncols, double* p_out,
                                 double* alpha_out, int32_t* info_out) {
    return guarded([&] {
        if (!h || !t || !p_out || !info_out || (alpha_out && !Z)) throw Error("gsum_toep_loo_blocked: null pointer argument");
        solve_columns("gsum_toep_loo_blocked", {kLH2D, kLUpdate, kLLevinson, kLSolve, kLD2H, &kLevinsonClock}, h, t, m, n, Z, ncols, nullptr, alpha_out,
                      p_out, info_out);
    });
}

GT_API int gsum_toep_levinson_times(gsum_toep* h, double* ms, int32_t reset) {
    return guarded([&] {
        if (!h || !ms) throw Error("gsum_toep_levinson_times: null pointer argument");
        read_times(h, kGrandPhases, kUltimatePhases - kGrandPhases, ms, reset);
    });
}
