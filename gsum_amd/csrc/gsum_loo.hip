// libgsum_loo.so: the C ABI of include/gsum_loo.h (leave-one-out and leave-group-out diagnostics).  Kernels: kernels/loo.hip.h.
#include <utility>
#include <vector>

#include "gsum_loo.h"
#include "host/sidelib.hip.h"
#include "kernels/loo.hip.h"

#define GL_API extern "C" __attribute__((visibility("default")))

namespace {

enum Phase { kUpload = 0, kInverse, kReduce, kH2D, kSolve, kD2H, kPhases,        // gsum_loo_times
             kFGather = kPhases, kFGram, kFFactor, kFInverse, kFLogdet, kFApply, kFScatter, kAllPhases };    // gsum_loo_fold_times
constexpr int kFoldPhases = kAllPhases - kPhases;
constexpr int64_t kMaxN = (int64_t)1 << 20;        // keeps every byte count below far inside int64; no device holds such a matrix
constexpr int64_t kChunk = 512;                    // the columns of R one pair of solve launches takes
constexpr int64_t kMaxGroups = 32768;              // the groups of one chunk: they ride on a grid dimension

}  // namespace

struct gsum_loo : TimedHandle<kAllPhases> {
    int64_t n = 0, N = 0;                          // the order of L, and n rounded up to loo::kBlock
    DevBuf<double> W;                              // N x N: the inverse of the padded factor
    DevBuf<double, true> R, Y;                     // N x ldr each: a chunk of right-hand sides and its forward product
    std::vector<double> p;                         // n
    double sum_log_diag = 0;
    int64_t fold_budget = 0;                       // bytes one chunk of groups may take; 0: what hipMemGetInfo leaves
};

namespace {

// The levels of the recursive doubling above the diagonal blocks, for `count` matrices of leading dimension N, N * N elements apart
// (sizes: their orders on the device, or nullptr for one matrix of order N).
void merge_levels(hipStream_t st, const double* Ld, double* W, double* T, int64_t N, int64_t count, const int64_t* sizes) {
    for (int64_t g = 2 * loo::kBlock; g / 2 < N; g *= 2) {
        const int64_t pairs = (N - g / 2 + g - 1) / g, tiles = (g / 2 / loo::kTile) * (g / 2 / loo::kTile);
        const dim3 grid((unsigned)tiles, (unsigned)pairs, (unsigned)count);
        loo::k_merge<0><<<grid, 256, 0, st>>>(Ld, W, T, N, g, N * N, sizes);
        loo::k_merge<1><<<grid, 256, 0, st>>>(Ld, W, T, N, g, N * N, sizes);
        loo::k_merge<2><<<grid, 256, 0, st>>>(Ld, W, T, N, g, N * N, sizes);
        loo::k_merge<3><<<grid, 256, 0, st>>>(Ld, W, T, N, g, N * N, sizes);
        SL_LAUNCHED("k_merge");
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
            loo::k_invert_diag<<<(unsigned)nb, loo::kBlock, loo::kInvertLds, st>>>(Ld, h->W.p, N, h->n, info.p, logs.p, 0, nullptr, 0, nb);
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
            merge_levels(st, Ld, h->W.p, T, N, 1, nullptr);
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
                    loo::k_colsq_partial<<<dim3((unsigned)nb, (unsigned)nb), loo::kBlock, 0, st>>>(h->W.p, N, partial.p, 0, 0, nullptr);
                    SL_LAUNCHED("k_colsq_partial");
                    loo::k_colsq_total<<<(unsigned)nb, loo::kBlock, 0, st>>>(partial.p, N, pd.p, 0, nullptr);
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

namespace {

// (L L^T)^-1 R for the n x k host matrix R, in chunks of kChunk columns; a chunk's n x kc result goes to the host matrix alpha
// (n x k) or, where alpha is null, to the device matrix A of leading dimension lda, at the chunk's columns.
void solve_columns(gsum_loo* h, const double* R, int64_t k, double* alpha, double* A, int64_t lda) {
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
                loo::k_solve_forward<<<grid, 256, 0, st>>>(h->W.p, N, h->R.p, h->Y.p, ldr, 0, 0, nullptr);
                SL_LAUNCHED("k_solve_forward");
                loo::k_solve_backward<<<grid, 256, 0, st>>>(h->W.p, N, h->Y.p, h->R.p, ldr, 0, 0, nullptr);
                SL_LAUNCHED("k_solve_backward");
            });
            if (alpha)
                timed(h, kD2H, [&] {
                    SL_CHECK(hipMemcpy2DAsync(alpha + c0, sizeof(double) * k, h->R.p, pitch, sizeof(double) * kc, (size_t)n, hipMemcpyDeviceToHost, st));
                });
            else
                SL_CHECK(hipMemcpy2DAsync(A + c0, sizeof(double) * lda, h->R.p, pitch, sizeof(double) * kc, (size_t)n, hipMemcpyDeviceToDevice, st));
        });
    }
}

// -- leave-group-out ---------------------------------------------------------------------------------------------------------
int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// The groups of one launch sequence: caller's groups [first, first + count), their common leading dimension G, and the host image
// of the device record loo::Folds (off, g, gp: count each; then the sorted indices, group after group).
struct Chunk {
    int64_t first = 0, count = 0, G = 0, gmax = 0;
    std::vector<int64_t> meta;
};

// The device memory of one chunk: one arena (as large as the largest chunk needs, which the budget bounds) cut into the per-group
// matrices of the chunk at hand.  panel and Q: N x G per group; P: the scratch T of the inverse after the factorisation; U: V^T
// after it.
struct FoldBuffers {
    DevBuf<int64_t> meta;
    DevBuf<int> info;
    DevBuf<double> arena;
    double *panel = nullptr, *P = nullptr, *U = nullptr, *V = nullptr, *Cf = nullptr, *Q = nullptr, *Ag = nullptr, *Z = nullptr, *partial = nullptr,
           *qpart = nullptr, *vg = nullptr, *logs = nullptr, *corr = nullptr;
    static int64_t doubles(int64_t count, int64_t N, int64_t G, int64_t ldr, bool gram_only) {
        const int64_t nb = G / loo::kBlock, nbr = N / loo::kBlock;
        return gram_only ? count * (N * G + G * G) : count * (2 * N * G + 4 * G * G + 2 * G * ldr + nb * G + nbr * G + G + nb + 2);
    }
    void carve(int64_t count, int64_t N, int64_t G, int64_t ldr, bool gram_only) {
        const int64_t nb = G / loo::kBlock, nbr = N / loo::kBlock;
        panel = arena.p;
        P = panel + count * N * G;
        if (gram_only) return;
        U = P + count * G * G;
        V = U + count * G * G;
        Cf = V + count * G * G;
        Q = Cf + count * G * G;
        Ag = Q + count * N * G;
        Z = Ag + count * G * ldr;
        partial = Z + count * G * ldr;
        qpart = partial + count * nb * G;
        vg = qpart + count * nbr * G;
        logs = vg + count * G;
        corr = logs + count * nb;
    }
};

Chunk make_chunk(int64_t first, int64_t count, const int64_t* ptr, const int64_t* sorted) {
    Chunk c;
    c.first = first;
    c.count = count;
    c.meta.resize((size_t)(3 * count));
    int64_t off = 0;
    for (int64_t q = 0; q < count; ++q) {
        const int64_t g = ptr[first + q + 1] - ptr[first + q];
        c.meta[(size_t)q] = off;
        c.meta[(size_t)(count + q)] = g;
        c.meta[(size_t)(2 * count + q)] = round_up(g, loo::kBlock);
        c.gmax = std::max(c.gmax, g);
        off += g;
    }
    c.G = round_up(c.gmax, loo::kBlock);
    c.meta.insert(c.meta.end(), sorted + ptr[first], sorted + ptr[first + count]);
    return c;
}

loo::Folds upload(gsum_loo* h, const Chunk& c, FoldBuffers& b) {
    b.meta.reserve(c.meta.size());
    SL_CHECK(hipMemcpyAsync(b.meta.p, c.meta.data(), sizeof(int64_t) * c.meta.size(), hipMemcpyHostToDevice, h->stream));
    return loo::Folds{b.meta.p, b.meta.p + c.count, b.meta.p + 2 * c.count, b.meta.p + 3 * c.count};
}

// P[z] = W[:, G_z]^T W[:, G_z] for the chunk's groups, upper block triangle, with the identity tail.
void gather_and_gram(gsum_loo* h, const Chunk& c, const loo::Folds& f, FoldBuffers& b) {
    const int64_t N = h->N, G = c.G, tn = G / loo::kTile;
    hipStream_t st = h->stream;
    timed(h, kFGather, [&] {
        loo::k_gather_columns<<<dim3((unsigned)N, (unsigned)c.count), 256, 0, st>>>(h->W.p, N, f, b.panel, G);
        SL_LAUNCHED("k_gather_columns");
    });
    timed(h, kFGram, [&] {
        loo::k_gram<<<dim3((unsigned)(tn * tn), (unsigned)c.count), 256, 0, st>>>(b.panel, N, f, b.P, G);
        SL_LAUNCHED("k_gram");
        loo::k_identity_tail<<<(unsigned)c.count, loo::kBlock, 0, st>>>(f, b.P, G);
        SL_LAUNCHED("k_identity_tail");
    });
}

// C = chol(P) for the chunk's groups and V = C^-1; info and logs take k_invert_diag's report per block.  Then the first-order
// correction of the log-determinant, corr = tr(V P V^T) - g from the panel itself (Q = panel V^T): the factor of the rounded Gram
// carries an error of the order of cond(P) roundings in its log-determinant, the correction one of the order of cond(P)^(1/2).
void factor_and_invert(gsum_loo* h, const Chunk& c, const loo::Folds& f, FoldBuffers& b) {
    const int64_t G = c.G, nb = G / loo::kBlock;
    hipStream_t st = h->stream;
    double* Cf = b.Cf;
    timed(h, kFFactor, [&] {
        SL_CHECK(hipMemsetAsync(b.info.p, 0, sizeof(int) * c.count * nb, st));                             // blocks past a group's own order
        SL_CHECK(hipMemsetAsync(b.logs, 0, sizeof(double) * c.count * nb, st));
        for (int64_t s = 0; s < nb; ++s) {
            loo::k_chol_diag<<<(unsigned)c.count, loo::kBlock, loo::kCholLds, st>>>(b.P, Cf, G, f, s);
            SL_LAUNCHED("k_chol_diag");
            loo::k_invert_diag<<<dim3(1, (unsigned)c.count), loo::kBlock, loo::kInvertLds, st>>>(Cf, b.V, G, G, b.info.p, b.logs, G * G, f.gp, s, nb);
            SL_LAUNCHED("k_invert_diag");
            const int64_t tn = (G - (s + 1) * loo::kBlock) / loo::kTile;
            if (!tn) break;
            loo::k_chol_panel<<<dim3((unsigned)(2 * tn), (unsigned)c.count), 256, 0, st>>>(b.V, b.P, b.U, G, f, s);
            SL_LAUNCHED("k_chol_panel");
            loo::k_chol_trailing<<<dim3((unsigned)(tn * tn), (unsigned)c.count), 256, 0, st>>>(b.U, b.P, G, f, s);
            SL_LAUNCHED("k_chol_trailing");
        }
        if (nb > 1) {
            const int64_t tn = G / loo::kTile;
            loo::k_transpose_blocks<true><<<dim3((unsigned)(tn * tn), (unsigned)c.count), 256, 0, st>>>(b.U, Cf, G, f);
            SL_LAUNCHED("k_transpose_blocks");
        }
    });
    timed(h, kFInverse, [&] { merge_levels(st, Cf, b.V, b.P, G, c.count, f.gp); });
    timed(h, kFLogdet, [&] {
        const int64_t N = h->N, tn = G / loo::kTile;
        loo::k_transpose_blocks<false><<<dim3((unsigned)(tn * tn), (unsigned)c.count), 256, 0, st>>>(b.V, b.U, G, f);
        SL_LAUNCHED("k_transpose_blocks");
        loo::k_q_product<<<dim3((unsigned)(N / loo::kTile), (unsigned)tn, (unsigned)c.count), 256, 0, st>>>(b.panel, b.U, b.Q, N, G, f);
        SL_LAUNCHED("k_q_product");
        loo::k_qnorm_partial<<<dim3((unsigned)nb, (unsigned)(N / loo::kBlock), (unsigned)c.count), loo::kBlock, 0, st>>>(b.Q, N, G, f, b.qpart);
        SL_LAUNCHED("k_qnorm_partial");
        loo::k_qnorm_total<<<(unsigned)c.count, loo::kBlock, 0, st>>>(b.qpart, N, G, f, b.corr);
        SL_LAUNCHED("k_qnorm_total");
    });
}

void check_indices(const char* who, const int64_t* idx, int64_t count, int64_t n, std::vector<char>& seen) {
    for (int64_t q = 0; q < count; ++q) {
        if (idx[q] < 0 || idx[q] >= n) throw Error(std::string(who) + ": index " + std::to_string(idx[q]) + " is outside 0 ... " + std::to_string(n - 1));
        if (seen[(size_t)idx[q]]) throw Error(std::string(who) + ": index " + std::to_string(idx[q]) + " appears more than once");
        seen[(size_t)idx[q]] = 1;
    }
}

int64_t free_bytes() {
    size_t free_b = 0, total_b = 0;
    SL_CHECK(hipMemGetInfo(&free_b, &total_b));
    return (int64_t)free_b - ((int64_t)64 << 20);
}

void allow_lds() {
    SL_CHECK(hipFuncSetAttribute((const void*)loo::k_invert_diag, hipFuncAttributeMaxDynamicSharedMemorySize, (int)loo::kInvertLds));
    SL_CHECK(hipFuncSetAttribute((const void*)loo::k_chol_diag, hipFuncAttributeMaxDynamicSharedMemorySize, (int)loo::kCholLds));
}

}  // namespace

GL_API int gsum_loo_solve(gsum_loo* h, const double* R, int64_t k, double* alpha) {
    return guarded([&] {
        if (!h || !R || !alpha) throw Error("gsum_loo_solve: null pointer argument");
        if (k < 1) throw Error("gsum_loo_solve: k must be >= 1, got " + std::to_string(k));
        solve_columns(h, R, k, alpha, nullptr, 0);
    });
}

GL_API int gsum_loo_precision_block(gsum_loo* h, const int64_t* idx, int64_t g, double* P) {
    return guarded([&] {
        if (g < 1) throw Error("gsum_loo_precision_block: g must be >= 1, got " + std::to_string(g));
        if (!h || !idx || !P) throw Error("gsum_loo_precision_block: null pointer argument");
        const int64_t n = h->n, N = h->N;
        if (g > n) throw Error("gsum_loo_precision_block: g must be <= n = " + std::to_string(n) + ", got " + std::to_string(g));
        std::vector<char> seen((size_t)n, 0);
        check_indices("gsum_loo_precision_block", idx, g, n, seen);
        std::vector<int64_t> order((size_t)g), sorted((size_t)g);
        for (int64_t q = 0; q < g; ++q) order[(size_t)q] = q;
        std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return idx[a] < idx[b]; });
        for (int64_t q = 0; q < g; ++q) sorted[(size_t)q] = idx[order[(size_t)q]];
        const int64_t ptr[2] = {0, g};
        const Chunk c = make_chunk(0, 1, ptr, sorted.data());
        const int64_t G = c.G, need = (N * G + G * G) * (int64_t)sizeof(double);
        SL_CHECK(hipSetDevice(h->device));
        const int64_t have = free_bytes();
        if (need > have)
            throw Error("gsum_loo_precision_block: a group of " + std::to_string(g) + " points needs " + std::to_string(need >> 20) +
                        " MiB of device memory, " + std::to_string(std::max<int64_t>(have, 0) >> 20) + " MiB are free");
        FoldBuffers b;
        b.arena.alloc((size_t)FoldBuffers::doubles(1, N, G, 0, true));
        b.carve(1, N, G, 0, true);
        std::vector<double> up((size_t)(g * g));
        run(h, [&] {
            const loo::Folds f = upload(h, c, b);
            gather_and_gram(h, c, f, b);
            timed(h, kFScatter, [&] {
                SL_CHECK(hipMemcpy2DAsync(up.data(), sizeof(double) * g, b.P, sizeof(double) * G, sizeof(double) * g, (size_t)g, hipMemcpyDeviceToHost, h->stream));
            });
        });
        // the device wrote the tiles on and above the diagonal tiles; every entry comes from the sorted pair's upper position
        for (int64_t a = 0; a < g; ++a)
            for (int64_t q = a; q < g; ++q) {
                const double v = up[(size_t)(a * g + q)];
                P[order[(size_t)a] * g + order[(size_t)q]] = v;
                P[order[(size_t)q] * g + order[(size_t)a]] = v;
            }
    });
}

GL_API int gsum_loo_fold_budget(gsum_loo* h, int64_t bytes) {
    return guarded([&] {
        if (!h) throw Error("gsum_loo_fold_budget: null pointer argument");
        if (bytes < 0) throw Error("gsum_loo_fold_budget: bytes must be >= 0, got " + std::to_string(bytes));
        h->fold_budget = bytes;
    });
}

GL_API int gsum_loo_folds(gsum_loo* h, const int64_t* fold_ptr, const int64_t* fold_idx, int64_t n_folds, const double* R, int64_t k, double* resid,
                          double* var, double* md2, double* logdet) {
    return guarded([&] {
        if (n_folds < 1) throw Error("gsum_loo_folds: n_folds must be >= 1, got " + std::to_string(n_folds));
        if (k < 1) throw Error("gsum_loo_folds: k must be >= 1, got " + std::to_string(k));
        if (!h || !fold_ptr || !fold_idx || !R || !resid || !var || !md2 || !logdet) throw Error("gsum_loo_folds: null pointer argument");
        const int64_t n = h->n, N = h->N;
        if (n_folds > n) throw Error("gsum_loo_folds: n_folds must be <= n = " + std::to_string(n) + ", got " + std::to_string(n_folds));
        if (fold_ptr[0] != 0 || fold_ptr[n_folds] != n)
            throw Error("gsum_loo_folds: fold_ptr must start at 0 and end at n = " + std::to_string(n));
        for (int64_t q = 0; q < n_folds; ++q)
            if (fold_ptr[q + 1] <= fold_ptr[q] || fold_ptr[q + 1] > n)
                throw Error("gsum_loo_folds: fold_ptr must increase strictly (group " + std::to_string(q) + " is empty or out of range)");
        std::vector<char> seen((size_t)n, 0);
        check_indices("gsum_loo_folds", fold_idx, n, n, seen);
        std::vector<int64_t> sorted(fold_idx, fold_idx + n);
        for (int64_t q = 0; q < n_folds; ++q) std::sort(sorted.begin() + fold_ptr[q], sorted.begin() + fold_ptr[q + 1]);

        // the chunks: groups in the caller's order, as many as the budget holds at their common leading dimension
        const int64_t ldr = round_up(k, loo::kTile);
        const auto bytes_of = [&](int64_t count, int64_t G) {      // the arena, and the small records beside it (meta, info)
            return (FoldBuffers::doubles(count, N, G, ldr, false) + count * (G + G / loo::kBlock + 3)) * (int64_t)sizeof(double);
        };
        SL_CHECK(hipSetDevice(h->device));
        const int64_t shared = (2 * N * ldr + N + n_folds * ldr + 2 * N * std::min(ldr, kChunk)) * (int64_t)sizeof(double);
        const int64_t budget = h->fold_budget ? h->fold_budget : free_bytes() - shared;
        std::vector<Chunk> chunks;
        for (int64_t first = 0; first < n_folds;) {
            int64_t count = 0, gmax = 0;
            while (first + count < n_folds && count < kMaxGroups) {
                const int64_t g = std::max(gmax, fold_ptr[first + count + 1] - fold_ptr[first + count]);
                if (bytes_of(count + 1, round_up(g, loo::kBlock)) > budget) break;
                gmax = g;
                ++count;
            }
            if (!count) {
                const int64_t g = fold_ptr[first + 1] - fold_ptr[first];
                throw Error("gsum_loo_folds: group " + std::to_string(first) + " of " + std::to_string(g) + " points needs " +
                            std::to_string(bytes_of(1, round_up(g, loo::kBlock)) >> 20) + " MiB of device memory, " +
                            std::to_string(std::max<int64_t>(budget, 0) >> 20) + " MiB are there for a chunk of groups");
            }
            chunks.push_back(make_chunk(first, count, fold_ptr, sorted.data()));
            first += count;
        }

        int64_t amax = 0, bmax = 0, mmax = 0;
        for (const Chunk& c : chunks) {
            amax = std::max(amax, FoldBuffers::doubles(c.count, N, c.G, ldr, false));
            bmax = std::max(bmax, c.count * (c.G / loo::kBlock));
            mmax = std::max(mmax, (int64_t)c.meta.size());
        }
        FoldBuffers b;
        DevBuf<double> A, E, vout, md;
        A.alloc((size_t)(N * ldr));
        E.alloc((size_t)(n * ldr));
        vout.alloc((size_t)n);
        md.alloc((size_t)(n_folds * ldr));
        b.meta.alloc((size_t)mmax);
        b.info.alloc((size_t)bmax);
        b.arena.alloc((size_t)amax);
        allow_lds();
        hipStream_t st = h->stream;

        run(h, [&] { SL_CHECK(hipMemsetAsync(A.p, 0, sizeof(double) * N * ldr, st)); });                    // the padding columns
        solve_columns(h, R, k, nullptr, A.p, ldr);

        std::vector<double> logdet_h((size_t)n_folds);
        std::vector<int> bad;
        std::vector<double> logs, corr;
        for (const Chunk& c : chunks) {
            const int64_t G = c.G, nb = G / loo::kBlock;
            bad.assign((size_t)(c.count * nb), 0);
            logs.assign((size_t)(c.count * nb), 0.0);
            corr.assign((size_t)c.count, 0.0);
            b.carve(c.count, N, G, ldr, false);
            run(h, [&] {
                const loo::Folds f = upload(h, c, b);
                timed(h, kFGather, [&] {
                    loo::k_gather_rows<<<dim3((unsigned)G, (unsigned)c.count), 64, 0, st>>>(A.p, ldr, f, b.Ag, G);
                    SL_LAUNCHED("k_gather_rows");
                });
                gather_and_gram(h, c, f, b);
                factor_and_invert(h, c, f, b);
                SL_CHECK(hipMemcpyAsync(bad.data(), b.info.p, sizeof(int) * c.count * nb, hipMemcpyDeviceToHost, st));
                SL_CHECK(hipMemcpyAsync(logs.data(), b.logs, sizeof(double) * c.count * nb, hipMemcpyDeviceToHost, st));
                SL_CHECK(hipMemcpyAsync(corr.data(), b.corr, sizeof(double) * c.count, hipMemcpyDeviceToHost, st));
                timed(h, kFApply, [&] {
                    const dim3 grid((unsigned)(G / loo::kTile), (unsigned)(ldr / loo::kTile), (unsigned)c.count);
                    loo::k_solve_forward<<<grid, 256, 0, st>>>(b.V, G, b.Ag, b.Z, ldr, G * G, G * ldr, f.gp);
                    SL_LAUNCHED("k_solve_forward");
                    loo::k_solve_backward<<<grid, 256, 0, st>>>(b.V, G, b.Z, b.Ag, ldr, G * G, G * ldr, f.gp);
                    SL_LAUNCHED("k_solve_backward");
                    loo::k_md2<<<dim3((unsigned)(ldr / loo::kTile), (unsigned)c.count), 256, 0, st>>>(b.Z, ldr, f, G, md.p + c.first * ldr);
                    SL_LAUNCHED("k_md2");
                    loo::k_colsq_partial<<<dim3((unsigned)nb, (unsigned)nb, (unsigned)c.count), loo::kBlock, 0, st>>>(b.V, G, b.partial, G * G, nb * G, f.gp);
                    SL_LAUNCHED("k_colsq_partial");
                    loo::k_colsq_total<<<dim3((unsigned)nb, (unsigned)c.count), loo::kBlock, 0, st>>>(b.partial, G, b.vg, nb * G, f.gp);
                    SL_LAUNCHED("k_colsq_total");
                });
                timed(h, kFScatter, [&] {
                    loo::k_scatter<<<dim3((unsigned)c.gmax, (unsigned)c.count), 64, 0, st>>>(b.Ag, b.vg, ldr, f, G, E.p, vout.p);
                    SL_LAUNCHED("k_scatter");
                });
            });
            for (int64_t q = 0; q < c.count; ++q) {
                double s = 0;
                for (int64_t blk = 0; blk < nb; ++blk) {
                    if (bad[(size_t)(q * nb + blk)])
                        throw Error("gsum_loo_folds: group " + std::to_string(c.first + q) + " does not factor: the pivot of its row " +
                                    std::to_string(blk * loo::kBlock + bad[(size_t)(q * nb + blk)] - 1) + " (indices ascending) is not a finite positive number");
                    s += logs[(size_t)(q * nb + blk)];
                }
                logdet_h[(size_t)(c.first + q)] = -(2.0 * s + corr[(size_t)q]);       // log det P = 2 sum log C_ii + (tr(V P V^T) - g) to first order
            }
        }
        std::vector<double> resid_h((size_t)(n * k)), var_h((size_t)n), md_h((size_t)(n_folds * k));
        run(h, [&] {
            timed(h, kFScatter, [&] {
                SL_CHECK(hipMemcpy2DAsync(resid_h.data(), sizeof(double) * k, E.p, sizeof(double) * ldr, sizeof(double) * k, (size_t)n, hipMemcpyDeviceToHost, st));
                SL_CHECK(hipMemcpy2DAsync(md_h.data(), sizeof(double) * k, md.p, sizeof(double) * ldr, sizeof(double) * k, (size_t)n_folds, hipMemcpyDeviceToHost, st));
                SL_CHECK(hipMemcpyAsync(var_h.data(), vout.p, sizeof(double) * n, hipMemcpyDeviceToHost, st));
            });
        });
        std::copy(resid_h.begin(), resid_h.end(), resid);
        std::copy(var_h.begin(), var_h.end(), var);
        std::copy(md_h.begin(), md_h.end(), md2);
        std::copy(logdet_h.begin(), logdet_h.end(), logdet);
    });
}

GL_API int gsum_loo_fold_times(gsum_loo* h, double* ms, int32_t reset) {
    return guarded([&] {
        if (!h || !ms) throw Error("gsum_loo_fold_times: null pointer argument");
        read_times(h, kPhases, kFoldPhases, ms, reset);
    });
}

GL_API int gsum_loo_times(gsum_loo* h, double* ms, int32_t reset) {
    return guarded([&] {
        if (!h || !ms) throw Error("gsum_loo_times: null pointer argument");
        read_times(h, 0, kPhases, ms, reset);
    });
}

GL_API void gsum_loo_free(gsum_loo* h) { destroy(h); }
