// Kernels of libgsum_band.so (gfx950 only): kernel matrices in LAPACK lower band storage, their batched band Cholesky, the forward
// substitution against the stored factor and the Gram matrices of the solved columns.
//
// Band layout, per matrix: AB[k, j] = A[j + k, j], k = 0 .. b, j = 0 .. n - 1, row-major (b + 1) x n: diagonal k is contiguous in j.
// Entries with j + k >= n are never read and are written as zeros.
//
// The kernel entries come from kernels/build.hip.h (the exp restatement, gs_base_value, gs_tree_eval): one definition, not a copy.
//
// ORDER OF EVERY SUM.  An entry (i, c) of the factor is (a_ic - sum_k l_ik l_ck) / l_cc with k ascending over the columns left of c: the
// trailing updates of the earlier block steps first (each one v_mfma_f64_16x16x4_f64 chain over its 16 columns, ascending), then the
// columns of c's own block, ascending.  A solved entry y_i is (z_i - sum_k l_ik y_k) / l_ii with k ascending, one fma per k.  A Gram
// entry is one MFMA chain over the rows 0 .. n in steps of four.  sum log L_jj: 256 partial sums over j = t, t + 256, ..., then a
// binary tree.  Nothing of this depends on the number of matrices, on the chunk, or on which workgroup runs it; a band stored with
// extra all-zero diagonals adds terms 0 * x = 0 to the same chains (fma(0, x, acc) = acc), so its results are the same bits.
#pragma once
#include "kernels/common.hip.h"
#include "kernels/build.hip.h"

namespace gb {

constexpr int kBlock = 16;                 // columns the factorisation advances per step (gsum_band_block)
constexpr int kMaxB = 255;                 // the widest half-bandwidth (gsum_band_max_halfwidth): the rows under a diagonal block fit one
                                           // thread each in a 256-thread workgroup
constexpr int kThreads = 256;
constexpr int kPanelRows = 256;            // kMaxB rounded up to whole 16-row tiles
constexpr int kStr = 17;                   // odd LDS row stride of the 16-column operands

typedef double acc4 __attribute__((ext_vector_type(4)));

// ---- entries ---------------------------------------------------------------------------------------------------------------------------

// K(x_i, x_j), i != j, of the two-argument form (what the dense device build returns for kernel(X, X) off the diagonal): the flattened
// form as k_build2<CROSS> computes it, a tree through gs_tree_eval as k_build_tree<CROSS> does.
__device__ __forceinline__ double off_diagonal(const gsum_kernel_desc& desc, double xi, double xj) {
#pragma clang fp contract(off)
    if (desc.n_ops > 0) return gs_tree_eval(desc, &xi, &xj, 1, false, nullptr, nullptr, true);
    const double ls = desc.length_scale[0];
    const double e = xi / ls - xj / ls;
    return desc.amplitude * gs_base_value(desc.family, e * e) + desc.additive_const;
}

// the one-argument diagonal plus the nugget: amplitude * 1 + white + additive for the flattened form, the tree's walk with every leaf 1
__device__ __forceinline__ double diagonal(const gsum_kernel_desc& desc, double x, double nugget) {
#pragma clang fp contract(off)
    double v;
    if (desc.n_ops > 0) v = gs_tree_eval(desc, &x, &x, 1, true, nullptr, nullptr);
    else v = desc.amplitude * 1.0 + desc.white_noise + desc.additive_const;
    return v + nugget;
}

// flags[i, k - 1] = 1 where some K_i(x_j, x_{j+k}), k = 1 .. kmax, has bits other than +-0 (NaN and Inf count).  The flags are zeroed by
// the caller; every workgroup that sees such an entry stores the same 1.  grid = (column chunks, kmax, matrices).
__global__ __launch_bounds__(kThreads) void k_band_width(const gsum_kernel_desc* descs, const double* X, int n, int kmax, int32_t* flags) {
    const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int k = blockIdx.y + 1;
    const gsum_kernel_desc& desc = descs[blockIdx.z];
    bool nz = false;
    if (j + k < n) {
        const double v = off_diagonal(desc, X[j + k], X[j]);
        nz = ((unsigned long long)__double_as_longlong(v) << 1) != 0ull;
    }
    if (__syncthreads_or(nz) && threadIdx.x == 0) flags[(int64_t)blockIdx.z * kmax + blockIdx.y] = 1;
}

// AB[i, k, j] of the matrices of descs: grid = (column chunks, b + 1, matrices)
__global__ __launch_bounds__(kThreads) void k_band_build(const gsum_kernel_desc* descs, const double* X, int n, int b, double nugget, double* AB) {
    const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= n) return;
    const int k = blockIdx.y;
    const gsum_kernel_desc& desc = descs[blockIdx.z];
    double v = 0.0;
    if (k == 0) v = diagonal(desc, X[j], nugget);
    else if (j + k < n) v = off_diagonal(desc, X[j + k], X[j]);
    AB[((int64_t)blockIdx.z * (b + 1) + k) * n + j] = v;
}

// ---- factorisation ---------------------------------------------------------------------------------------------------------------------

// A = L L^T in place, one workgroup per matrix, kBlock columns per step:
//   1. the 16 x 16 diagonal block in the registers of one wave (lane r holds row r; the column being eliminated travels by shuffles),
//   2. the at most b rows under it, one thread per row: x = a L_dd^-T by substitution, kept in LDS as the panel P,
//   3. the window of the at most b x b entries those rows span: W -= P P^T on v_mfma_f64_16x16x4_f64, 16 x 16 tiles on or below the
//      diagonal dealt to the four waves; the tile is the accumulator, read from and written to the band in global memory (L2-resident
//      at these sizes), the operands come from the panel in LDS.  One code for every b (b = 0: steps 2 and 3 have no rows).
// info[i] = 0, or the 1-based order of the first pivot that is not finite and positive (a NaN fails the test); the factorisation of
// that matrix stops there.
__global__ __launch_bounds__(kThreads) void k_band_factor(double* Lall, int n, int b, int32_t* info) {
    __shared__ double D[kBlock][kStr];
    __shared__ double P[kPanelRows][kStr];
    __shared__ int s_fail;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t ln = n;
    double* L = Lall + (int64_t)blockIdx.x * (b + 1) * ln;
    if (t == 0) s_fail = 0;
    for (int j0 = 0; j0 < n; j0 += kBlock) {
        const int nb = min(kBlock, n - j0);
        __syncthreads();
        if (w == 0) {
            // row `lane` of the block (zeros beyond the block, the band or the matrix)
            double row[kBlock];
#pragma unroll
            for (int c = 0; c < kBlock; ++c)
                row[c] = (lane < nb && c <= lane && lane - c <= b) ? L[(int64_t)(lane - c) * ln + j0 + c] : 0.0;
            int fail = 0;
#pragma unroll
            for (int c = 0; c < kBlock; ++c) {
                if (c < nb && fail == 0) {
                    const double p = __shfl(row[c], c, 64);
                    if (!(p > 0.0 && p < __builtin_inf())) {
                        fail = j0 + c + 1;
                    } else {
                        const double l = sqrt(p);
                        const double x = lane == c ? l : (lane > c ? row[c] / l : 0.0);
                        row[c] = x;
#pragma unroll
                        for (int k = c + 1; k < kBlock; ++k) {
                            const double xk = __shfl(x, k, 64);
                            if (lane >= k) row[k] = __builtin_fma(-x, xk, row[k]);
                        }
                    }
                }
            }
            if (fail == 0) {
#pragma unroll
                for (int c = 0; c < kBlock; ++c) {
                    if (lane < kBlock) D[lane][c] = row[c];
                    if (lane < nb && c <= lane && lane - c <= b) L[(int64_t)(lane - c) * ln + j0 + c] = row[c];
                }
            } else if (lane == 0) {
                s_fail = fail;
            }
        }
        __syncthreads();
        if (s_fail != 0) break;
        const int nr = min(b, n - (j0 + kBlock));          // rows under the block that its columns reach
        if (nr <= 0) continue;
        const int nt = (nr + 15) >> 4;
        if (t < nt * 16) {
            const int i = j0 + kBlock + t;
            double x[kBlock];
#pragma unroll
            for (int c = 0; c < kBlock; ++c) {
                const int d = i - (j0 + c);
                double a = (t < nr && d <= b) ? L[(int64_t)d * ln + j0 + c] : 0.0;
#pragma unroll
                for (int k = 0; k < c; ++k) a = __builtin_fma(-x[k], D[c][k], a);
                x[c] = a / D[c][c];
                P[t][c] = x[c];
                if (t < nr && d <= b) L[(int64_t)d * ln + j0 + c] = x[c];
            }
        }
        __syncthreads();
        const int tiles = nt * (nt + 1) / 2;
        const int fr = lane & 15, fq = lane >> 4;
        for (int idx = w; idx < tiles; idx += kThreads / 64) {
            int ti = (int)((sqrtf(8.f * (float)idx + 1.f) - 1.f) * 0.5f);
            while ((ti + 1) * (ti + 2) / 2 <= idx) ++ti;
            while (ti * (ti + 1) / 2 > idx) --ti;
            const int tj = idx - ti * (ti + 1) / 2;
            const int col = j0 + kBlock + 16 * tj + fr;
            acc4 acc;
            bool ok[4];
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                const int row = j0 + kBlock + 16 * ti + fq + 4 * x;
                ok[x] = row < n && row >= col && row - col <= b;
                acc[x] = ok[x] ? L[(int64_t)(row - col) * ln + col] : 0.0;
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const double af = -P[16 * ti + fr][4 * s + fq];
                const double bf = P[16 * tj + fr][4 * s + fq];
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(af, bf, acc, 0, 0, 0);
            }
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                const int row = j0 + kBlock + 16 * ti + fq + 4 * x;
                if (ok[x]) L[(int64_t)(row - col) * ln + col] = acc[x];
            }
        }
    }
    if (t == 0) info[blockIdx.x] = s_fail;
}

// sld[i] = sum_j log L_jj, NaN where info[i] != 0.  L_jj = f 2^e with f in [sqrt(1/2), sqrt(2)): the exponents are summed as integers
// and the logarithms of the fractions in the fixed order above, so a diagonal of powers of two gives (sum e) ln 2 rounded once.
__global__ __launch_bounds__(kThreads) void k_band_sld(const double* Lall, int n, int b, const int32_t* info, double* sld) {
    __shared__ double sf[kThreads];
    __shared__ long long se[kThreads];
    const int t = threadIdx.x;
    const double* dg = Lall + (int64_t)blockIdx.x * (b + 1) * (int64_t)n;
    double f = 0.0;
    long long e = 0;
    for (int64_t j = t; j < n; j += kThreads) {
        int ex;
        double fr = frexp(dg[j], &ex);                     // [1/2, 1)
        if (fr < 0.70710678118654752440) {
            fr *= 2.0;
            --ex;
        }
        f += log(fr);
        e += ex;
    }
    sf[t] = f;
    se[t] = e;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (t < s) {
            sf[t] = sf[t] + sf[t + s];
            se[t] = se[t] + se[t + s];
        }
        __syncthreads();
    }
    if (t == 0) sld[blockIdx.x] = info[blockIdx.x] != 0 ? __builtin_nan("") : __builtin_fma((double)se[0], 0.69314718055994530942, sf[0]);
}

// ---- forward substitution --------------------------------------------------------------------------------------------------------------

// Y = L^-1 Z for one matrix and 16 columns per workgroup: grid = (column chunks, matrices).  Z is n x ncols column-major (shared by the
// matrices), Y is ncols x n per matrix (the same layout).  Thread t owns row t & 15 of the current 16-row block and column t >> 4 of
// the chunk: it subtracts the products with the b solved rows above the block, ascending, from the block of L staged in LDS and the
// ring of solved rows, then the block's own triangle is solved among the 16 lanes of the column by shuffles.  info != null: a matrix
// with info != 0 is left alone.
// LDS (dynamic, forward_lds_bytes(b)): Lt[16][ls], the block's rows of L by diagonal (Lt[tt][d] = L[i0 + tt, i0 + tt - d]), ls = b + 1
// rounded up to 1 mod 4 (the 16 rows a quarter wave reads fall into 16 banks), and the ring yh[R][16] of the last R = max(b, 16)
// solved rows.
__host__ __device__ constexpr int forward_ls(int b) { return b + 1 + ((5 - ((b + 1) & 3)) & 3); }
__host__ __device__ constexpr int forward_ring(int b) { return b > kBlock ? b : kBlock; }
__host__ __device__ constexpr size_t forward_lds_bytes(int b) { return sizeof(double) * (kBlock * (size_t)forward_ls(b) + (size_t)forward_ring(b) * 16); }
static_assert(forward_ls(kMaxB) % 4 == 1 && forward_ls(0) == 1 && forward_ls(4) == 5 && forward_lds_bytes(kMaxB) <= 65536, "the substitution's LDS");

__global__ __launch_bounds__(kThreads) void k_band_forward(const double* Lall, int n, int b, const double* Z, int ncols, double* Yall,
                                                            const int32_t* info) {
    extern __shared__ double lds[];
    if (info && info[blockIdx.y] != 0) return;
    const int ls = forward_ls(b), R = forward_ring(b);
    double* Lt = lds;
    double* yh = lds + kBlock * ls;
    const int t = threadIdx.x, r = t & 15, c = t >> 4;
    const int64_t ln = n;
    const double* L = Lall + (int64_t)blockIdx.y * (b + 1) * ln;
    double* Y = Yall + (int64_t)blockIdx.y * ncols * ln;
    const int cg = blockIdx.x * 16 + c;
    const bool incol = cg < ncols;
    const int grp = (t & 63) & ~15;
    for (int i0 = 0; i0 < n; i0 += kBlock) {
        for (int idx = t; idx < (b + 1) * kBlock; idx += kThreads) {
            const int d = idx >> 4, tt = idx & 15;
            const int row = i0 + tt, col = row - d;
            Lt[tt * ls + d] = (row < n && col >= 0) ? L[(int64_t)d * ln + col] : 0.0;
        }
        __syncthreads();
        const int i = i0 + r;
        double acc = (incol && i < n) ? Z[(int64_t)cg * ln + i] : 0.0;
        // the solved rows i0 - b .. i0 - 1 that row i reaches: columns col = i0 - b + kk, kk >= r (inside the band) and col >= 0
        const int kk0 = max(r, b - i0);
        if (kk0 < b) {
            int slot = (i0 - b + kk0) % R;
            for (int kk = kk0; kk < b; ++kk) {
                acc = __builtin_fma(-Lt[r * ls + (r + b - kk)], yh[slot * 16 + c], acc);
                slot = slot + 1 == R ? 0 : slot + 1;
            }
        }
        const double lrr = i < n ? Lt[r * ls] : 1.0;
#pragma unroll
        for (int k = 0; k < kBlock; ++k) {
            if (r == k) acc = acc / lrr;
            const double yk = __shfl(acc, grp + k, 64);
            if (r > k && r - k <= b) acc = __builtin_fma(-Lt[r * ls + (r - k)], yk, acc);
        }
        __syncthreads();                                  // every read of the ring and of Lt is done
        yh[(i % R) * 16 + c] = acc;
        if (incol && i < n) Y[(int64_t)cg * ln + i] = acc;
    }
}

// ---- Gram matrices ---------------------------------------------------------------------------------------------------------------------

// G[i, s] = Y_s^T Y_s (cols x cols) on v_mfma_f64_16x16x4_f64, one wave per (set, matrix): lane l holds Y[k0 + (l >> 4), column l & 15
// of the set] as the A and as the B operand, so (a, b) and (b, a) see the same products in the same chain: G is bitwise symmetric.  The
// K loop runs 0 .. n in steps of four, never split.  NaN where info != 0.  grid = (sets, matrices), block = 64.
// Y holds `sets` sets per matrix, which are the sets set0 .. of the sets_total that G has room for.
__global__ __launch_bounds__(64) void k_band_gram(const double* Yall, int n, int cols, int sets, int64_t sets_total, int64_t set0,
                                                   const int32_t* info, double* G) {
    const int lane = threadIdx.x, fr = lane & 15, fq = lane >> 4;
    const int64_t ln = n;
    const double* Y = Yall + ((int64_t)blockIdx.y * sets + blockIdx.x) * cols * ln + (int64_t)fr * ln;
    acc4 acc = {0.0, 0.0, 0.0, 0.0};
    const bool bad = info[blockIdx.y] != 0;
    if (!bad) {
        for (int k0 = 0; k0 < n; k0 += 4) {
            const int k = k0 + fq;
            const double f = (fr < cols && k < n) ? Y[k] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(f, f, acc, 0, 0, 0);
        }
    }
    if (fr >= cols) return;
    double* g = G + ((int64_t)blockIdx.y * sets_total + set0 + blockIdx.x) * cols * cols;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        const int row = fq + 4 * x;
        if (row < cols) g[row * cols + fr] = bad ? __builtin_nan("") : acc[x];
    }
}

}  // namespace gb
