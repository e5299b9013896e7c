// Kernels of libgsum_loo.so (gfx950 only): the inverse W of a lower Cholesky factor L by blocked recursive doubling, the column
// sums of squares of W, and the two triangular products of alpha = W^T (W R); and for the leave-group-out
// predictions (section 17) the gathered block Gram P_GG = W[:, G]^T W[:, G] and the blocked Cholesky factorisation of a batch of
// such blocks.
//
// The matrices are N x N row-major with N a multiple of kBlock (the caller pads with an identity tail), so no tile has a ragged
// edge and no load is clamped.  Every sum has one fixed order: nothing here uses an atomic, a flag or a wait.
//
// The kernels of the inverse, the column sums and the two products also run on a batch of matrices: matrix z of the batch starts
// `bstride` elements after matrix z - 1, all have the leading dimension `ld`, and sizes[z] (a multiple of kBlock, at most ld) is
// the order of matrix z; workgroups past it leave, so that matrix z is computed exactly as it would be alone.  sizes == nullptr is
// the single matrix of order N.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace loo {

typedef double d2 __attribute__((ext_vector_type(2)));
typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int kBlock = 128;                        // the diagonal block of level 0 and the unit of padding
constexpr int kPanel = 8;                          // rows of L staged per step of k_invert_diag
constexpr int kTile = 64;                          // the product tile: 64 x 64, four waves of 32 x 32
constexpr int kKC = 16;                            // the depth of one staged operand chunk
constexpr int kStrA = kKC + 1;                     // LDS row stride of a row-major A chunk (gemm_nt.hip.h: conflict-free fragment reads)
constexpr int kStrB = kTile + 16;                  // LDS row stride of a k-major chunk: lanes 16..31 land 32 banks after lanes 0..15
constexpr int kPacked = kBlock * (kBlock + 1) / 2; // the lower triangle of a diagonal block, packed by rows
constexpr size_t kInvertLds = sizeof(double) * (kPacked + kPanel * kBlock + kBlock);

// The products are sums of MFMA terms and every other sum is written as separate multiplies and adds, so that the result of a
// sum depends on its order alone.
#pragma clang fp contract(off)

__device__ __forceinline__ int64_t order_of(const int64_t* __restrict__ sizes, int64_t z, int64_t N) { return sizes ? sizes[z] : N; }

// The uploaded factor made a clean lower-triangular N x N matrix where the kernels below read it: zeros above the diagonal inside
// every diagonal block (the caller's upper triangle is ignored; blocks above the diagonal are never read) and ones on the diagonal
// of the identity tail.  One workgroup of kBlock threads per diagonal block, thread j on column j.
__global__ __launch_bounds__(kBlock) void k_clean_factor(double* __restrict__ L, int64_t N, int64_t n) {
    const int j = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * kBlock;
    double* Lb = L + r0 * N + r0;
    for (int i = 0; i < j; ++i) Lb[(int64_t)i * N + j] = 0.0;
    if (r0 + j >= n) Lb[(int64_t)j * N + j] = 1.0;
}

// Level 0: W_bb = L_bb^-1 for the diagonal blocks b = b0 + blockIdx.x of matrix blockIdx.y, one workgroup of kBlock threads each.
// Thread j owns column j of the block: forward substitution down the rows, with the finished part of the column in LDS (packed
// lower triangle, w(i, j) at i (i + 1) / 2 + j: neighbouring threads on neighbouring banks) and kPanel rows of L staged at a
// time.  A thread reads back only what it wrote itself; the barriers are for the staged rows.  Rows and columns >= n are the
// identity tail and are never read from L.
// info[z * nbs + b] = 1 + the first row of the block whose diagonal entry is not a finite positive number (0: none);
// logdiag[z * nbs + b] = sum of log L_ii over the block's rows < n, in row order.  In a batch n is the matrix's own order.
__global__ __launch_bounds__(kBlock) void k_invert_diag(const double* __restrict__ L, double* __restrict__ W, int64_t N, int64_t n,
                                                        int* __restrict__ info, double* __restrict__ logdiag, int64_t bstride,
                                                        const int64_t* __restrict__ sizes, int64_t b0, int64_t nbs) {
    extern __shared__ double lds[];
    double* w = lds;                               // kPacked
    double* rows = lds + kPacked;                  // kPanel x kBlock
    double* dg = rows + kPanel * kBlock;           // kBlock: the diagonal of L
    const int j = threadIdx.x;
    const int64_t z = blockIdx.y, b = b0 + blockIdx.x, r0 = b * kBlock;
    if (sizes) n = sizes[z];
    if (sizes && r0 >= n) return;
    const double* Lb = L + z * bstride + r0 * N + r0;
    double* Wb = W + z * bstride + r0 * N + r0;

    dg[j] = r0 + j < n ? Lb[(int64_t)j * N + j] : 1.0;
    __syncthreads();
    if (j == 0) {
        int bad = 0;
        double s = 0.0;
        for (int i = 0; i < kBlock; ++i) {
            const double d = dg[i];
            if (!bad && !(d > 0.0 && d <= 1.7976931348623157e308)) bad = i + 1;
            s += log(d);
        }
        info[z * nbs + b] = bad;
        logdiag[z * nbs + b] = s;
    }
    for (int i0 = 0; i0 < kBlock; i0 += kPanel) {
        __syncthreads();                           // the previous panel is consumed
        for (int r = 0; r < kPanel; ++r) {
            const int i = i0 + r;
            rows[r * kBlock + j] = (j <= i && r0 + i < n) ? Lb[(int64_t)i * N + j] : (j == i ? 1.0 : 0.0);
        }
        __syncthreads();
        // s_i = [i == j] - sum_{j <= k < i} l_ik w_kj in ascending k for the panel's rows: the terms above the panel are kPanel
        // independent chains over one read of the column, the terms inside it use the entries just found, from registers
        double s[kPanel], own[kPanel];
#pragma unroll
        for (int r = 0; r < kPanel; ++r) s[r] = j == i0 + r ? 1.0 : 0.0;
        for (int k = j; k < i0; ++k) {
            const double wk = w[k * (k + 1) / 2 + j];
#pragma unroll
            for (int r = 0; r < kPanel; ++r) s[r] -= rows[r * kBlock + k] * wk;
        }
#pragma unroll
        for (int r = 0; r < kPanel; ++r) {
            const int i = i0 + r;
            own[r] = 0.0;
            if (j <= i) {
                const double* lr = rows + r * kBlock;
#pragma unroll
                for (int q = 0; q < r; ++q)
                    if (i0 + q >= j) s[r] -= lr[i0 + q] * own[q];
                own[r] = s[r] / lr[i];
                w[i * (i + 1) / 2 + j] = own[r];
            }
            Wb[(int64_t)i * N + j] = own[r];       // the whole block, zeros above the diagonal included
        }
    }
}

// One 64 x 64 tile of C (+)= sign * op(A) * B over k in [kbeg, kend) (multiples of kKC), on v_mfma_f64_16x16x4_f64; with ACC the
// accumulators start as C.  B is k-major (row-major K x N); op(A) is A (row-major M x K) or, with TA, A^T of a row-major K x M
// matrix.  Operands go global -> registers -> LDS in chunks of kKC, two LDS stages, one barrier per chunk, the next chunk's loads
// in flight during the MFMAs (the staging of gemm_nt.hip.h).  A, B and C point at the tile's first row / column; sign is +1 or -1
// and rides on the staged A operand.
template <bool TA, bool ACC>
__device__ __forceinline__ void product_tile(double* __restrict__ C, int64_t ldc, const double* __restrict__ A, int64_t lda,
                                             const double* __restrict__ B, int64_t ldb, int64_t kbeg, int64_t kend, double sign) {
    constexpr int kStageA = TA ? kKC * kStrB : kTile * kStrA;
    constexpr int kStage = kStageA + kKC * kStrB;
    __shared__ __attribute__((aligned(16))) double lds[2 * kStage];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int wm = wv & 1, wn = wv >> 1;
    const int fr = lane & 15, fq = lane >> 4;
    d4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
            for (int x = 0; x < 4; ++x)
                acc[i][jj][x] = ACC ? C[(int64_t)(wm * 32 + i * 16 + fq + 4 * x) * ldc + wn * 32 + jj * 16 + fr] : 0.0;

    d2 ra[2], rb[2];                               // 512 pairs of doubles per operand chunk, two per thread
    auto gload = [&](int64_t k0) {
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int vv = t + it * 256;
            if (TA)
                ra[it] = *reinterpret_cast<const d2*>(A + (k0 + (vv >> 5)) * lda + 2 * (vv & 31));
            else
                ra[it] = *reinterpret_cast<const d2*>(A + (int64_t)(vv >> 3) * lda + k0 + 2 * (vv & 7));
            rb[it] = *reinterpret_cast<const d2*>(B + (k0 + (vv >> 5)) * ldb + 2 * (vv & 31));
        }
    };
    auto swrite = [&](int stage) {
        double* sA = lds + stage * kStage;
        double* sB = sA + kStageA;
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int vv = t + it * 256;
            if (TA) {
                *reinterpret_cast<d2*>(sA + (vv >> 5) * kStrB + 2 * (vv & 31)) = ra[it] * sign;
            } else {                               // rows are only 8-B aligned at an odd stride: two 8-byte stores
                double* q = sA + (vv >> 3) * kStrA + 2 * (vv & 7);
                q[0] = ra[it][0] * sign;
                q[1] = ra[it][1] * sign;
            }
            *reinterpret_cast<d2*>(sB + (vv >> 5) * kStrB + 2 * (vv & 31)) = rb[it];
        }
    };
    auto multiply = [&](int stage) {
        const double* sA = lds + stage * kStage;
        const double* sB = sA + kStageA + fq * kStrB + wn * 32 + fr;
#pragma unroll
        for (int ks = 0; ks < kKC / 4; ++ks) {
            double af[2], bf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i)
                af[i] = TA ? sA[(ks * 4 + fq) * kStrB + wm * 32 + i * 16 + fr] : sA[(wm * 32 + i * 16 + fr) * kStrA + ks * 4 + fq];
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) bf[jj] = sB[ks * 4 * kStrB + jj * 16];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) acc[i][jj] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i], bf[jj], acc[i][jj], 0, 0, 0);
        }
    };
    const int nk = (int)((kend - kbeg) / kKC);
    gload(kbeg);
    swrite(0);
    __syncthreads();
    for (int c = 0; c < nk; ++c) {
        if (c + 1 < nk) gload(kbeg + (int64_t)(c + 1) * kKC);
        multiply(c & 1);
        if (c + 1 < nk) swrite((c + 1) & 1);
        __syncthreads();
    }
    // accumulator map of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
            for (int x = 0; x < 4; ++x) C[(int64_t)(wm * 32 + i * 16 + fq + 4 * x) * ldc + wn * 32 + jj * 16 + fr] = acc[i][jj][x];
}

// The pair q of the level with groups of g rows: the leading half [c0, c0 + h1) is inverted, and so is the trailing part
// [c0 + h1, c0 + h1 + h2), which is shorter than h1 where the matrix ends inside the group (an odd block count).
struct Pair {
    int64_t c0, h1, h2;
    __device__ Pair(int64_t g, int64_t N) {                      // N: the order of the pair's own matrix
        c0 = (int64_t)blockIdx.y * g;
        h1 = g / 2;
        h2 = N - c0 - h1 < h1 ? N - c0 - h1 : h1;
    }
};

// Level s, all pairs in one launch (blockIdx.y = pair, blockIdx.x = tile of the pair's h2 x h1 block 21); workgroups past the tile
// count of a short last pair leave.  Four steps, one launch each:
//   0  T  = L21 W11       W11 is lower triangular: column tile n0 needs k >= n0 only
//   1  W21 = -W22 T       W22 is lower triangular: row tile m0 needs k < m0 + kTile only
//   2  T += L22 W21       the residual of L W = I in block 21 (T still holds L21 W11); L22 is lower triangular
//   3  W21 -= W22 T       one step of refinement: without it the product form loses a factor of ~cond(L) against substitution
// Steps 2 and 3 update their own output tile in place and read nothing another workgroup of the launch writes.
// blockIdx.z = the matrix of a batch; N is the leading dimension of all three, and the order of the single matrix.
template <int STEP>
__global__ __launch_bounds__(256) void k_merge(const double* __restrict__ L, double* W, double* T, int64_t N, int64_t g, int64_t bstride,
                                               const int64_t* __restrict__ sizes) {
    const Pair p(g, order_of(sizes, blockIdx.z, N));
    if (p.h2 <= 0) return;                         // a smaller matrix of the batch has no such pair
    L += (int64_t)blockIdx.z * bstride;
    W += (int64_t)blockIdx.z * bstride;
    T += (int64_t)blockIdx.z * bstride;
    const int64_t tn = p.h1 / kTile, tiles = (p.h2 / kTile) * tn;
    if ((int64_t)blockIdx.x >= tiles) return;
    const int64_t m0 = (blockIdx.x / tn) * kTile, n0 = (blockIdx.x % tn) * kTile;
    const int64_t r2 = p.c0 + p.h1, r = r2 + m0, c = p.c0 + n0;
    if (STEP == 0) product_tile<false, false>(T + r * N + c, N, L + r * N + p.c0, N, W + p.c0 * N + c, N, n0, p.h1, 1.0);
    if (STEP == 1) product_tile<false, false>(W + r * N + c, N, W + r * N + r2, N, T + r2 * N + c, N, 0, m0 + kTile, -1.0);
    if (STEP == 2) product_tile<false, true>(T + r * N + c, N, L + r * N + r2, N, W + r2 * N + c, N, 0, m0 + kTile, 1.0);
    if (STEP == 3) product_tile<false, true>(W + r * N + c, N, W + r * N + r2, N, T + r2 * N + c, N, 0, m0 + kTile, -1.0);
}

// Y = W R (R, Y: N x ldr row-major, ldr a multiple of kTile; blockIdx.x = row tile, blockIdx.y = column tile, blockIdx.z = the
// matrix of a batch, whose R and Y start rstride elements after the one before; N is the leading dimension of W).
__global__ __launch_bounds__(256) void k_solve_forward(const double* __restrict__ W, int64_t N, const double* __restrict__ R, double* __restrict__ Y,
                                                       int64_t ldr, int64_t bstride, int64_t rstride, const int64_t* __restrict__ sizes) {
    const int64_t m0 = (int64_t)blockIdx.x * kTile, n0 = (int64_t)blockIdx.y * kTile;
    if (m0 >= order_of(sizes, blockIdx.z, N)) return;
    W += (int64_t)blockIdx.z * bstride;
    R += (int64_t)blockIdx.z * rstride;
    Y += (int64_t)blockIdx.z * rstride;
    product_tile<false, false>(Y + m0 * ldr + n0, ldr, W + m0 * N, N, R + n0, ldr, 0, m0 + kTile, 1.0);
}

// alpha = W^T Y: row tile m0 of W^T is column tile m0 of W, which is zero above row m0.
__global__ __launch_bounds__(256) void k_solve_backward(const double* __restrict__ W, int64_t N, const double* __restrict__ Y,
                                                        double* __restrict__ alpha, int64_t ldr, int64_t bstride, int64_t rstride,
                                                        const int64_t* __restrict__ sizes) {
    const int64_t m0 = (int64_t)blockIdx.x * kTile, n0 = (int64_t)blockIdx.y * kTile, rows = order_of(sizes, blockIdx.z, N);
    if (m0 >= rows) return;
    W += (int64_t)blockIdx.z * bstride;
    Y += (int64_t)blockIdx.z * rstride;
    alpha += (int64_t)blockIdx.z * rstride;
    product_tile<true, false>(alpha + m0 * ldr + n0, ldr, W + m0, N, Y + n0, ldr, m0, rows, 1.0);
}

// partial[rb * N + j] = sum of W_ij^2 over the rows i of block row rb, in row order (blockIdx.x = block column cb of kBlock columns,
// blockIdx.y = rb; block rows above the diagonal hold nothing and are skipped; blockIdx.z = the matrix of a batch, whose partial
// sums start pstride elements after those of the one before).
__global__ __launch_bounds__(kBlock) void k_colsq_partial(const double* __restrict__ W, int64_t N, double* __restrict__ partial, int64_t bstride,
                                                          int64_t pstride, const int64_t* __restrict__ sizes) {
    if (blockIdx.y < blockIdx.x || (int64_t)blockIdx.y * kBlock >= order_of(sizes, blockIdx.z, N)) return;
    W += (int64_t)blockIdx.z * bstride;
    partial += (int64_t)blockIdx.z * pstride;
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x, i0 = (int64_t)blockIdx.y * kBlock;
    double s = 0.0;
    for (int64_t i = i0 > j ? i0 : j; i < i0 + kBlock; ++i) {
        const double v = W[i * N + j];
        s += v * v;
    }
    partial[(int64_t)blockIdx.y * N + j] = s;
}

// p[j] = the partial sums of column j from its diagonal block row down, in that order (blockIdx.y = the matrix of a batch; its
// p starts N elements after that of the one before).
__global__ __launch_bounds__(kBlock) void k_colsq_total(const double* __restrict__ partial, int64_t N, double* __restrict__ p, int64_t pstride,
                                                        const int64_t* __restrict__ sizes) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x, nb = order_of(sizes, blockIdx.y, N) / kBlock;
    if ((int64_t)blockIdx.x >= nb) return;
    partial += (int64_t)blockIdx.y * pstride;
    p += (int64_t)blockIdx.y * N;
    double s = 0.0;
    for (int64_t rb = blockIdx.x; rb < nb; ++rb) s += partial[rb * N + j];
    p[j] = s;
}

// -- leave-group-out ----------------------------------------------------------------------------------
// The groups of one chunk: group z has g[z] ascending indices idx[off[z] ...] into the rows of W and the order gp[z] = g[z] rounded
// up to kBlock.  Every per-group matrix of the chunk has the leading dimension G >= gp[z] (a multiple of kBlock) and G * G
// elements; a group is computed on its own gp[z] x gp[z] corner, with an identity tail from g[z] on, whatever G is.
struct Folds {
    const int64_t* off;
    const int64_t* g;
    const int64_t* gp;
    const int64_t* idx;
};

constexpr size_t kCholLds = sizeof(double) * (kPacked + kBlock);

// panel[z] (N x G): column j < g[z] is column idx[j] of W from its diagonal down (W holds nothing above its diagonal blocks, so what
// lies above the diagonal is written as zero, not read); the other columns are zero.  blockIdx.x = row, blockIdx.y = group.
__global__ __launch_bounds__(256) void k_gather_columns(const double* __restrict__ W, int64_t N, Folds f, double* __restrict__ panel, int64_t G) {
    const int64_t z = blockIdx.y, row = blockIdx.x, g = f.g[z];
    const int64_t* idx = f.idx + f.off[z];
    double* out = panel + (z * N + row) * G;
    for (int64_t j = threadIdx.x; j < G; j += 256) {
        double v = 0.0;
        if (j < g) {
            const int64_t c = idx[j];
            if (c <= row) v = W[row * N + c];
        }
        out[j] = v;
    }
}

// Ag[z] (G x ldr): row j < g[z] is row idx[j] of A (N x ldr); the other rows are zero.  blockIdx.x = row of the group, blockIdx.y = group.
__global__ __launch_bounds__(64) void k_gather_rows(const double* __restrict__ A, int64_t ldr, Folds f, double* __restrict__ Ag, int64_t G) {
    const int64_t z = blockIdx.y, j = blockIdx.x;
    const bool live = j < f.g[z];
    const double* src = A + (live ? f.idx[f.off[z] + j] : 0) * ldr;
    double* out = Ag + (z * G + j) * ldr;
    for (int64_t c = threadIdx.x; c < ldr; c += 64) out[c] = live ? src[c] : 0.0;
}

// The upper block triangle of P[z] = panel[z]^T panel[z] (tiles with n0 >= m0; blockIdx.x = tile, blockIdx.y = group).  Column j of
// the panel is zero above row idx[j] and the indices ascend, so a tile's terms start at the larger of the two tiles' first
// indices, rounded down to kKC; a tile of padding columns alone takes the last chunk, which it multiplies by zeros.
__global__ __launch_bounds__(256) void k_gram(const double* __restrict__ panel, int64_t N, Folds f, double* __restrict__ P, int64_t G) {
    const int64_t z = blockIdx.y, tn = G / kTile;
    const int64_t m0 = (blockIdx.x / tn) * kTile, n0 = (blockIdx.x % tn) * kTile;
    if (n0 < m0 || n0 >= f.gp[z]) return;
    const int64_t g = f.g[z];
    const int64_t* idx = f.idx + f.off[z];
    int64_t kbeg = N - kKC;
    if (n0 < g) kbeg = idx[n0] / kKC * kKC;        // idx[n0] >= idx[m0]
    const double* pz = panel + z * N * G;
    product_tile<true, false>(P + z * G * G + m0 * G + n0, G, pz + m0, G, pz + n0, G, kbeg, N, 1.0);
}

// The identity tail of P[z]: ones on the diagonal from g[z] to gp[z] (k_gram left zeros there).  One workgroup per group.
__global__ __launch_bounds__(kBlock) void k_identity_tail(Folds f, double* __restrict__ P, int64_t G) {
    const int64_t z = blockIdx.x, j = f.g[z] + threadIdx.x;
    if (j < f.gp[z]) P[z * G * G + j * G + j] = 1.0;
}

// Step b of the factorisation P = C C^T: the lower Cholesky factor of the diagonal block b of P[z] (read from its upper triangle),
// written to the same block of Cf[z] with zeros above the diagonal.  One workgroup of kBlock threads per group, thread i on row
// i, the factor in LDS in the packed layout of k_invert_diag.  Left-looking: s_ij = p_ij - sum_{k < j} c_ik c_jk in ascending k, one
// fma per term (one rounding, as in the MFMA products), c_jj = sqrt(s_jj), c_ij = s_ij / c_jj.  The columns go kCholPanel at a
// time: a thread first takes the terms k < j0 off its kCholPanel entries of the panel, which are that many independent chains
// over one read of its own row, and then walks the panel's columns with its own entries in registers; only that walk waits on
// other threads (two barriers per column: the pivot, then the column).  A pivot s_jj that is not a finite positive number leaves
// a c_jj that is none either (NaN, 0 or inf); k_invert_diag, which runs on this block next, reports its row.
constexpr int kCholPanel = 8;
__global__ __launch_bounds__(kBlock) void k_chol_diag(const double* __restrict__ P, double* __restrict__ Cf, int64_t G, Folds f, int64_t b) {
    extern __shared__ double lds[];
    double* c = lds;                               // kPacked
    double* piv = lds + kPacked;                   // kBlock
    const int i = threadIdx.x, ri = i * (i + 1) / 2;
    const int64_t z = blockIdx.x, r0 = b * kBlock;
    if (r0 >= f.gp[z]) return;
    const double* Pb = P + z * G * G + r0 * G + r0;
    double* Cb = Cf + z * G * G + r0 * G + r0;
    for (int j = 0; j <= i; ++j) c[ri + j] = Pb[(int64_t)j * G + i];
    for (int j0 = 0; j0 < kBlock; j0 += kCholPanel) {
        double s[kCholPanel], own[kCholPanel];
        if (i >= j0) {                             // rows j0 ... up to column j0 - 1 are final since the previous panel's last barrier
#pragma unroll
            for (int jj = 0; jj < kCholPanel; ++jj) s[jj] = j0 + jj <= i ? c[ri + j0 + jj] : 0.0;
            for (int k = 0; k < j0; ++k) {
                const double a = -c[ri + k];
#pragma unroll
                for (int jj = 0; jj < kCholPanel; ++jj) s[jj] = fma(a, c[(j0 + jj) * (j0 + jj + 1) / 2 + k], s[jj]);
            }
        }
#pragma unroll
        for (int jj = 0; jj < kCholPanel; ++jj) {
            const int j = j0 + jj;
            if (i >= j) {
                const double* rj = c + j * (j + 1) / 2 + j0;
#pragma unroll
                for (int kk = 0; kk < jj; ++kk) s[jj] = fma(-own[kk], rj[kk], s[jj]);
                if (i == j) piv[j] = sqrt(s[jj]);
            }
            __syncthreads();
            if (i >= j) {
                own[jj] = i == j ? piv[j] : s[jj] / piv[j];
                c[ri + j] = own[jj];
            }
            __syncthreads();                       // row j + 1 is final up to column j
        }
    }
    for (int r = 0; r < kBlock; ++r) Cb[(int64_t)r * G + i] = i <= r ? c[r * (r + 1) / 2 + i] : 0.0;
}

// Step b, the block row of the upper factor right of the diagonal block: U12 = C_bb^-1 P12 (V holds C_bb^-1 in its diagonal block
// b, lower triangular: row tile m0 needs k < m0 + kTile only).  blockIdx.x = (column tile, row tile of the two), blockIdx.y = group.
__global__ __launch_bounds__(256) void k_chol_panel(const double* __restrict__ V, const double* __restrict__ P, double* __restrict__ U, int64_t G,
                                                    Folds f, int64_t b) {
    const int64_t z = blockIdx.y, r0 = b * kBlock, m0 = (blockIdx.x & 1) * kTile, c = r0 + kBlock + (blockIdx.x >> 1) * kTile;
    if (c >= f.gp[z]) return;
    const int64_t base = z * G * G;
    product_tile<false, false>(U + base + (r0 + m0) * G + c, G, V + base + (r0 + m0) * G + r0, G, P + base + r0 * G + c, G, 0, m0 + kTile, 1.0);
}

// Step b, the trailing update P22 -= U12^T U12 on the upper block triangle (tiles with n >= m; blockIdx.x = tile, blockIdx.y = group).
__global__ __launch_bounds__(256) void k_chol_trailing(const double* __restrict__ U, double* __restrict__ P, int64_t G, Folds f, int64_t b) {
    const int64_t z = blockIdx.y, r0 = b * kBlock, r1 = r0 + kBlock, tn = (G - r1) / kTile;
    const int64_t m = r1 + (blockIdx.x / tn) * kTile, n = r1 + (blockIdx.x % tn) * kTile;
    if (n < m || n >= f.gp[z]) return;
    const int64_t base = z * G * G;
    product_tile<true, true>(P + base + m * G + n, G, U + base + r0 * G + m, G, U + base + r0 * G + n, G, 0, kBlock, -1.0);
}

// dst[z] = src[z]^T on a block triangle: with LOWER the blocks below the diagonal blocks (the factor C from U; k_chol_diag wrote
// the diagonal blocks), without it the diagonal blocks and the blocks above them (V^T from the lower triangular V).
// blockIdx.x = 64 x 64 tile of dst, blockIdx.y = group.
template <bool LOWER>
__global__ __launch_bounds__(256) void k_transpose_blocks(const double* __restrict__ src, double* __restrict__ dst, int64_t G, Folds f) {
    __shared__ double tile[kTile][kTile + 1];
    const int64_t z = blockIdx.y, tn = G / kTile;
    const int64_t r = (blockIdx.x / tn) * kTile, c = (blockIdx.x % tn) * kTile;
    if ((LOWER ? r / kBlock <= c / kBlock : r / kBlock > c / kBlock) || r >= f.gp[z] || c >= f.gp[z]) return;
    const int x = threadIdx.x & 63, y0 = threadIdx.x >> 6;
    const int64_t base = z * G * G;
    for (int y = y0; y < kTile; y += 4) tile[y][x] = src[base + (c + y) * G + r + x];
    __syncthreads();
    for (int y = y0; y < kTile; y += 4) dst[base + (r + y) * G + c + x] = tile[x][y];
}

// The correction of the log-determinant, first launch: Q[z] = panel[z] V[z]^T (N x G; VT holds V^T), whose columns would be
// orthonormal if P = C C^T held exactly for the exact Gram P of the panel.  V^T is upper triangular, so column tile n0 needs
// k < n0 + kTile, and row tile m0 of the panel holds nothing in the columns whose index lies below it: k stops at the number of the
// group's indices <= m0 + kTile - 1 (rounded up to kKC).  blockIdx.x = row tile of N, blockIdx.y = column tile, blockIdx.z = group.
__global__ __launch_bounds__(256) void k_q_product(const double* __restrict__ panel, const double* __restrict__ VT, double* __restrict__ Q, int64_t N,
                                                   int64_t G, Folds f) {
    const int64_t z = blockIdx.z, m0 = (int64_t)blockIdx.x * kTile, n0 = (int64_t)blockIdx.y * kTile;
    if (n0 >= f.gp[z]) return;
    const int64_t* idx = f.idx + f.off[z];
    int64_t lo = 0, hi = f.g[z];                   // the count of indices <= m0 + kTile - 1
    while (lo < hi) {
        const int64_t mid = (lo + hi) / 2;
        if (idx[mid] <= m0 + kTile - 1) lo = mid + 1; else hi = mid;
    }
    int64_t kend = (lo + kKC - 1) / kKC * kKC;
    if (kend > n0 + kTile) kend = n0 + kTile;
    product_tile<false, false>(Q + (z * N + m0) * G + n0, G, panel + (z * N + m0) * G, G, VT + z * G * G + n0, G, 0, kend, 1.0);
}

// qpart[z][rb * G + j] = sum of Q_ij^2 over the kBlock rows of block row rb, in row order (blockIdx.x = block of kBlock columns,
// blockIdx.y = rb, blockIdx.z = group).
__global__ __launch_bounds__(kBlock) void k_qnorm_partial(const double* __restrict__ Q, int64_t N, int64_t G, Folds f, double* __restrict__ qpart) {
    const int64_t z = blockIdx.z, j = (int64_t)blockIdx.x * kBlock + threadIdx.x, i0 = (int64_t)blockIdx.y * kBlock;
    if ((int64_t)blockIdx.x * kBlock >= f.gp[z]) return;
    const double* q = Q + (z * N + i0) * G + j;
    double s = 0.0;
    for (int i = 0; i < kBlock; ++i) {
        const double v = q[(int64_t)i * G];
        s += v * v;
    }
    qpart[(z * (N / kBlock) + blockIdx.y) * G + j] = s;
}

// corr[z] = sum over the columns j < g[z] of (|q_j|^2 - 1) = tr(V P V^T) - g, the first-order term of log det P - log det C C^T:
// a column's block rows are added from the top down, thread t takes the columns t, t + kBlock, ... in that order, and the kBlock
// sums are added by a fixed tree.  One workgroup per group.
__global__ __launch_bounds__(kBlock) void k_qnorm_total(const double* __restrict__ qpart, int64_t N, int64_t G, Folds f, double* __restrict__ corr) {
    __shared__ double part[kBlock];
    const int64_t z = blockIdx.x, nbr = N / kBlock, g = f.g[z];
    const double* qp = qpart + z * nbr * G;
    double s = 0.0;
    for (int64_t j = threadIdx.x; j < g; j += kBlock) {
        double c = 0.0;
        for (int64_t rb = 0; rb < nbr; ++rb) c += qp[rb * G + j];
        s += c - 1.0;
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w /= 2) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) corr[z] = part[0];
}

// md2[z * ldr + c] = sum over the rows of Z[z] (G x ldr; rows from g[z] on are zero) of Z_ic^2: four interleaved row sums per
// column in row order, added as (s0 + s1) + (s2 + s3).  blockIdx.x = tile of 64 columns, blockIdx.y = group.
__global__ __launch_bounds__(256) void k_md2(const double* __restrict__ Z, int64_t ldr, Folds f, int64_t G, double* __restrict__ md2) {
    __shared__ double part[4][kTile];
    const int64_t z = blockIdx.y, c = (int64_t)blockIdx.x * kTile + (threadIdx.x & 63), rows = f.gp[z];
    const int q = threadIdx.x >> 6;
    const double* col = Z + z * G * ldr + c;
    double s = 0.0;
    for (int64_t i = q; i < rows; i += 4) {
        const double v = col[i * ldr];
        s += v * v;
    }
    part[q][threadIdx.x & 63] = s;
    __syncthreads();
    if (q == 0) {
        const int x = threadIdx.x;
        md2[z * ldr + c] = (part[0][x] + part[1][x]) + (part[2][x] + part[3][x]);
    }
}

// Back to the caller's rows: resid[idx[j]] = E[z] row j (k of its ldr columns) and var[idx[j]] = vg[z * G + j] for j < g[z].
// blockIdx.x = row of the group, blockIdx.y = group.
__global__ __launch_bounds__(64) void k_scatter(const double* __restrict__ E, const double* __restrict__ vg, int64_t ldr, Folds f, int64_t G,
                                                double* __restrict__ resid, double* __restrict__ var) {
    const int64_t z = blockIdx.y, j = blockIdx.x;
    if (j >= f.g[z]) return;
    const int64_t i = f.idx[f.off[z] + j];
    const double* src = E + (z * G + j) * ldr;
    for (int64_t c = threadIdx.x; c < ldr; c += 64) resid[i * ldr + c] = src[c];
    if (threadIdx.x == 0) var[i] = vg[z * G + j];
}

}  // namespace loo
