// Kernels of libgsum_loo.so (gfx950 only): the inverse W of a lower Cholesky factor L by blocked recursive doubling, the column
// sums of squares of W, and the two triangular products of alpha = W^T (W R).  DESIGN.md section 15.
//
// The matrices are N x N row-major with N a multiple of kBlock (the caller pads with an identity tail), so no tile has a ragged
// edge and no load is clamped.  Every sum has one fixed order: nothing here uses an atomic, a flag or a wait.
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

// Level 0: W_bb = L_bb^-1 for every diagonal block b, one workgroup of kBlock threads each.  Thread j owns column j of the block:
// forward substitution down the rows, with the finished part of the column in LDS (packed lower triangle, w(i, j) at i (i + 1) / 2
// + j: neighbouring threads on neighbouring banks) and kPanel rows of L staged at a time.  A thread reads back only what it wrote
// itself; the barriers are for the staged rows.  Rows and columns >= n are the identity tail and are never read from L.
// info[b] = 1 + the first row of the block whose diagonal entry is not a finite positive number (0: none);
// logdiag[b] = sum of log L_ii over the block's rows < n, in row order.
__global__ __launch_bounds__(kBlock) void k_invert_diag(const double* __restrict__ L, double* __restrict__ W, int64_t N, int64_t n,
                                                        int* __restrict__ info, double* __restrict__ logdiag) {
    extern __shared__ double lds[];
    double* w = lds;                               // kPacked
    double* rows = lds + kPacked;                  // kPanel x kBlock
    double* dg = rows + kPanel * kBlock;           // kBlock: the diagonal of L
    const int j = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * kBlock;
    const double* Lb = L + r0 * N + r0;
    double* Wb = W + r0 * N + r0;

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
        info[blockIdx.x] = bad;
        logdiag[blockIdx.x] = s;
    }
    for (int i0 = 0; i0 < kBlock; i0 += kPanel) {
        __syncthreads();                           // the previous panel is consumed
        for (int r = 0; r < kPanel; ++r) {
            const int i = i0 + r;
            rows[r * kBlock + j] = (j <= i && r0 + i < n) ? Lb[(int64_t)i * N + j] : (j == i ? 1.0 : 0.0);
        }
        __syncthreads();
        for (int r = 0; r < kPanel; ++r) {
            const int i = i0 + r;
            double v = 0.0;
            if (j <= i) {
                double s = j == i ? 1.0 : 0.0;
                const double* lr = rows + r * kBlock;
                for (int k = j; k < i; ++k) s -= lr[k] * w[k * (k + 1) / 2 + j];
                v = s / lr[i];
                w[i * (i + 1) / 2 + j] = v;
            }
            Wb[(int64_t)i * N + j] = v;            // the whole block, zeros above the diagonal included
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
    __device__ Pair(int64_t g, int64_t N) {
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
template <int STEP>
__global__ __launch_bounds__(256) void k_merge(const double* __restrict__ L, double* W, double* T, int64_t N, int64_t g) {
    const Pair p(g, N);
    const int64_t tn = p.h1 / kTile, tiles = (p.h2 / kTile) * tn;
    if ((int64_t)blockIdx.x >= tiles) return;
    const int64_t m0 = (blockIdx.x / tn) * kTile, n0 = (blockIdx.x % tn) * kTile;
    const int64_t r2 = p.c0 + p.h1, r = r2 + m0, c = p.c0 + n0;
    if (STEP == 0) product_tile<false, false>(T + r * N + c, N, L + r * N + p.c0, N, W + p.c0 * N + c, N, n0, p.h1, 1.0);
    if (STEP == 1) product_tile<false, false>(W + r * N + c, N, W + r * N + r2, N, T + r2 * N + c, N, 0, m0 + kTile, -1.0);
    if (STEP == 2) product_tile<false, true>(T + r * N + c, N, L + r * N + r2, N, W + r2 * N + c, N, 0, m0 + kTile, 1.0);
    if (STEP == 3) product_tile<false, true>(W + r * N + c, N, W + r * N + r2, N, T + r2 * N + c, N, 0, m0 + kTile, -1.0);
}

// Y = W R (R, Y: N x ldr row-major, ldr a multiple of kTile; blockIdx.x = row tile, blockIdx.y = column tile).
__global__ __launch_bounds__(256) void k_solve_forward(const double* __restrict__ W, int64_t N, const double* __restrict__ R, double* __restrict__ Y,
                                                       int64_t ldr) {
    const int64_t m0 = (int64_t)blockIdx.x * kTile, n0 = (int64_t)blockIdx.y * kTile;
    product_tile<false, false>(Y + m0 * ldr + n0, ldr, W + m0 * N, N, R + n0, ldr, 0, m0 + kTile, 1.0);
}

// alpha = W^T Y: row tile m0 of W^T is column tile m0 of W, which is zero above row m0.
__global__ __launch_bounds__(256) void k_solve_backward(const double* __restrict__ W, int64_t N, const double* __restrict__ Y,
                                                        double* __restrict__ alpha, int64_t ldr) {
    const int64_t m0 = (int64_t)blockIdx.x * kTile, n0 = (int64_t)blockIdx.y * kTile;
    product_tile<true, false>(alpha + m0 * ldr + n0, ldr, W + m0, N, Y + n0, ldr, m0, N, 1.0);
}

// partial[rb * N + j] = sum of W_ij^2 over the rows i of block row rb, in row order (blockIdx.x = block column cb of kBlock columns,
// blockIdx.y = rb; block rows above the diagonal hold nothing and are skipped).
__global__ __launch_bounds__(kBlock) void k_colsq_partial(const double* __restrict__ W, int64_t N, double* __restrict__ partial) {
    if (blockIdx.y < blockIdx.x) return;
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x, i0 = (int64_t)blockIdx.y * kBlock;
    double s = 0.0;
    for (int64_t i = i0 > j ? i0 : j; i < i0 + kBlock; ++i) {
        const double v = W[i * N + j];
        s += v * v;
    }
    partial[(int64_t)blockIdx.y * N + j] = s;
}

// p[j] = the partial sums of column j from its diagonal block row down, in that order.
__global__ __launch_bounds__(kBlock) void k_colsq_total(const double* __restrict__ partial, int64_t N, double* __restrict__ p) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x, nb = N / kBlock;
    double s = 0.0;
    for (int64_t rb = blockIdx.x; rb < nb; ++rb) s += partial[rb * N + j];
    p[j] = s;
}

}  // namespace loo
