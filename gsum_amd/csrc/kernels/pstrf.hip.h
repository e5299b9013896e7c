// pivoted Cholesky (LAPACK dpstrf, lower, tol < 0): the pivot search, and the permute / centre / transpose kernels of gsum_sqrt_errors
// (part of gsum_kernels.hip.h: included from there, in order; gfx950 only)
#pragma once
// The search runs dpstrf's blocked algorithm on a scratch copy of the matrix (host driver: host/pstrf.hip.h).  One panel of up to 128
// pivot steps is ONE launch of k_pstrf_panel: G workgroups own contiguous slices of the trailing rows and meet once per step at a
// grid barrier in HBM (the release / acquire form of the chain kernel's flags, chain.hip.h).  During a panel the trailing matrix is
// read-only: the panel's columns go to W (column-major, M rows per column) in the rows' order at the start of the panel, and LAPACK's
// row / column swaps are kept as bookkeeping (the physical position of every row), so a swap moves no data and MAXLOC's tie-break
// (the first physical position) is kept exactly.  After the panel, k_pstrf_slots resolves the positions, k_pstrf_gather moves the
// trailing matrix into the new order, k_pstrf_wrows the panel rows into GEMM operand layout, and the trailing update is the library's
// fp64-MFMA lower-triangular GEMM.
#define GS_PS_NB 128                  // pivot steps per panel (the GEMM's K)
#define GS_PS_MAXG 128                // workgroups of one panel launch at most
#define GS_PS_MAXROWS 1024            // rows one workgroup owns at most
#define GS_PS_FL_COUNT 1              // flags[GS_FL_ABORT]: a barrier timed out; flags[1]: the step barrier's arrival counter
// stat[0]: global step at which the search stopped (the rank), stat[1]: 1 once it stopped
__device__ __forceinline__ bool gs_ps_better(double v1, int p1, double v2, int p2) { return v1 > v2 || (v1 == v2 && p1 < p2); }

__device__ __forceinline__ void gs_ps_wave_best(double& v, int& p, int& r) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double v2 = __shfl_xor(v, off, 64);
        const int p2 = __shfl_xor(p, off, 64), r2 = __shfl_xor(r, off, 64);
        if (gs_ps_better(v2, p2, v, p)) { v = v2; p = p2; r = r2; }
    }
}

// dstop = n eps max_i A_ii (dpstrf with tol < 0; eps = dlamch('Epsilon') = 2^-53), perm = identity
__global__ __launch_bounds__(256) void k_pstrf_init(const double* A, int64_t ld, int n, double* dstop, int* perm) {
    __shared__ double red[4];
    double m = -INFINITY;
    for (int i = threadIdx.x; i < n; i += 256) {
        const double v = A[(int64_t)i * ld + i];
        m = (v > m || v != v) ? v : m;          // a NaN diagonal propagates into dstop: step 0 stops, info 1 (LAPACK stops too, at a rank
                                                // that depends on where the NaN lies: rank 4 for 2 I_5 with A(3,3) NaN, 0 with A(1,1) NaN)
        perm[i] = i;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double o = __shfl_xor(m, off, 64);
        m = (o > m || o != o) ? o : m;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        double b = red[0];
        for (int w = 1; w < 4; ++w) b = (red[w] > b || red[w] != red[w]) ? red[w] : b;
        dstop[0] = (double)n * 1.1102230246251565e-16 * b;
        dstop[1] = b;
    }
}

// One panel: steps t = 0 .. nb - 1 at global step k0 + t.  C: the trailing matrix at (k0, k0) (lower triangle read), M = n - k0 rows.
// W: nb columns of M doubles.  part: GS_PS_NB x G x {value, position, row} candidates.  hist: GS_PS_NB x {pivot row, its position,
// the row that moved there}.  Every spin is bounded (GS_CH_TIMEOUT); a timeout sets flags[GS_FL_ABORT] and every workgroup leaves.
__global__ __launch_bounds__(256) void k_pstrf_panel(const double* __restrict__ C, int64_t ldc, int M, int nb, int k0, int rpw, double* W,
                                                     double* pval, int* pidx, unsigned* flags, int* stat, int* hist, const double* dstop_p) {
    __shared__ double work_s[GS_PS_MAXROWS], diag_s[GS_PS_MAXROWS];
    __shared__ int pos_s[GS_PS_MAXROWS];
    __shared__ double wp[GS_PS_NB];
    __shared__ int mv_pos[GS_PS_NB], mv_row[GS_PS_NB];
    __shared__ double red_v[4];
    __shared__ int red_p[4], red_r[4];
    __shared__ double pick_v;
    __shared__ int pick_p, pick_r, pick_rt, sh_ok;
    if (gs_flag_ld(flags + GS_FL_ABORT) != 0u || __hip_atomic_load(stat + 1, GS_RLX_AGENT) != 0) return;   // an earlier panel stopped
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = blockIdx.x, G = gridDim.x;
    const int base = g * rpw, rend = min(M, base + rpw), own = max(0, rend - base);
    const double dstop = dstop_p[0];
    for (int li = tid; li < own; li += 256) {
        const int r = base + li;
        work_s[li] = 0.0;                                     // dpstrf: WORK(K:N) = 0 at the start of every panel
        diag_s[li] = C[(int64_t)r * ldc + r];
        pos_s[li] = r;
    }
    __syncthreads();
    for (int t = 0; t < nb; ++t) {
        // (1) candidates of this workgroup's rows: WORK(I) += A(I, J-1)^2, WORK(N+I) = A(I,I) - WORK(I), MAXLOC over positions >= t
        double bv = -INFINITY;
        int bp = 0x7fffffff, br = -1;
        for (int li = tid; li < own; li += 256) {
            const int p = pos_s[li];
            if (p < t) continue;
            if (t > 0) {
                const double x = W[(int64_t)(t - 1) * M + base + li];
                work_s[li] += x * x;
            }
            const double dv = diag_s[li] - work_s[li];
            if (gs_ps_better(dv, p, bv, bp)) { bv = dv; bp = p; br = base + li; }
        }
        gs_ps_wave_best(bv, bp, br);
        if (lane == 0) { red_v[w] = bv; red_p[w] = bp; red_r[w] = br; }
        __syncthreads();
        if (tid == 0) {
            for (int q = 1; q < 4; ++q)
                if (gs_ps_better(red_v[q], red_p[q], red_v[0], red_p[0])) { red_v[0] = red_v[q]; red_p[0] = red_p[q]; red_r[0] = red_r[q]; }
            const int64_t o = (int64_t)t * G + g;
            pval[o] = red_v[0];
            pidx[2 * o] = red_p[0];
            pidx[2 * o + 1] = red_r[0];
        }
        // (2) grid barrier: every storing wave drains, one lane releases and arrives; one wave polls and acquires
        gs_drain();
        __syncthreads();
        if (tid == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            gs_drain();
            gs_flag_add(flags + GS_PS_FL_COUNT);
        }
        if (!gs_wg_wait_ge(flags + GS_PS_FL_COUNT, (unsigned)(G * (t + 1)), flags, &sh_ok)) return;
        // (3) the step's pivot: the best candidate of all workgroups (same order of comparison everywhere: identical result)
        if (w == 0) {
            double v = -INFINITY;
            int p = 0x7fffffff, r = -1;
            for (int q = lane; q < G; q += 64) {
                const int64_t o = (int64_t)t * G + q;
                const double v2 = pval[o];
                const int p2 = pidx[2 * o], r2 = pidx[2 * o + 1];
                if (gs_ps_better(v2, p2, v, p)) { v = v2; p = p2; r = r2; }
            }
            gs_ps_wave_best(v, p, r);
            // the row now at position t: the newest move onto position t, else the row that started there
            int found = -1;
            for (int q = lane; q < t; q += 64)
                if (mv_pos[q] == t) found = max(found, q);
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) found = max(found, __shfl_xor(found, off, 64));
            if (lane == 0) {
                pick_v = v; pick_p = p; pick_r = r;
                pick_rt = found >= 0 ? mv_row[found] : t;
            }
        }
        __syncthreads();
        const double ajj = pick_v;
        const int prow = pick_r, ppos = pick_p, rt = pick_rt;
        if (!(ajj > dstop) || !(ajj > 0.0) || prow < 0) {          // dpstrf: AJJ <= DSTOP or NaN -> RANK = J - 1
            if (g == 0 && tid == 0) {
                __hip_atomic_store(stat, k0 + t, GS_RLX_AGENT);
                __hip_atomic_store(stat + 1, 1, GS_RLX_AGENT);
            }
            return;
        }
        // (4) the swap as bookkeeping: the pivot row goes to position t, the row at position t to the pivot's old position
        if (tid == 0) { mv_pos[t] = ppos; mv_row[t] = rt; }
        if (prow >= base && prow < rend) pos_s[prow - base] = t;
        if (rt != prow && rt >= base && rt < rend) pos_s[rt - base] = ppos;
        if (g == 0 && tid == 0) { hist[3 * t] = prow; hist[3 * t + 1] = ppos; hist[3 * t + 2] = rt; }
        if (tid < t) wp[tid] = W[(int64_t)tid * M + prow];       // the pivot row's panel entries (written by its owner, acquired above)
        __syncthreads();
        // (5) column t: A(I, J) -= A(I, K:J-1) A(J, K:J-1)^T, scaled by 1 / sqrt(AJJ)
        const double inv = 1.0 / sqrt(ajj);
        for (int li = tid; li < own; li += 256) {
            if (pos_s[li] <= t) continue;
            const int r = base + li;
            double a = r >= prow ? C[(int64_t)r * ldc + prow] : C[(int64_t)prow * ldc + r];
            for (int q = 0; q < t; ++q) a -= W[(int64_t)q * M + r] * wp[q];
            W[(int64_t)t * M + r] = a * inv;
        }
    }
}

// The order after a panel: slot[s] = the row (in the panel's starting order) at position s; the global permutation follows
// (perm_out[k0 + s] = perm_in[k0 + slot[s]]).  steps: nb, or fewer where the search stopped inside this panel.
__global__ __launch_bounds__(256) void k_pstrf_slots(const int* hist, const int* stat, int n, int k0, int nb, int* slot, const int* perm_in,
                                                     int* perm_out) {
    __shared__ int h[3 * GS_PS_NB];
    const int stopped = stat[1], at = stat[0];
    const int steps = stopped ? max(0, min(nb, at - k0)) : nb;
    for (int i = threadIdx.x; i < 3 * steps; i += 256) h[i] = hist[i];
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (stopped && at < k0) { perm_out[i] = perm_in[i]; return; }       // an earlier panel stopped: nothing moves any more
    if (i < k0) { perm_out[i] = perm_in[i]; return; }
    const int s = i - k0;
    int row = s;
    if (s < steps) row = h[3 * s];
    else
        for (int q = steps - 1; q >= 0; --q)
            if (h[3 * q + 1] == s) { row = h[3 * q + 2]; break; }
    slot[s] = row;
    perm_out[i] = perm_in[k0 + row];
}

// trailing matrix in the new order (lower triangle, rows / columns nb .. M - 1 of the panel's frame): Cn[s][s'] = Co[slot s][slot s']
__global__ __launch_bounds__(256) void k_pstrf_gather(const double* Co, double* Cn, int64_t ldc, int M, int nb, const int* slot, const int* stat) {
    if (stat[1]) return;
    const int s = nb + blockIdx.y, c = nb + blockIdx.x * 256 + threadIdx.x;
    if (c > s) return;
    const int a = slot[s], b = slot[c];
    Cn[(int64_t)s * ldc + c] = a >= b ? Co[(int64_t)a * ldc + b] : Co[(int64_t)b * ldc + a];
}

// the panel's rows nb .. M - 1 in the new order, row-major with K = GS_PS_NB contiguous: the operand of the trailing update
__global__ __launch_bounds__(256) void k_pstrf_wrows(const double* W, int M, int nb, const int* slot, double* Wp, const int* stat) {
    if (stat[1]) return;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)(M - nb) * GS_PS_NB) return;
    const int s = (int)(e / GS_PS_NB), t = (int)(e % GS_PS_NB);
    Wp[e] = W[(int64_t)t * M + slot[nb + s]];
}

// P^T A P (full symmetric n x n from the lower triangle of A) into T
__global__ __launch_bounds__(256) void k_pstrf_permute(const double* A, int64_t lda, double* T, int64_t ldt, int n, const int* perm) {
    const int i = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const int a = perm[i], b = perm[j];
    T[(int64_t)i * ldt + j] = a >= b ? A[(int64_t)a * lda + b] : A[(int64_t)b * lda + a];
}

// Bt (kc rows x ldb, the forward sweep's layout: one row per right-hand side) <- (P^T (Y - mean 1^T))^T, zero in columns n .. np - 1.
// Y: n x kc row-major on the device; perm == NULL: P = I.  64 x 64 tiles through LDS (both sides coalesced).
__global__ __launch_bounds__(256) void k_centre_t(const double* Y, int kc, const double* mean, const int* perm, int n, int np, double* Bt,
                                                  int64_t ldb) {
    __shared__ double tile[64][65];
    const int i0 = blockIdx.x * 64, j0 = blockIdx.y * 64, tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int r = ty; r < 64; r += 4) {
        const int i = i0 + r, j = j0 + tx;
        double v = 0.0;
        if (i < n && j < kc) {
            const int src = perm ? perm[i] : i;
            v = Y[(int64_t)src * kc + j] - (mean ? mean[src] : 0.0);
        }
        tile[r][tx] = v;
    }
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        const int j = j0 + r, i = i0 + tx;
        if (j < kc && i < np) Bt[(int64_t)j * ldb + i] = tile[tx][r];
    }
}

// E (n x kc row-major) <- the first n columns of Bt, transposed
__global__ __launch_bounds__(256) void k_untranspose(const double* Bt, int64_t ldb, int n, int kc, double* E) {
    __shared__ double tile[64][65];
    const int i0 = blockIdx.x * 64, j0 = blockIdx.y * 64, tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int r = ty; r < 64; r += 4) {
        const int j = j0 + r, i = i0 + tx;
        tile[r][tx] = (j < kc && i < n) ? Bt[(int64_t)j * ldb + i] : 0.0;
    }
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        const int i = i0 + r, j = j0 + tx;
        if (i < n && j < kc) E[(int64_t)i * kc + j] = tile[tx][r];
    }
}
