// C ABI: gsum_sqrt_errors -- pivoted Cholesky (LAPACK dpstrf) and error vectors / Mahalanobis distances against a factor
// (part of gsum_capi.hip: included from there, in order -- one translation unit)
#pragma once
// Pivoted factorisation: the pivot search is dpstrf's blocked algorithm on scratch copies of the trailing matrix
// (k_pstrf_panel + gather + the bulk lower-triangular GEMM per panel of 128 steps; A itself is only read).  A full-rank search is
// followed by P^T A P in place of A and the library's own factorisation of it (gs_potrf): the factor then carries the tables every
// consumer of a factor reads (substitution tables, sibling images), and the Cholesky factor of P^T A P is unique.  A rank-deficient
// search leaves A as it was and reports *info = rank + 1.
static int gs_pstrf(gsum_ctx* ctx, gsum_mat* m, int64_t* info) {
    const int64_t n = m->n, ld = m->ld;
    hipStream_t s = ctx->cur->sm;
    // scratch: two trailing-matrix buffers (n + 128 rows, stride ld: room for the GEMM's last partial tile), W and its GEMM image (n x 128 each), the per-step candidates, bookkeeping
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t rows = (size_t)n + GS_NB, o_c0 = 0, o_c1 = up(rows * ld * 8), o_w = o_c1 + up(rows * ld * 8), o_wp = o_w + up((size_t)n * GS_PS_NB * 8),
                 o_pv = o_wp + up((size_t)n * GS_PS_NB * 8), o_pi = o_pv + up((size_t)GS_PS_NB * GS_PS_MAXG * 8),
                 o_fl = o_pi + up((size_t)GS_PS_NB * GS_PS_MAXG * 2 * 4), o_st = o_fl + 256, o_hi = o_st + 256, o_ds = o_hi + up(3 * GS_PS_NB * 4),
                 o_sl = o_ds + 256, o_p0 = o_sl + up((size_t)n * 4), o_p1 = o_p0 + up((size_t)n * 4), total = o_p1 + up((size_t)n * 4);
    if (gs_reserve(ctx, &ctx->pscratch, &ctx->pscratch_cap, total)) return -1;
    char* base = (char*)ctx->pscratch;
    double* buf[2] = {(double*)(base + o_c0), (double*)(base + o_c1)};
    double *W = (double*)(base + o_w), *Wp = (double*)(base + o_wp), *pval = (double*)(base + o_pv), *dstop = (double*)(base + o_ds);
    int *pidx = (int*)(base + o_pi), *stat = (int*)(base + o_st), *hist = (int*)(base + o_hi), *slot = (int*)(base + o_sl);
    int* perm[2] = {(int*)(base + o_p0), (int*)(base + o_p1)};
    unsigned* flags = (unsigned*)(base + o_fl);
    GS_CHECK(hipMemsetAsync(flags, 0, 256, s));
    GS_CHECK(hipMemsetAsync(stat, 0, 256, s));
    hipLaunchKernelGGL(k_pstrf_init, dim3(1), dim3(256), 0, s, (const double*)m->A, ld, (int)n, dstop, perm[0]);
    GS_CHECK(hipGetLastError());
    int pc = 0, cur = -1;                               // perm[pc]: the current order; buf[cur]: the trailing matrix (-1: still A itself)
    for (int64_t k0 = 0; k0 < n; k0 += GS_PS_NB) {
        const int64_t M = n - k0;
        const int nb = (int)std::min<int64_t>(GS_PS_NB, M);
        const int G = (int)std::min<int64_t>(GS_PS_MAXG, (M + 255) / 256);
        const int rpw = (int)((M + G - 1) / G);
        if (rpw > GS_PS_MAXROWS) GS_FAIL("pstrf: internal row split");
        const double* Cin = (cur < 0 ? m->A : buf[cur]) + k0 * ld + k0;
        GS_CHECK(hipMemsetAsync(flags + GS_PS_FL_COUNT, 0, sizeof(unsigned), s));
        hipLaunchKernelGGL(k_pstrf_panel, dim3((unsigned)G), dim3(256), 0, s, Cin, ld, (int)M, nb, (int)k0, rpw, W, pval, pidx, flags, stat,
                           hist, (const double*)dstop);
        GS_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_pstrf_slots, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const int*)hist, (const int*)stat, (int)n,
                           (int)k0, nb, slot, (const int*)perm[pc], perm[pc ^ 1]);
        GS_CHECK(hipGetLastError());
        pc ^= 1;
        if (M <= nb) break;
        const int nxt = cur == 0 ? 1 : 0;
        double* Cout = buf[nxt] + k0 * ld + k0;
        const int64_t R = M - nb;
        hipLaunchKernelGGL(k_pstrf_gather, dim3((unsigned)((R + 255) / 256), (unsigned)R), dim3(256), 0, s, Cin, Cout, ld, (int)M, nb,
                           (const int*)slot, (const int*)stat);
        GS_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_pstrf_wrows, dim3((unsigned)((R * GS_PS_NB + 255) / 256)), dim3(256), 0, s, (const double*)W, (int)M, nb,
                           (const int*)slot, Wp, (const int*)stat);
        GS_CHECK(hipGetLastError());
        if (gs_gemm(ctx, s, GS_BULK, Cout + nb * ld + nb, ld, Wp, GS_PS_NB, Wp, GS_PS_NB, R, R, GS_PS_NB, 1, 1, -1.0)) return -1;
        cur = nxt;
    }
    int hst[2] = {0, 0};
    unsigned hfl[2] = {0, 0};
    std::vector<int> hperm((size_t)n);
    GS_CHECK(hipMemcpyAsync(hst, stat, sizeof hst, hipMemcpyDeviceToHost, s));
    GS_CHECK(hipMemcpyAsync(hfl, flags, sizeof hfl, hipMemcpyDeviceToHost, s));
    GS_CHECK(hipMemcpyAsync(hperm.data(), perm[pc], (size_t)n * 4, hipMemcpyDeviceToHost, s));
    GS_CHECK(hipStreamSynchronize(s));
    if (hfl[GS_FL_ABORT]) {
        ctx->err = "pstrf: a pivot step's grid barrier timed out (the panel kernel's workgroups were not all resident); A is unchanged";
        return -1;
    }
    m->perm.assign(hperm.begin(), hperm.end());
    if (hst[1]) {                                       // rank deficient: A is untouched, the factor is not formed
        *info = (int64_t)hst[0] + 1;
        return 0;
    }
    // P^T A P in place of A (through the first trailing buffer), then its Cholesky factor
    hipLaunchKernelGGL(k_pstrf_permute, dim3((unsigned)((n + 255) / 256), (unsigned)n), dim3(256), 0, s, (const double*)m->A, ld, buf[0], ld,
                       (int)n, (const int*)perm[pc]);
    GS_CHECK(hipGetLastError());
    GS_CHECK(hipMemcpy2DAsync(m->A, (size_t)ld * 8, buf[0], (size_t)ld * 8, (size_t)n * 8, (size_t)n, hipMemcpyDeviceToDevice, s));
    if (!m->dperm) GS_CHECK(hipMalloc((void**)&m->dperm, (size_t)n * 4));
    GS_CHECK(hipMemcpyAsync(m->dperm, perm[pc], (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    return gs_potrf_info(ctx, m, info);
}

// E = L^-1 P^T (Y - mean 1^T) and md2 in chunks of columns: each chunk is centred, permuted and transposed into the rows of a sweep
// operand (k_centre_t), swept by gs_fwd_sweep -- the predictive path's own forward substitution --, then read out (k_untranspose,
// k_rowsumsq).  Chunks bound the device memory to ~256 MB of operand.
static int gs_sqrt_errors_run(gsum_ctx* ctx, gsum_mat* L, const double* Y, const double* mean, int64_t k, double* E, double* md2) {
    const int64_t n = L->n, np = L->np, ldb = np + GS_BORDER;
    const int64_t kc = std::max<int64_t>(1, std::min<int64_t>(k, ((int64_t)256 << 20) / (ldb * 8)));
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t o_bt = 0, o_y = up((size_t)kc * ldb * 8), o_e = o_y + up((size_t)n * kc * 8), o_m = o_e + up((size_t)n * kc * 8),
                 o_ss = o_m + up((size_t)n * 8), total = o_ss + up((size_t)kc * 8);
    if (gs_reserve(ctx, &ctx->scratch, &ctx->scratch_cap, total)) return -1;
    char* base = (char*)ctx->scratch;
    double *Bt = (double*)(base + o_bt), *dY = (double*)(base + o_y), *dE = (double*)(base + o_e), *dM = (double*)(base + o_m),
           *dSS = (double*)(base + o_ss);
    hipStream_t s = ctx->cur->sm;
    if (mean) GS_CHECK(hipMemcpyAsync(dM, mean, (size_t)n * 8, hipMemcpyHostToDevice, s));
    const int* perm = L->pivoted ? L->dperm : nullptr;
    for (int64_t j0 = 0; j0 < k; j0 += kc) {
        const int64_t c = std::min(kc, k - j0);
        GS_CHECK(hipMemcpy2DAsync(dY, (size_t)c * 8, Y + j0, (size_t)k * 8, (size_t)c * 8, (size_t)n, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_centre_t, dim3((unsigned)((np + 63) / 64), (unsigned)((c + 63) / 64)), dim3(256), 0, s, (const double*)dY, (int)c,
                           mean ? (const double*)dM : (const double*)nullptr, perm, (int)n, (int)np, Bt, ldb);
        GS_CHECK(hipGetLastError());
        if (gs_fwd_sweep(ctx, L, Bt, ldb, c)) return -1;
        if (md2) {
            hipLaunchKernelGGL(k_rowsumsq, dim3((unsigned)((c + 3) / 4)), dim3(256), 0, s, (const double*)Bt, ldb, (int)c, (int)np, dSS);
            GS_CHECK(hipGetLastError());
            GS_CHECK(hipMemcpyAsync(md2 + j0, dSS, (size_t)c * 8, hipMemcpyDeviceToHost, s));
        }
        if (E) {
            hipLaunchKernelGGL(k_untranspose, dim3((unsigned)((n + 63) / 64), (unsigned)((c + 63) / 64)), dim3(256), 0, s, (const double*)Bt, ldb,
                               (int)n, (int)c, dE);
            GS_CHECK(hipGetLastError());
            GS_CHECK(hipMemcpy2DAsync(E + j0, (size_t)k * 8, dE, (size_t)c * 8, (size_t)c * 8, (size_t)n, hipMemcpyDeviceToHost, s));
        }
        GS_CHECK(hipStreamSynchronize(s));             // (the next chunk overwrites the operand and the host copies are pageable)
    }
    return 0;
}

int gsum_sqrt_errors(gsum_ctx* ctx, gsum_mat* A, int32_t pivot, int64_t* piv, int64_t* info, const double* Y, const double* mean, int64_t n,
                     int64_t k, double* E, double* md2) {
    if (!ctx || !A || !info) return -2;
    GS_CHECK(hipSetDevice(ctx->device));
    if (pivot != 0 && pivot != 1) GS_FAIL("sqrt_errors: pivot must be 0 (Cholesky) or 1 (pivoted Cholesky)");
    if (n != A->n) GS_FAIL("sqrt_errors: n differs from the matrix order");
    if (k < 0) GS_FAIL("sqrt_errors: k must be >= 0");
    if (k > 0 && (E || md2) && !Y) GS_FAIL("sqrt_errors: Y is NULL");
    if (gs_refuse_failed(ctx, A, "sqrt_errors")) return -2;
    *info = 0;
    if (!A->factored) {
        A->solved_k = -1;
        A->pivoted = pivot;
        const int rc = pivot ? gs_pstrf(ctx, A, info) : gs_potrf_info(ctx, A, info);
        if (rc) return rc;
        if (pivot && piv)
            for (int64_t i = 0; i < n; ++i) piv[i] = A->perm[(size_t)i];
        if (*info > 0) {
            A->failed = true;           // (a rank-deficient search leaves A's entries as they were, a failed potrf does not: refused alike)
            return 0;
        }
    } else {
        if (A->pivoted != pivot)
            GS_FAIL(A->pivoted ? "sqrt_errors: the matrix holds a pivoted factor (pivot = 1)" : "sqrt_errors: the matrix holds an unpivoted factor (pivot = 0)");
        if (pivot && piv)
            for (int64_t i = 0; i < n; ++i) piv[i] = A->perm[(size_t)i];
    }
    if (k == 0 || (!E && !md2)) return 0;
    return gs_sqrt_errors_run(ctx, A, Y, mean, k, E, md2);
}
