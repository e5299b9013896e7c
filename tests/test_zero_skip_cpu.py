"""The zero-skip of the grouped batch schedule without a GPU: the K-window rule of the trailing-update tiles against brute force (a
stand-alone host program over gsum_amd/csrc/kernels/zwin.h), the structure the test inputs claim (tests/zero_skip_cases.py), and a numpy
model of the blocked bordered factorisation that skips by the same flags and must equal the dense one under ==."""
from __future__ import annotations

import os
import shutil
import subprocess

import numpy as np
import pytest

import zero_skip_cases as zc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB2, BORDER = 256, 16


def test_window_rule_against_brute_force(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path / "zwin_host")
    subprocess.run([gxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "gsum_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c_host", "zwin_host.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.startswith("ok "), res.stdout[-500:] + res.stderr[-500:]
    assert int(res.stdout.split()[1]) > 5_000_000


def _nonzero(a):
    """bits other than +-0 (NaN and Inf count)"""
    return (np.ascontiguousarray(a).view(np.uint64) << np.uint64(1)) != 0


@pytest.fixture(scope="module")
def factors():
    """name -> lower Cholesky factor of the case's first kernel matrix (numpy: raises if it is not positive definite)"""
    return {name: np.linalg.cholesky(zc.kernel_matrix(c)) for name, c in zc.cases().items()}


@pytest.mark.parametrize("name", list(zc.cases()))
def test_every_kernel_of_every_case_is_positive_definite(name):
    c = zc.cases()[name]
    for i in range(len(c["kernels"])):
        np.linalg.cholesky(zc.kernel_matrix(c, i))
    assert 3 <= len(c["kernels"]) <= 6


def _halfwidth(M):
    i, j = np.nonzero(_nonzero(M))
    return int((i - j).max())


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_band_cases_have_the_claimed_half_width_in_matrix_and_factor(name, factors):
    c = zc.cases()[name]
    assert _halfwidth(np.tril(zc.kernel_matrix(c))) == c["halfwidth"]
    assert _halfwidth(factors[name]) == c["halfwidth"]               # no pivoting: the envelope is kept


def test_case_a_has_subnormal_entries_at_the_band_edge():
    K = zc.kernel_matrix(zc.cases()["a"])
    tiny = np.finfo(float).tiny
    for lag in (76, 77):
        v = K[lag, 0]
        assert 0.0 < v < tiny, (lag, v)
    assert K[78, 0] == 0.0


def test_dense_case_has_no_zero(factors):
    L = factors["e"]
    assert L.shape[0] % NB2 == 0                                   # no padding rows: they would be zero under every panel
    assert _nonzero(L)[np.tril_indices(L.shape[0])].all()


def _panel_flags(L, n):
    """flags[p, g] of the factor's solved panels: 16-row group g (of the padded, bordered matrix) has a nonzero in columns [256 p, 256 p + 256)"""
    np_ = -(-n // NB2) * NB2
    S, ng = np_ // NB2, (np_ + BORDER) // 16
    fl = np.zeros((S, ng), dtype=bool)
    nz = _nonzero(L)
    for p in range(S):
        rows = nz[:, NB2 * p:NB2 * (p + 1)].any(axis=1)
        for g in range(NB2 * (p + 1) // 16, ng):
            fl[p, g] = rows[16 * g:16 * g + 16].any()
    return fl


@pytest.mark.parametrize("name", ["f40", "f48", "f272"])
def test_cluster_cases_have_zero_groups_between_nonzero_ones(name, factors):
    """In some panel a 16-row group that is all zero lies between two that are not (matrix rows only: the right-hand-side rows are
    nonzero everywhere): the flags cannot be replaced by one band width."""
    n = zc.N
    fl = _panel_flags(factors[name], n)[:, :n // 16]
    holes = 0
    for p in range(fl.shape[0]):
        on = np.flatnonzero(fl[p])
        if on.size:
            holes += int((~fl[p, on[0]:on[-1] + 1]).sum())
    assert holes > 0


def _plan(np_, depth=4):
    """gs_wave_bulk_plan: per outer step (near?, K, first panel of the macro-step)"""
    S = np_ // NB2
    plan, a = [None] * S, 0
    while a < S:
        r2, L = NB2 * (a + 1), 1
        while L < depth and r2 + NB2 * (L + 1) <= np_:
            L += 1
        for i in range(L):
            plan[a + i] = (i < L - 1, NB2 * (i + 1), a)
        a += L
    return plan


def _window(fl, first, nP, gA0, nA, gB0, nB):
    need = [bool(fl[p, gA0:gA0 + nA].any() and fl[p, gB0:gB0 + nB].any()) for p in range(first, first + nP)]
    if not any(need):
        return 0, 0
    return NB2 * need.index(True), NB2 * (nP - need[::-1].index(True))


def _bordered_factorisation(K, Z, skip, counts=None):
    """The batch schedule's arithmetic in numpy: outer steps of 256 columns on the padded matrix bordered by the right-hand-side rows,
    panel solves per 16-row group, trailing updates per 128 x 64 tile and per 256-column operand panel in ascending order (near updates of
    the next panel's columns inside a macro-step, one far update at its end).  skip: by the flags, as the device code does."""
    from scipy.linalg import solve_triangular
    n, k = Z.shape
    np_ = -(-n // NB2) * NB2
    naug, S = np_ + BORDER, np_ // NB2
    A = np.zeros((naug, naug))
    A[:n, :n] = K
    A[np.arange(n, np_), np.arange(n, np_)] = 1.0
    A[np_:np_ + k, :n] = Z.T
    fl = np.zeros((S, naug // 16), dtype=bool)
    plan = _plan(np_)
    for s in range(S):
        c0, r2 = NB2 * s, NB2 * (s + 1)
        A[c0:r2, c0:r2] = np.linalg.cholesky(A[c0:r2, c0:r2])
        Ld = A[c0:r2, c0:r2]
        for g in range(r2 // 16, naug // 16):
            rows = A[16 * g:16 * g + 16, c0:r2]
            if not skip or _nonzero(rows).any():
                rows[...] = solve_triangular(Ld, rows.T, lower=True).T
            fl[s, g] = _nonzero(rows).any()
        near, Kk, first = plan[s]
        M, N, nP = naug - r2, (NB2 if near else naug - r2), Kk // NB2
        off = M % 128 if M > 128 else 0                       # the shifted grid: the partial tile row first
        row_tiles = ([(0, off)] if off else []) + [(m0, min(m0 + 128, M)) for m0 in range(off, M, 128)]
        for m0, m1 in row_tiles:
            for n0 in range(0, N, 64):
                n1 = min(n0 + 64, N)
                if not near and n0 > m1 - 1:
                    break                                       # lower tiles only
                lo, hi = (0, Kk) if not skip else _window(fl, first, nP, (r2 + m0) // 16, (m1 - m0) // 16, (r2 + n0) // 16, (n1 - n0) // 16)
                if counts is not None:
                    counts[0] += 1
                    counts[1] += hi > lo
                for kp in range(lo, hi, NB2):
                    ka = NB2 * first + kp
                    A[r2 + m0:r2 + m1, r2 + n0:r2 + n1] -= A[r2 + m0:r2 + m1, ka:ka + NB2] @ A[r2 + n0:r2 + n1, ka:ka + NB2].T
    return A, fl


@pytest.mark.parametrize("name", list(zc.cases()))
def test_skipping_by_the_flags_equals_the_dense_factorisation(name):
    c = zc.cases()[name]
    K = zc.kernel_matrix(c)
    dense, fl_dense = _bordered_factorisation(K, c["Z"], skip=False)
    counts = [0, 0]
    skipped, fl = _bordered_factorisation(K, c["Z"], skip=True, counts=counts)
    low = np.tril_indices(dense.shape[0])
    assert np.all(dense[low] == skipped[low])                    # (== : zeros may differ in sign)
    assert np.array_equal(fl, fl_dense)
    if c["dense"]:
        assert counts[1] == counts[0] and fl[0, NB2 // 16:].all()
    elif c["halfwidth"] or c["holes"]:
        assert counts[1] < counts[0]
    # the model is the factorisation: its factor is numpy's to rounding, its flags are the factor's zero structure
    n = K.shape[0]
    L = np.linalg.cholesky(K)
    assert np.allclose(np.tril(dense[:n, :n]), L, rtol=0, atol=1e-6 * np.abs(L).max())


@pytest.mark.parametrize("name", list(zc.cases()))
def test_the_cpu_reference_is_defined_to_the_bound_on_every_case(name):
    """The GPU test holds the batch's log-likelihoods to 1e-10 of the CPU oracle's.  That asks something only where the oracle's own value
    does not move by more than that with the order of summation: here the blocked numpy model (skipping by the flags) against scipy's
    Cholesky (the oracle), every kernel of the case, same bound."""
    from gsum_amd._cpu import CpuContext
    from gsum_amd.conjugate import lml_from_gram_batch
    import gsum_amd
    c = zc.cases()[name]
    n, k = c["Z"].shape
    cpu = CpuContext()
    cpu.set_inputs(c["X"], c["Z"])
    G2, s2, info = cpu.lml_resident([gsum_amd.describe_kernel(kern, 1) for kern in c["kernels"]], c["nugget"])
    assert np.all(info == 0)
    ref = lml_from_gram_batch(G2, s2, n, 0.0, 0.0, 1, 1)
    for i in range(len(c["kernels"])):
        A, _ = _bordered_factorisation(zc.kernel_matrix(c, i), c["Z"], skip=True)
        np_ = A.shape[0] - BORDER
        G = -np.tril(A[np_:np_ + k, np_:np_ + k])
        G = G + np.tril(G, -1).T
        sld = np.log(np.diag(A)[:n]).sum()
        lml = lml_from_gram_batch(G[None], np.array([sld]), n, 0.0, 0.0, 1, 1)[0]
        assert abs(lml - ref[i]) <= 1e-10 * abs(ref[i]), (name, i, abs(lml - ref[i]) / abs(ref[i]))
