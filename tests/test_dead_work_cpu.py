"""The row-group envelope of the grouped batch schedule (option wave_env) without a GPU: the envelope computed from
the kernel matrix as the build computes it, against the blocked numpy model of the bordered factorisation in the schedule's block sizes
(tests/test_zero_skip_cpu.py) -- every 16 x 256 block of a row group below a panel that the envelope calls dead is exactly +-0 in the
factor, so a panel wave that returns there is one that would have stored nothing."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import zero_skip_cases as zc
from test_zero_skip_cpu import BORDER, NB2, _bordered_factorisation, _nonzero


def test_far_plan_maps_and_rule(tmp_path):
    """the id -> tile maps and the plan's rule (kernels/zwin.h) against the host tile counts and the K-window rule: a stand-alone program"""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path / "far_plan_host")
    subprocess.run([gxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(root, "gsum_amd", "csrc"),
                    os.path.join(root, "tests", "c_host", "far_plan_host.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.startswith("ok "), res.stdout[-500:] + res.stderr[-500:]
    assert int(res.stdout.split()[1]) > 100_000


def envelope(K):
    """env[g] of the padded matrix (identity padding up to a multiple of 256): the first 256-column panel in which 16-row group g has, on
    or below the diagonal, an entry with bits other than +-0; S where there is none."""
    n = K.shape[0]
    np_ = -(-n // NB2) * NB2
    S = np_ // NB2
    A = np.zeros((np_, np_))
    A[:n, :n] = K
    A[np.arange(n, np_), np.arange(n, np_)] = 1.0
    nz = _nonzero(np.tril(A))
    env = np.full(np_ // 16, S, dtype=np.int64)
    for g in range(np_ // 16):
        cols = np.flatnonzero(nz[16 * g:16 * g + 16].any(axis=0))
        if cols.size:
            env[g] = cols[0] // NB2
    return env


def live_counts(env, np_):
    """(panel waves that load, panel waves launched) of one member over all outer steps; the border group always loads"""
    S, live, every = np_ // NB2, 0, 0
    for s in range(S):
        g0 = NB2 * (s + 1) // 16
        every += (np_ + BORDER) // 16 - g0
        live += int((env[g0:] <= s).sum()) + BORDER // 16
    return live, every


@functools.lru_cache(maxsize=None)
def _model(name, i):
    c = zc.cases()[name]
    K = zc.kernel_matrix(c, i)
    A, fl = _bordered_factorisation(K, c["Z"], skip=False)
    return K, A, fl


@pytest.mark.parametrize("name", list(zc.cases()))
def test_dead_blocks_are_exactly_zero_in_the_factor(name):
    c = zc.cases()[name]
    for i in range(len(c["kernels"])):
        K, A, fl = _model(name, i)
        env = envelope(K)
        np_ = A.shape[0] - BORDER
        S = np_ // NB2
        assert env.shape == (np_ // 16,) and env.min() >= 0 and env.max() < S          # (the diagonal: no group of the matrix rows is empty)
        nz = _nonzero(A)
        for g in range(np_ // 16):
            assert env[g] <= 16 * g // NB2                                               # never behind the group's own diagonal panel
            dead = nz[16 * g:16 * g + 16, :NB2 * env[g]]
            assert not dead.any(), (name, i, g, int(env[g]))
            # ... and what the model's panel solves flagged agrees: no flag in a dead block
            assert not fl[:env[g], g].any()


@pytest.mark.parametrize("name", list(zc.cases()))
def test_live_group_counts(name):
    c = zc.cases()[name]
    K, A, _ = _model(name, 0)
    np_ = A.shape[0] - BORDER
    live, every = live_counts(envelope(K), np_)
    print(name, "live", live, "of", every)
    assert 0 < live <= every
    if name in ("a", "h") or c["halfwidth"] or c["holes"]:
        assert live < every
    if name == "e":
        assert live == every


@pytest.mark.parametrize("name", ["f40", "f48", "f272"])
def test_the_envelope_is_a_superset_of_the_flags(name):
    """The holed cases: every group the model's panel solves flag in panel s is live there (env <= s); groups that are live and unflagged
    are left to gs_panel256_body, as before."""
    K, A, fl = _model(name, 0)
    env = envelope(K)
    np_ = A.shape[0] - BORDER
    for s in range(np_ // NB2):
        g = np.arange(NB2 * (s + 1) // 16, np_ // 16)
        assert np.all(env[g][fl[s, g]] <= s)
