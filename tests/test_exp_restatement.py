"""The device kernel-build kernel does not call a generic exp: it restates, operation for operation, the
routine numpy's float64 exp dispatches to on AVX512 hosts (Intel SVML __svml_exp8_ha), because that
routine is not correctly rounded and a single differing ulp in one kernel value moves the uniform-grid
log-likelihood by 6e-10.  This CPU test pins the restatement: a Python model of
gs_exp_core (gsum_amd/csrc/kernels/build.hip.h: the one body behind gs_exp_np, gs_exp_np_t and gs_exp_np_nobranch) with exactly
rounded FMAs must equal np.exp bit for bit, and every constant of it is written once in the device sources.
The same check runs against the device in tests/test_gpu_parity.py::test_kernel_matrix_matches_sklearn."""
import math
import re
from fractions import Fraction as F

import numpy as np
import pytest

from conftest import ROOT

H = float.fromhex
HEX =r"-?0x[0-9a-f.]+p[+-]\d+"


def _core_source():
    """The range limit and gs_exp_core: the one place the restatement's constants are written."""
    src = open(f"{ROOT}/gsum_amd/csrc/kernels/build.hip.h").read()
    return src, src[src.index("#define GS_EXP_INRANGE"):src.index("double gs_exp_np_t(")]


def _device_constants():
    """Read the tables / coefficients straight from the HIP source, so the test pins what ships."""
    src, body = _core_source()
    assert "double gs_exp_core(" in body
    th = re.search(r"gs_exp_th\[16\] = \{(.*?)\};", src, re.S).group(1)
    tl = re.search(r"gs_exp_tl\[16\] = \{(.*?)\};", src, re.S).group(1)
    hexes = re.findall(HEX, body)
    return [H(v) for v in re.findall(HEX, th)], [H(v) for v in re.findall(HEX, tl)], [H(v) for v in hexes]


def fma(a, b, c):
    return float(F(a) * F(b) + F(c))       # exact, then one round-to-nearest-even


def exp_model(x, TH, TL, c):
    THR, L2E, SH, L2H, L2L, A1, A0, B1, B0, C1, C0 = c[:11]
    assert abs(x) < THR
    t = fma(x, L2E, SH)
    nn = t - SH
    dd = fma(x, L2E, -nn)
    N = nn - 0.0625 if dd < 0 else nn
    k16 = int(N * 16)
    j = k16 & 15
    R = fma(-N, L2H, x)
    R = fma(-N, L2L, R)
    R2 = R * R
    pA, pB, pC = fma(A1, R, A0), fma(B1, R, B0), fma(C1, R, C0)
    pp = fma(R2, pA, pB)
    pp = fma(R2, pp, pC)
    q = fma(pp, R, TL[j])
    return math.ldexp(fma(TH[j], q, TH[j]), k16 >> 4)


def _numpy_uses_svml():
    try:
        from numpy._core._multiarray_umath import __cpu_features__ as feats
    except Exception:
        return False
    return bool(feats.get("AVX512_SKX"))


def test_constants_parse():
    TH, TL, c = _device_constants()
    assert len(TH) == 16 and len(TL) == 16 and len(c) >= 11
    assert TH[0] == 1.0 and TH[8] == math.sqrt(2.0) and TL[0] == 0.0
    assert c[0] == H("0x1.61da04cbafe44p+9") and c[1] == H("0x1.71547652b82fep+0")


def test_each_constant_is_written_once():
    """One definition: the range limit, the four reduction constants and the six polynomial coefficients each occur exactly once
    in the device sources, so the model above pins the exp of every path (kernel build, fused likelihood, gradient, trees)."""
    import glob
    literals = re.findall(HEX, _core_source()[1])
    assert len(literals) == 11 and len(set(literals)) == 11
    files = [f for f in glob.glob(f"{ROOT}/gsum_amd/csrc/**/*", recursive=True) if f.endswith((".h", ".hip", ".hpp", ".cpp"))]
    assert f"{ROOT}/gsum_amd/csrc/kernels/build.hip.h" in files
    text = "".join(open(f).read() for f in files).lower()
    counts = {v: text.count(v.lstrip("-")) for v in literals}
    assert all(n == 1 for n in counts.values()), counts


@pytest.mark.skipif(not _numpy_uses_svml(), reason="host numpy does not dispatch exp to SVML (no AVX512_SKX)")
def test_exp_model_is_bit_identical_to_numpy():
    TH, TL, c = _device_constants()
    rng = np.random.RandomState(0)
    xs = np.concatenate([
        -0.125 * np.arange(0, 75) ** 2.0,                 # the S2/S3 uniform-grid kernel arguments
        -0.5 * ((0.1 * np.arange(40) - 0.1 * 4096) / 0.2 - (0.1 * 4096 - 0.1 * 4096) / 0.2) ** 2,
        -rng.rand(3000) * 50, rng.randn(1500) * 3, -rng.rand(1500) * 700, rng.rand(500) * 700,
        [-0.49999999999994316, 0.0, -1e-300, 1e-5, -707.0, 700.0, 1e-20, -1e-20, 5e-324]])
    xs = xs[np.abs(xs) < c[0]]
    ref = np.exp(xs)
    bad = [(float(x), exp_model(float(x), TH, TL, c), float(r)) for x, r in zip(xs, ref)
           if exp_model(float(x), TH, TL, c) != r]
    assert not bad, bad[:5]
    # and numpy's value is genuinely not the correctly rounded one here — the reason this exists
    from decimal import Decimal, getcontext
    getcontext().prec = 50
    assert float(np.exp(-0.125)) != float(Decimal(-0.125).exp())
