"""The Schur step of the Toeplitz path is written once (gsum_amd/csrc/kernels/toeplitz.hip.h: step_coeffs, rotate).  The routes of the
recursion (k_schur, k_schur_panel, k_schur_lead / k_schur_tiles) and the replay (k_coeffs, k_levinson) are bit for bit one another
because they call those two functions; a second copy of an expression would turn that back into a promise kept by hand, which only
the device tests would notice.  No device, no library: the sources are read as text."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = f"{ROOT}/gsum_amd/csrc/kernels/toeplitz.hip.h"

# (a + r * b) * c in double-double, whatever the operands are called: either half of the hyperbolic rotation
ROTATION = re.compile(r"dd_mul\(dd_add\((\w+),dd_mul\((\w+),(\w+)\)\),(\w+)\)")


def _device_code():
    """Every device source, comments dropped and whitespace removed."""
    files = sorted(f for f in glob.glob(f"{ROOT}/gsum_amd/csrc/**/*", recursive=True) if f.endswith((".h", ".hip", ".hpp", ".cpp")))
    assert HEADER in files
    text = "".join(open(f).read() for f in files)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return re.sub(r"\s+", "", text)


def test_the_step_is_written_once():
    code = _device_code()
    # the rotation's two expressions: u' = (us - rho v) / c and v' = (v - rho us) / c, the same coefficients, the operands swapped
    halves = ROTATION.findall(code)
    assert len(halves) == 2, halves
    (a, r, b, c), (a2, r2, b2, c2) = halves
    assert (a2, b2) == (b, a) and a != b and (r2, c2) == (r, c), halves
    # 1 / c = 1 / sqrt((1 - rho)(1 + rho)) and the failure test on rho's high word
    assert code.count("dd_rsqrt(dd_mul(dd_sub(") == 1
    assert code.count("fabs(rho.h)<1.0") == 1
    assert len(re.findall(r"fabs\(\w+\.h\)<1\.0", code)) == 1                 # nor under another name

    # the five kernels that rotate call rotate, the four that need (rho, 1 / c) from a pivot pair call step_coeffs, and both are
    # defined under the header's fp contract(off), before the first kernel
    src = re.sub(r"//[^\n]*", "", open(HEADER).read())
    heads = [(m.start(), m.group(1)) for m in re.finditer(r"__global__[^\n]*\bvoid (k_\w+)\(", src)]
    body = {name: src[at:(heads[i + 1][0] if i + 1 < len(heads) else len(src))] for i, (at, name) in enumerate(heads)}
    for k in ("k_schur", "k_schur_panel", "k_schur_lead", "k_schur_tiles", "k_levinson"):
        assert len(re.findall(r"\brotate\(", body[k])) == 1, k
    for k in ("k_schur", "k_schur_panel", "k_schur_lead", "k_coeffs"):
        assert len(re.findall(r"\bstep_coeffs\(", body[k])) == 1, k
    prelude = src[:heads[0][0]]
    assert prelude.index("fp contract(off)") < prelude.index(" step_coeffs(") < prelude.index(" rotate(")
