#!/usr/bin/env python3
"""Generate tests/golden/vario_lattice_truth.json: the mpmath truth of tests/vario_lattice.py for every lattice cov case, so that the
GPU tests need no mpmath.  Data only: gamma~ of the rational model, the truth sums, E, M, sq and the one-ulp-rho sensitivity.
Needs mpmath; no GPU, no reference checkout.  Usage:  python tests/golden/make_vario_lattice_truth.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import vario_lattice  # noqa: E402


def main():
    path = os.path.join(HERE, "vario_lattice_truth.json")
    with open(path, "w") as f:
        json.dump(vario_lattice.make_fixture(), f, sort_keys=True)
    print(path, os.path.getsize(path), "bytes")
    import mpmath
    import numpy
    versions = os.path.join(HERE, "VERSIONS.json")                  # this file's line beside the other fixtures' versions
    with open(versions) as f:
        rec = json.load(f)
    rec["vario_lattice_truth.json"] = f"mpmath {mpmath.__version__} at 30 digits, numpy {numpy.__version__}; no reference checkout"
    with open(versions, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
