#!/usr/bin/env python3
"""The known answer of the blocked route of the Toeplitz path just beyond the one-workgroup limit -> tests/golden/toeplitz_blocked.json.

The truth is that of make_golden_toeplitz_classes.py, imported from there: the Schur recursion with the forward substitution beside it
in mpmath at 60 digits on the Toeplitz matrix of the fp64 first column (checked there against the dense mpmath Cholesky answers and the
ARFIMA closed form).  The file holds

  "arfima": G = Z^T T^-1 Z of tests/toeplitz_cases.py: arfima_column(8193, d) with Z = rhs_columns(8193, 4) for d in DS, with the
            sum_log_diag of that fp64 column and of the closed form beside it.

About twenty minutes per first column with mpmath's pure-Python backend; the two run side by side.

    python tests/golden/make_golden_toeplitz_blocked.py [--jobs N]
"""
import argparse
import json
import multiprocessing
import os

import make_golden_toeplitz_classes as classes

HERE = os.path.dirname(os.path.abspath(__file__))
N = 8193


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=2)
    args = ap.parse_args()
    classes.check_closed_form()
    with multiprocessing.Pool(args.jobs) as pool:
        arfima = pool.map(classes.run_arfima, [(N, d) for d in classes.tc.DS], chunksize=1)
    arfima.sort(key=lambda r: -r["d"])
    with open(os.path.join(HERE, "toeplitz_blocked.json"), "w") as f:
        json.dump(dict(method=f"make_golden_toeplitz_classes.mp_schur_gram: the Schur recursion with the forward substitution beside it "
                              f"in mpmath at {classes.DIGITS} digits, rounded to fp64 at the end (make_golden_toeplitz_blocked.py)",
                       digits=classes.DIGITS,
                       inputs=f"t = toeplitz_cases.arfima_column({N}, d), Z = toeplitz_cases.rhs_columns({N}, {classes.COLS})",
                       arfima=arfima), f)


if __name__ == "__main__":
    main()
