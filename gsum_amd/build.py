"""Build the HIP library in-tree with hipcc for gfx950.

    python -m gsum_amd.build [--force] [--lab]

``libgsum_hip.so``      the product: the C ABI of include/gsum_hip.h, nothing else exported
``libgsum_hip_lab.so``  the same sources with -DGSUM_LAB: plus include/gsum_hip_debug.h (diagnostics, probes, microbenchmarks,
                        schedule switches); what tools/ and the schedule-equivalence tests load.  Built by ``--lab`` / ``build(lab=True)``
                        and by ``__graft_entry__.build()``.
``libgsum_vario.so``    the variogram (include/gsum_vario.h): its own small library, built by every product ``build()`` with its own
                        dependency list and up-to-date check.
``libgsum_refdist.so``  the reference distributions of GraphicalDiagnostic (include/gsum_refdist.h): column sort, row percentiles,
                        interval coverage.  Its own small library, built like the variogram's.
``libgsum_pointwise.so`` the grid log likelihood and the interval coverage of TruncationPointwise (include/gsum_pointwise.h).  Its own
                        small library, built like the variogram's.
``libgsum_loo.so``      the leave-one-out and leave-group-out diagnostics (include/gsum_loo.h): the inverse of a Cholesky factor, the
                        diagonal and the blocks of the precision matrix, (L L^T)^-1 R and the predictions of every group of a
                        partition from the points outside it.  Its own small library, built like the variogram's.
``libgsum_toep.so``     the Toeplitz likelihood path (include/gsum_toep.h): the Schur recursion of a symmetric Toeplitz matrix in
                        double-double arithmetic with the forward substitution beside it, the Gram matrices of the solved
                        columns, and the gradient pieces from the first column of the inverse (Levinson's recursion,
                        Gohberg-Semencul), and the panel route that solves any number of columns from one recursion.  Its own
                        small library, built like the variogram's.
``libgsum_band.so``     the banded likelihood path (include/gsum_band.h): kernel matrices in LAPACK band storage on sorted
                        one-dimensional points, their batched band Cholesky, forward substitution and Gram matrices.  Its own small
                        library, built like the variogram's; it includes kernels/build.hip.h for the kernel entries.
The side libraries are the entries of ``SIDE``, built by ``build_side``; their host files share csrc/host/sidelib.hip.h.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "csrc", "gsum_capi.hip")
KERNEL_PARTS = ("common", "build", "diag", "panel", "chain", "gemm_nt", "fused", "tile", "solve", "grad", "pstrf", "probes")
DEPS = [SRC, os.path.join(HERE, "csrc", "gsum_kernels.hip.h"), os.path.join(ROOT, "include", "gsum_hip.h"),
        os.path.join(ROOT, "include", "gsum_hip_debug.h")] + [os.path.join(HERE, "csrc", "kernels", f"{p}.hip.h") for p in KERNEL_PARTS]
HOST_PARTS = ("context", "gemm", "matrices", "potrf", "api_context", "api_operators", "pstrf", "api_fused", "wave", "api_lml", "api_multi", "api_grad", "api_measure")
DEPS += [os.path.join(HERE, "csrc", "host", f"{p}.hip.h") for p in HOST_PARTS] + [os.path.join(HERE, "csrc", "kernels", "zwin.h")]
OUT = os.path.join(HERE, "libgsum_hip.so")
OUT_LAB = os.path.join(HERE, "libgsum_hip_lab.so")
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-fvisibility=hidden", "-pthread",
               "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(HERE, "csrc")]
SIDE_SCAFFOLD = os.path.join(HERE, "csrc", "host", "sidelib.hip.h")      # the host scaffold every side library includes
# name -> (source, linker version script: only gsum_<name>_* exported, kernel header, public header, output)
SIDE = {name: (os.path.join(HERE, "csrc", f"gsum_{name}.hip"), os.path.join(HERE, "csrc", f"gsum_{name}.map"),
               os.path.join(HERE, "csrc", "kernels", f"{kernels}.hip.h"), os.path.join(ROOT, "include", f"gsum_{name}.h"),
               os.path.join(HERE, f"libgsum_{name}.so"))
        for name, kernels in (("vario", "variogram"), ("refdist", "refdist"), ("pointwise", "pointwise"), ("loo", "loo"), ("toep", "toeplitz"),
                              ("band", "band"))}
# what a side library includes beyond its own four files and the scaffold
SIDE_EXTRA = {"band": [os.path.join(HERE, "csrc", "kernels", "build.hip.h"), os.path.join(HERE, "csrc", "kernels", "common.hip.h"),
                       os.path.join(ROOT, "include", "gsum_hip.h")]}


def hipcc_path():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found")


def up_to_date(out=OUT, deps=None):
    return os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in (DEPS if deps is None else deps))


def build_side(name: str, force: bool = False, verbose: bool = False) -> str:
    """libgsum_<name>.so: the product's hipcc flags, only gsum_<name>_* exported."""
    src, vmap, kernels, header, out = SIDE[name]
    if not force and up_to_date(out, [src, vmap, kernels, header, SIDE_SCAFFOLD] + SIDE_EXTRA.get(name, [])):
        return out
    cmd = [hipcc_path()] + HIPCC_FLAGS + ["-Wl,--version-script=" + vmap, "-o", out, src]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return out


def build_vario(force: bool = False, verbose: bool = False) -> str:
    return build_side("vario", force, verbose)


def build_refdist(force: bool = False, verbose: bool = False) -> str:
    return build_side("refdist", force, verbose)


def build_pointwise(force: bool = False, verbose: bool = False) -> str:
    return build_side("pointwise", force, verbose)


def build_loo(force: bool = False, verbose: bool = False) -> str:
    return build_side("loo", force, verbose)


def build_toep(force: bool = False, verbose: bool = False) -> str:
    return build_side("toep", force, verbose)


def build_band(force: bool = False, verbose: bool = False) -> str:
    return build_side("band", force, verbose)


def build(force: bool = False, verbose: bool = False, lab: bool = False) -> str:
    out = OUT_LAB if lab else OUT
    if not lab:
        for name in SIDE:
            build_side(name, force, verbose)
    if not force and up_to_date(out):
        return out
    cmd = [hipcc_path()] + HIPCC_FLAGS + (["-DGSUM_LAB"] if lab else []) + ["-o", out, SRC]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return out


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
    for side in SIDE.values():
        print(side[-1])
    if "--lab" in sys.argv:
        print(build(force="--force" in sys.argv, verbose=True, lab=True))
