"""Small statistics helpers of the reference that its notebooks call beside the models (gsum/helpers.py:19, 264-307): highest
probability density intervals of a distribution or of a tabulated pdf, the median of a tabulated pdf, Cartesian products.
Host numpy / scipy on every backend: they work on a few hundred numbers.
"""
from __future__ import annotations

import numpy as np
from scipy.optimize import fmin

__all__ = ["hpd", "hpd_pdf", "median_pdf", "cartesian"]

_trapezoid = getattr(np, "trapezoid", None) or np.trapz              # numpy renamed trapz; either may be the one installed


def cartesian(*arrays):
    """The Cartesian product of 1-D arrays of lengths N_1 .. N_p as rows of an (N_1 * ... * N_p, p) array; the first array varies
    slowest."""
    grids = np.meshgrid(*arrays, indexing="ij")
    return np.stack(grids, axis=-1).reshape(-1, len(arrays))


def hpd(dist, alpha, *args):
    """``[low, high]``: the shortest interval of probability ``alpha`` of a scipy distribution (``dist(*args)`` when arguments are
    given).  The lower tail probability p minimises ``ppf(p + alpha) - ppf(p)``; the search is the reference's (Nelder-Mead from
    ``1 - alpha`` with ``ftol=1e-8``), so its results are reproduced to that tolerance."""
    frozen = dist(*args) if args else dist

    def width(p):
        return frozen.ppf(p + alpha) - frozen.ppf(p)

    p = fmin(width, 1 - alpha, ftol=1e-8, disp=False)[0]
    return frozen.ppf([p, p + alpha])


def hpd_pdf(pdf, alpha, x):
    """``[low, high]``: the highest probability density interval of mass ``alpha`` of a pdf tabulated at ``x``.  Every tabulated
    height is tried as the water line; the one whose region ``pdf >= height`` has trapezoid mass closest to ``alpha`` wins, and
    the interval spans the points strictly above it."""
    pdf, x = np.asarray(pdf), np.asarray(x)
    heights = np.unique(pdf)
    miss = [(_trapezoid(pdf[pdf >= h], x=x[pdf >= h]) - alpha) ** 2 for h in heights]
    inside = x[pdf > heights[np.argmin(miss)]]
    return np.array([np.min(inside), np.max(inside)])


def median_pdf(pdf, x):
    """The first ``x[i]`` at which the trapezoid mass of ``pdf[:i + 1]`` exceeds one half (the last x when none does)."""
    i = 0
    for i in range(len(x)):
        if _trapezoid(pdf[:i + 1], x[:i + 1]) > 0.5:
            break
    return x[i]
