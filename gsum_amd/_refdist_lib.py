"""ctypes binding of libgsum_refdist.so (C ABI: include/gsum_refdist.h), the reference distributions' own library."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _sidelib
from ._sidelib import DeviceHandle, _d, _i64

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgsum_refdist.so")

_p = C.c_void_p
_dp = C.POINTER(C.c_double)
PROTOTYPES = {
    "gsum_refdist_last_error": (C.c_char_p, []),
    "gsum_refdist_create": (C.c_int, [C.c_int32, _dp, C.c_int64, C.c_int64, C.POINTER(_p)]),
    "gsum_refdist_sort_columns": (C.c_int, [_p, _dp]),
    "gsum_refdist_row_percentiles": (C.c_int, [_p, _dp, C.c_int32, _dp]),
    "gsum_refdist_qq_bands": (C.c_int, [_p, _dp, C.c_int32, _dp, _dp]),
    "gsum_refdist_coverage": (C.c_int, [_p, _dp, _dp, C.c_int32, C.POINTER(C.c_int64)]),
    "gsum_refdist_times": (C.c_int, [_p, _dp, C.c_int32]),
    "gsum_refdist_free": (None, [_p]),
}
PHASES = ("h2d", "transpose", "column_sort", "percentiles", "coverage", "d2h")


def load_library(path: str | None = None):
    """dlopen libgsum_refdist.so and attach the prototypes.  Raises if it is absent (``python -m gsum_amd.build`` builds it)."""
    return _sidelib.load(LIB_PATH, PROTOTYPES, path)


def _check(lib, rc):
    _sidelib.check(lib, rc, "gsum_refdist_last_error")


def _matrix(a, name):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim != 2:
        raise ValueError(f"{name} must be 2-D, got shape {a.shape}")
    return a


class DeviceRefDist(DeviceHandle):
    """One n x m matrix resident on the device (uploaded once) and the operations of include/gsum_refdist.h on it."""

    _free = "gsum_refdist_free"
    _last_error = "gsum_refdist_last_error"

    def __init__(self, device, A):
        self._lib = lib = load_library()
        A = _matrix(A, "A")
        self.n, self.m = A.shape
        h = C.c_void_p()
        _check(lib, lib.gsum_refdist_create(int(device), _d(A), self.n, self.m, C.byref(h)))
        self._h = h

    def _handle(self):
        if self._h is None:
            raise ValueError("the device matrix is freed")
        return self._h

    def sort_columns(self, return_sorted=True):
        """The matrix becomes numpy.sort(matrix, axis=0) on the device; returned when ``return_sorted``."""
        out = np.empty((self.n, self.m)) if return_sorted else None
        _check(self._lib, self._lib.gsum_refdist_sort_columns(self._handle(), _d(out)))
        return out

    def row_percentiles(self, q):
        q = np.ascontiguousarray(q, dtype=np.float64).ravel()
        out = np.empty((q.shape[0], self.n))
        _check(self._lib, self._lib.gsum_refdist_row_percentiles(self._handle(), _d(q), q.shape[0], _d(out)))
        return out

    def qq_bands(self, q, return_sorted=False):
        q = np.ascontiguousarray(q, dtype=np.float64).ravel()
        bands = np.empty((q.shape[0], self.n))
        srt = np.empty((self.n, self.m)) if return_sorted else None
        _check(self._lib, self._lib.gsum_refdist_qq_bands(self._handle(), _d(q), q.shape[0], _d(bands), _d(srt)))
        return bands, srt

    def coverage(self, lower, upper):
        """int64 counts (m, K) of the points of each column strictly inside each of the K intervals (lower, upper: K x n)."""
        lower = _matrix(lower, "lower")
        upper = _matrix(upper, "upper")
        if lower.shape != upper.shape or lower.shape[1] != self.n:
            raise ValueError(f"lower and upper must both be (K, {self.n}), got {lower.shape} and {upper.shape}")
        K = lower.shape[0]
        counts = np.zeros((self.m, K), dtype=np.int64)
        _check(self._lib, self._lib.gsum_refdist_coverage(self._handle(), _d(lower), _d(upper), K, _i64(counts)))
        return counts

    def times(self, reset=False):
        """Device milliseconds (HIP events) spent so far, by phase (PHASES)."""
        return self._phase_times("gsum_refdist_times", PHASES, reset)
