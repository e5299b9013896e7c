"""ctypes binding of libgsum_loo.so (C ABI: include/gsum_loo.h), the library of the leave-one-out diagnostics."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _sidelib
from ._sidelib import DeviceHandle, _d

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgsum_loo.so")

_p = C.c_void_p
_dp = C.POINTER(C.c_double)
PROTOTYPES = {
    "gsum_loo_last_error": (C.c_char_p, []),
    "gsum_loo_open": (C.c_int, [_dp, C.c_int64, C.c_int, C.POINTER(_p)]),
    "gsum_loo_precision_diag": (C.c_int, [_p, _dp, _dp]),
    "gsum_loo_solve": (C.c_int, [_p, _dp, C.c_int64, _dp]),
    "gsum_loo_times": (C.c_int, [_p, _dp, C.c_int32]),
    "gsum_loo_free": (None, [_p]),
}
PHASES = ("upload", "inverse", "reduce", "h2d", "solve", "d2h")


def load_library(path: str | None = None):
    """dlopen libgsum_loo.so and attach the prototypes.  Raises if it is absent (``python -m gsum_amd.build`` builds it)."""
    return _sidelib.load(LIB_PATH, PROTOTYPES, path)


def _check(lib, rc):
    _sidelib.check(lib, rc, "gsum_loo_last_error")


class DeviceLoo(DeviceHandle):
    """The inverse of the lower Cholesky factor L (n x n; the upper triangle is ignored) resident on the device, with the
    operations of include/gsum_loo.h on it.  ValueError where L's diagonal is not finite and positive or the matrix does not fit."""

    _free = "gsum_loo_free"

    def __init__(self, device, L):
        self._lib = lib = load_library()
        L = np.ascontiguousarray(L, dtype=np.float64)
        if L.ndim != 2 or L.shape[0] != L.shape[1] or L.shape[0] < 1:
            raise ValueError(f"L must be square and non-empty, got shape {L.shape}")
        self.n = L.shape[0]
        h = C.c_void_p()
        _check(lib, lib.gsum_loo_open(_d(L), self.n, int(device), C.byref(h)))
        self._h = h

    def _handle(self):
        if self._h is None:
            raise ValueError("the device data are freed")
        return self._h

    def precision_diag(self):
        """(p, sum_log_diag): diag((L L^T)^-1), shape (n,), and sum_i log L_ii."""
        p = np.empty(self.n)
        sld = C.c_double()
        _check(self._lib, self._lib.gsum_loo_precision_diag(self._handle(), _d(p), C.byref(sld)))
        return p, sld.value

    def solve(self, R):
        """(L L^T)^-1 R for R of shape (n, k), k >= 1."""
        R = np.ascontiguousarray(R, dtype=np.float64)
        if R.ndim != 2 or R.shape[0] != self.n or R.shape[1] < 1:
            raise ValueError(f"R must be ({self.n}, k) with k >= 1, got {R.shape}")
        out = np.empty_like(R)
        _check(self._lib, self._lib.gsum_loo_solve(self._handle(), _d(R), R.shape[1], _d(out)))
        return out

    def times(self, reset=False):
        """Device milliseconds (HIP events) spent so far, by phase (PHASES)."""
        ms = np.zeros(len(PHASES))
        _check(self._lib, self._lib.gsum_loo_times(self._handle(), _d(ms), int(bool(reset))))
        return dict(zip(PHASES, ms.tolist()))
