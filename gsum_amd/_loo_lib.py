"""ctypes binding of libgsum_loo.so (C ABI: include/gsum_loo.h), the library of the leave-one-out diagnostics."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _sidelib
from ._sidelib import DeviceHandle, _d, _i64

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgsum_loo.so")

_p = C.c_void_p
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int64)
PROTOTYPES = {
    "gsum_loo_last_error": (C.c_char_p, []),
    "gsum_loo_open": (C.c_int, [_dp, C.c_int64, C.c_int, C.POINTER(_p)]),
    "gsum_loo_precision_diag": (C.c_int, [_p, _dp, _dp]),
    "gsum_loo_solve": (C.c_int, [_p, _dp, C.c_int64, _dp]),
    "gsum_loo_times": (C.c_int, [_p, _dp, C.c_int32]),
    "gsum_loo_precision_block": (C.c_int, [_p, _ip, C.c_int64, _dp]),
    "gsum_loo_folds": (C.c_int, [_p, _ip, _ip, C.c_int64, _dp, C.c_int64, _dp, _dp, _dp, _dp]),
    "gsum_loo_fold_budget": (C.c_int, [_p, C.c_int64]),
    "gsum_loo_fold_times": (C.c_int, [_p, _dp, C.c_int32]),
    "gsum_loo_free": (None, [_p]),
}
PHASES = ("upload", "inverse", "reduce", "h2d", "solve", "d2h")
FOLD_PHASES = ("gather", "gram", "factor", "inverse", "logdet", "apply", "scatter")


def load_library(path: str | None = None):
    """dlopen libgsum_loo.so and attach the prototypes.  Raises if it is absent (``python -m gsum_amd.build`` builds it)."""
    return _sidelib.load(LIB_PATH, PROTOTYPES, path)


def _check(lib, rc):
    _sidelib.check(lib, rc, "gsum_loo_last_error")


class DeviceLoo(DeviceHandle):
    """The inverse of the lower Cholesky factor L (n x n; the upper triangle is ignored) resident on the device, with the
    operations of include/gsum_loo.h on it.  ValueError where L's diagonal is not finite and positive or the matrix does not fit."""

    _free = "gsum_loo_free"
    _last_error = "gsum_loo_last_error"

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
        return self._phase_times("gsum_loo_times", PHASES, reset)

    def precision_block(self, idx):
        """The rows and columns ``idx`` of (L L^T)^-1, shape (g, g), in the order of ``idx``."""
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        if idx.ndim != 1:
            raise ValueError(f"idx must be one-dimensional, got shape {idx.shape}")
        P = np.empty((idx.size, idx.size))
        _check(self._lib, self._lib.gsum_loo_precision_block(self._handle(), _i64(idx), idx.size, _d(P)))
        return P

    def folds(self, fold_ptr, fold_idx, R):
        """(resid (n, k), var (n,), md2 (n_folds, k), logdet (n_folds,)) of the groups fold_idx[fold_ptr[q]:fold_ptr[q + 1]] for the
        residual curves R (n, k).  numpy.linalg.LinAlgError where a group's block of the precision does not factor."""
        R = np.ascontiguousarray(R, dtype=np.float64)
        if R.ndim != 2 or R.shape[0] != self.n or R.shape[1] < 1:
            raise ValueError(f"R must be ({self.n}, k) with k >= 1, got {R.shape}")
        fold_ptr = np.ascontiguousarray(fold_ptr, dtype=np.int64)
        fold_idx = np.ascontiguousarray(fold_idx, dtype=np.int64)
        if fold_ptr.ndim != 1 or fold_ptr.size < 2 or fold_idx.shape != (self.n,):
            raise ValueError(f"fold_ptr must be (n_folds + 1,) and fold_idx ({self.n},), got {fold_ptr.shape} and {fold_idx.shape}")
        nf, k = fold_ptr.size - 1, R.shape[1]
        resid, var, md2, logdet = np.empty_like(R), np.empty(self.n), np.empty((nf, k)), np.empty(nf)
        rc = self._lib.gsum_loo_folds(self._handle(), _i64(fold_ptr), _i64(fold_idx), nf, _d(R), k, _d(resid), _d(var), _d(md2), _d(logdet))
        if rc:
            msg = self._lib.gsum_loo_last_error().decode()
            if "does not factor" in msg:
                raise np.linalg.LinAlgError(msg)
            raise ValueError(msg)
        return resid, var, md2, logdet

    def set_fold_budget(self, nbytes):
        """The bytes one chunk of groups may take in ``folds`` (0: what the device has free)."""
        _check(self._lib, self._lib.gsum_loo_fold_budget(self._handle(), int(nbytes)))

    def fold_times(self, reset=False):
        """Device milliseconds spent so far in ``folds`` and ``precision_block``, by phase (FOLD_PHASES)."""
        return self._phase_times("gsum_loo_fold_times", FOLD_PHASES, reset)
