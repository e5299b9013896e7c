"""ctypes binding of libgsum_vario.so (C ABI: include/gsum_vario.h), the variogram's own library."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _sidelib
from ._sidelib import DeviceHandle, _d, _i32, _i64

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgsum_vario.so")

_p = C.c_void_p
_dp = C.POINTER(C.c_double)
PROTOTYPES = {
    "gsum_vario_last_error": (C.c_char_p, []),
    "gsum_vario_create": (C.c_int, [C.c_int32, _dp, C.c_int64, C.c_int32, _dp, C.c_int32, _dp, C.c_int32, C.POINTER(_p),
                                    C.POINTER(C.c_int64), _dp, _dp]),
    "gsum_vario_cov": (C.c_int, [_p, _dp, C.c_double, C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32, _dp]),
    "gsum_vario_corr": (C.c_int, [C.c_int32, _dp, C.c_int64, C.c_double, _dp]),
    "gsum_vario_free": (None, [_p]),
}


def load_library(path: str | None = None):
    """dlopen libgsum_vario.so and attach the prototypes.  Raises if it is absent (``python -m gsum_amd.build`` builds it)."""
    return _sidelib.load(LIB_PATH, PROTOTYPES, path)


def _check(lib, rc):
    _sidelib.check(lib, rc, "gsum_vario_last_error")


class DeviceVariogram(DeviceHandle):
    """The device object of one (X, z, bounds): the pair stage runs in the constructor; ``counts``, ``h_sum`` (Nb,) and ``dij_sum``
    (Nb, n_curves) are its per-bin integer counts and sums."""

    _free = "gsum_vario_free"

    def __init__(self, device, X, Z, bounds):
        self._lib = lib = load_library()
        X = np.ascontiguousarray(X, dtype=np.float64)
        Z = np.ascontiguousarray(Z, dtype=np.float64)
        bounds = np.ascontiguousarray(bounds, dtype=np.float64)
        n, d = X.shape
        nc = Z.shape[0]
        nb = bounds.shape[0] + 1
        self.counts = np.zeros(nb, dtype=np.int64)
        self.h_sum = np.zeros(nb)
        self.dij_sum = np.zeros((nb, nc))
        self.n_curves = nc
        h = C.c_void_p()
        _check(lib, lib.gsum_vario_create(int(device), _d(X), n, d, _d(Z), nc, _d(bounds), bounds.shape[0], C.byref(h),
                                          _i64(self.counts), _d(self.h_sum), _d(self.dij_sum)))
        self._h = h

    def cov_sums(self, gamma_tilde, var_factor, corr_factor, bin1, bin2):
        """Undivided sums of cov_ijkl over the pairs of bin1[r] x bin2[r], shape (len(bin1), n_curves)."""
        if self._h is None:
            raise ValueError("the variogram is closed")
        gt = np.ascontiguousarray(gamma_tilde, dtype=np.float64)
        b1 = np.ascontiguousarray(bin1, dtype=np.int32)
        b2 = np.ascontiguousarray(bin2, dtype=np.int32)
        out = np.zeros((b1.shape[0], self.n_curves))
        _check(self._lib, self._lib.gsum_vario_cov(self._h, _d(gt), float(var_factor), float(corr_factor), _i32(b1), _i32(b2),
                                                   b1.shape[0], _d(out)))
        return out


def device_corr(rho, corr_factor, device=0):
    """The device's correlation map corr(rho), elementwise (gsum_vario_corr)."""
    lib = load_library()
    rho = np.ascontiguousarray(rho, dtype=np.float64).ravel()
    out = np.empty_like(rho)
    _check(lib, lib.gsum_vario_corr(int(device), _d(rho), rho.shape[0], float(corr_factor), _d(out)))
    return out
