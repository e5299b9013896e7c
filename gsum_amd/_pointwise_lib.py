"""ctypes binding of libgsum_pointwise.so (C ABI: include/gsum_pointwise.h), TruncationPointwise's own library."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _sidelib
from ._sidelib import DeviceHandle, _d, _i32, _i64

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgsum_pointwise.so")

_p = C.c_void_p
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
PROTOTYPES = {
    "gsum_pointwise_last_error": (C.c_char_p, []),
    "gsum_pointwise_create": (C.c_int, [C.c_int32, _dp, _ip, _ip, C.c_int64, C.c_int32, C.POINTER(_p)]),
    "gsum_pointwise_loglike_grid": (C.c_int, [_p, _dp, C.c_int32, _dp, C.c_int32, C.c_int64, C.c_double, C.c_double, _dp]),
    "gsum_pointwise_coverage": (C.c_int, [_p, _dp, _dp, _dp, C.c_int32, _dp, _dp, C.c_int32, C.POINTER(C.c_int64)]),
    "gsum_pointwise_times": (C.c_int, [_p, _dp, C.c_int32]),
    "gsum_pointwise_free": (None, [_p]),
}
PHASES = ("h2d", "differences", "loglike", "coverage", "d2h")
MAX_ORDERS = 64                                                        # GSUM_POINTWISE_MAX_ORDERS
REF_SCALAR, REF_POINTS, REF_ROW_SCALAR, REF_ROW_POINTS = range(4)      # GSUM_POINTWISE_REF_*


def load_library(path: str | None = None):
    """dlopen libgsum_pointwise.so and attach the prototypes.  Raises if it is absent (``python -m gsum_amd.build`` builds it)."""
    return _sidelib.load(LIB_PATH, PROTOTYPES, path)


def _check(lib, rc):
    _sidelib.check(lib, rc, "gsum_pointwise_last_error")


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class DevicePointwise(DeviceHandle):
    """The first differences of the kept orders of y (n x k) resident on the device (uploaded once) and the operations of
    include/gsum_pointwise.h on them.  ``orders`` are integers, ``mask`` flags the orders that are kept."""

    _free = "gsum_pointwise_free"
    _last_error = "gsum_pointwise_last_error"

    def __init__(self, device, y, orders, mask):
        self._lib = lib = load_library()
        y = _f64(y)
        if y.ndim != 2:
            raise ValueError(f"y must be 2-D, got shape {y.shape}")
        orders = np.ascontiguousarray(orders, dtype=np.int32).ravel()
        mask = np.ascontiguousarray(mask, dtype=np.int32).ravel()
        self.n, self.k = y.shape
        if orders.shape[0] != self.k or mask.shape[0] != self.k:
            raise ValueError(f"orders and mask must have one entry per column of y ({self.k})")
        self.kp = int(np.count_nonzero(mask))
        h = C.c_void_p()
        _check(lib, lib.gsum_pointwise_create(int(device), _d(y), _i32(orders), _i32(mask), self.n, self.k, C.byref(h)))
        self._h = h

    def _handle(self):
        if self._h is None:
            raise ValueError("the device data are freed")
        return self._h

    def loglike_grid(self, ratios, refs, ref_mode, df0, scale0):
        """(G,): minus the ratio- and ref-dependent part of the log likelihood of every row.  ratios (G,) or (G, n); refs as
        ``ref_mode`` says: REF_SCALAR (1,), REF_POINTS (n,), REF_ROW_SCALAR (G,), REF_ROW_POINTS (G, n)."""
        ratios, refs = _f64(ratios), _f64(refs)
        G = ratios.shape[0]
        if ratios.shape not in ((G,), (G, self.n)) or G < 1:
            raise ValueError(f"ratios must be (G,) or (G, {self.n}), got {ratios.shape}")
        want = {REF_SCALAR: (1,), REF_POINTS: (self.n,), REF_ROW_SCALAR: (G,), REF_ROW_POINTS: (G, self.n)}
        if ref_mode not in want or refs.shape != want[ref_mode]:
            raise ValueError(f"refs of mode {ref_mode} must have shape {want.get(ref_mode)}, got {refs.shape}")
        out = np.empty(G)
        _check(self._lib, self._lib.gsum_pointwise_loglike_grid(self._handle(), _d(ratios), int(ratios.ndim == 2), _d(refs), int(ref_mode), G,
                                                                float(df0), float(scale0), _d(out)))
        return out

    def coverage(self, loc, scale, data, t_lo, t_hi):
        """int64 counts (D, kp) of the points with ``t_lo[d] * scale + loc < data < t_hi[d] * scale + loc`` (loc, scale: (n, kp);
        data: (n, kp) or (n, 1))."""
        loc, scale, data = _f64(loc), _f64(scale), _f64(data)
        t_lo, t_hi = _f64(t_lo).ravel(), _f64(t_hi).ravel()
        if loc.shape != (self.n, self.kp) or scale.shape != loc.shape:
            raise ValueError(f"loc and scale must both be ({self.n}, {self.kp}), got {loc.shape} and {scale.shape}")
        if data.shape not in ((self.n, 1), (self.n, self.kp)):
            raise ValueError(f"data must be ({self.n}, 1) or ({self.n}, {self.kp}), got {data.shape}")
        if t_lo.shape != t_hi.shape or t_lo.shape[0] < 1:
            raise ValueError("t_lo and t_hi must be non-empty and of one length")
        D = t_lo.shape[0]
        counts = np.zeros((D, self.kp), dtype=np.int64)
        _check(self._lib, self._lib.gsum_pointwise_coverage(self._handle(), _d(loc), _d(scale), _d(data), data.shape[1], _d(t_lo), _d(t_hi), D,
                                                            _i64(counts)))
        return counts

    def times(self, reset=False):
        """Device milliseconds (HIP events) spent so far, by phase (PHASES)."""
        return self._phase_times("gsum_pointwise_times", PHASES, reset)
