"""ctypes binding of libgsum_band.so (C ABI: include/gsum_band.h), the library of the banded likelihood path."""
from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np

from . import _sidelib
from ._lib import KernelDesc
from ._sidelib import DeviceHandle, _d, _i32

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgsum_band.so")

_p = C.c_void_p
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_kp = C.POINTER(KernelDesc)
PROTOTYPES = {
    "gsum_band_last_error": (C.c_char_p, []),
    "gsum_band_open": (C.c_int, [C.c_int32, C.POINTER(_p)]),
    "gsum_band_close": (None, [_p]),
    "gsum_band_max_halfwidth": (C.c_int32, [_p]),
    "gsum_band_block": (C.c_int32, [_p]),
    "gsum_band_set_chunk": (C.c_int, [_p, C.c_int64]),
    "gsum_band_width": (C.c_int, [_p, _kp, C.c_int64, _dp, C.c_int64, C.c_double, _ip]),
    "gsum_band_build": (C.c_int, [_p, _kp, C.c_int64, _dp, C.c_int64, C.c_double, C.c_int32, _dp]),
    "gsum_band_gram": (C.c_int, [_p, _dp, C.c_int64, C.c_int64, C.c_int32, _dp, C.c_int64, C.c_int32, _dp, _dp, _ip, _dp]),
    "gsum_band_forward": (C.c_int, [_p, _dp, C.c_int64, C.c_int64, C.c_int32, _dp, C.c_int64, _dp]),
    "gsum_band_times": (C.c_int, [_p, _dp, C.c_int32]),
}
PHASES = ("h2d", "build", "factor", "forward", "gram", "d2h")
MAX_COLS = 16                                                          # GSUM_BAND_MAX_COLS


def load_library(path: str | None = None):
    """dlopen libgsum_band.so and attach the prototypes.  Raises if it is absent (``python -m gsum_amd.build`` builds it)."""
    return _sidelib.load(LIB_PATH, PROTOTYPES, path)


def _check(lib, rc):
    _sidelib.check(lib, rc, "gsum_band_last_error")


def max_halfwidth():
    """The widest half-bandwidth the library takes (needs no device)."""
    return int(load_library().gsum_band_max_halfwidth(None))


def block():
    """The columns the factorisation advances per step (needs no device)."""
    return int(load_library().gsum_band_block(None))


def desc_array(descs):
    """The descriptors as one ctypes array (a copy)."""
    arr = (KernelDesc * len(descs))()
    for i, d in enumerate(descs):
        C.memmove(C.byref(arr[i]), C.byref(d), C.sizeof(KernelDesc))
    return arr


class DeviceBand(DeviceHandle):
    """A handle of libgsum_band.so on one device: its stream and its buffers, which grow with the calls."""

    _free = "gsum_band_close"
    _last_error = "gsum_band_last_error"

    def __init__(self, device):
        self._lib = lib = load_library()
        self._lock = threading.RLock()                                 # one call at a time: the buffers belong to the handle
        h = C.c_void_p()
        _check(lib, lib.gsum_band_open(int(device), C.byref(h)))
        self._h = h

    def _handle(self):
        if self._h is None:
            raise ValueError("the handle is closed")
        return self._h

    def set_chunk(self, max_elements):
        """The doubles a launch chunk's bands, and its solved columns, may hold (0: the default)."""
        with self._lock:
            _check(self._lib, self._lib.gsum_band_set_chunk(self._handle(), int(max_elements)))

    def width(self, descs, X, nugget=0.0):
        """width (m,) int32 of the descriptors on the points X (n,): gsum_band_width."""
        X = np.ascontiguousarray(X, dtype=np.float64).ravel()
        out = np.empty(len(descs), dtype=np.int32)
        with self._lock:
            _check(self._lib, self._lib.gsum_band_width(self._handle(), desc_array(descs), len(descs), _d(X), X.size, float(nugget), _i32(out)))
        return out

    def build(self, descs, X, nugget, b, to_host=True):
        """AB (m, b + 1, n) of the descriptors, kept on the device as well (``to_host=False``: there only, None returned)."""
        X = np.ascontiguousarray(X, dtype=np.float64).ravel()
        m = len(descs)
        AB = np.empty((m, int(b) + 1, X.size)) if to_host else None
        with self._lock:
            _check(self._lib, self._lib.gsum_band_build(self._handle(), desc_array(descs), m, _d(X), X.size, float(nugget), int(b), _d(AB)))
        return AB

    def gram(self, AB, Z, n_sets, shape=None, want_factor=False):
        """(G (m, n_sets, c, c), sum_log_diag (m,), info (m,) int32, L or None) of the bands AB (m, b + 1, n) -- None: the bands the last
        ``build`` left on the device, ``shape`` = (m, b + 1, n) -- and the right-hand sides Z (n, n_sets * c): gsum_band_gram."""
        if AB is not None:
            AB = np.ascontiguousarray(AB, dtype=np.float64)
            shape = AB.shape
        m, b1, n = shape
        Zf = np.asfortranarray(Z, dtype=np.float64)
        cols = Zf.shape[1] // n_sets
        G = np.empty((m, n_sets, cols, cols))
        sld = np.empty(m)
        info = np.empty(m, dtype=np.int32)
        L = np.empty((m, b1, n)) if want_factor else None
        with self._lock:
            _check(self._lib, self._lib.gsum_band_gram(self._handle(), _d(AB), m, n, b1 - 1, _d(Zf), n_sets, cols, _d(G), _d(sld), _i32(info), _d(L)))
        return G, sld, info, L

    def build_gram(self, descs, X, nugget, b, Z, n_sets):
        """``build`` on the device alone, then ``gram`` of what it left there: no band crosses the bus."""
        with self._lock:
            self.build(descs, X, nugget, b, to_host=False)
            return self.gram(None, Z, n_sets, shape=(len(descs), int(b) + 1, np.size(X)))[:3]

    def forward(self, L, Z):
        """Y (m, n, ncols) = L^-1 Z of the factors L (m, b + 1, n) and the columns Z (n, ncols): gsum_band_forward."""
        L = np.ascontiguousarray(L, dtype=np.float64)
        Zf = np.asfortranarray(Z, dtype=np.float64)
        m, b1, n = L.shape
        ncols = Zf.shape[1]
        Y = np.empty((m, ncols, n))
        with self._lock:
            _check(self._lib, self._lib.gsum_band_forward(self._handle(), _d(L), m, n, b1 - 1, _d(Zf), ncols, _d(Y)))
        return np.ascontiguousarray(Y.transpose(0, 2, 1))

    def times(self, reset=False):
        """Device milliseconds (HIP events) spent so far, by phase (PHASES)."""
        return self._phase_times("gsum_band_times", PHASES, reset)


_handles = {}
_handles_lock = threading.Lock()


def default_handle(device):
    """The process's one handle per device, opened on first use."""
    with _handles_lock:
        if device not in _handles:
            _handles[device] = DeviceBand(device)
        return _handles[device]
