"""ctypes binding of libgsum_toep.so (C ABI: include/gsum_toep.h), the library of the Toeplitz likelihood path."""
from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np

from . import _sidelib
from ._sidelib import DeviceHandle, _d, _i32

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgsum_toep.so")

_p = C.c_void_p
_dp = C.POINTER(C.c_double)
PROTOTYPES = {
    "gsum_toep_last_error": (C.c_char_p, []),
    "gsum_toep_open": (C.c_int, [C.c_int32, C.POINTER(_p)]),
    "gsum_toep_close": (None, [_p]),
    "gsum_toep_max_n": (C.c_int64, [_p]),
    "gsum_toep_gram": (C.c_int, [_p, _dp, C.c_int64, C.c_int64, _dp, C.c_int64, C.c_int32, _dp, _dp, C.POINTER(C.c_int32)]),
    "gsum_toep_times": (C.c_int, [_p, _dp, C.c_int32]),
    "gsum_toep_grad": (C.c_int, [_p, _dp, C.c_int64, C.c_int64, _dp, C.c_int64, _dp, C.c_int64, C.c_int32, _dp, _dp, C.POINTER(C.c_int32), _dp,
                                 _dp]),
    "gsum_toep_solve": (C.c_int, [_p, _dp, C.c_int64, C.c_int64, _dp, C.c_int64, _dp, _dp, C.POINTER(C.c_int32)]),
    "gsum_toep_grad_times": (C.c_int, [_p, _dp, C.c_int32]),
    "gsum_toep_predict": (C.c_int, [_p, _dp, C.c_int64, _dp, C.c_int64, _dp, C.c_int32, _dp, _dp, _dp, _dp, _dp, C.POINTER(C.c_int32)]),
    "gsum_toep_loo": (C.c_int, [_p, _dp, C.c_int64, C.c_int64, _dp, C.c_int64, _dp, _dp, C.POINTER(C.c_int32)]),
    "gsum_toep_post_times": (C.c_int, [_p, _dp, C.c_int32]),
    "gsum_toep_panel_width": (C.c_int32, [_p]),
    "gsum_toep_gram_panel": (C.c_int, [_p, _dp, C.c_int64, C.c_int64, _dp, C.c_int64, C.c_int32, _dp, _dp, C.POINTER(C.c_int32)]),
    "gsum_toep_predict_panel": (C.c_int, [_p, _dp, C.c_int64, _dp, C.c_int64, _dp, C.c_int32, _dp, _dp, _dp, _dp, _dp, C.POINTER(C.c_int32)]),
    "gsum_toep_panel_times": (C.c_int, [_p, _dp, C.c_int32]),
    "gsum_toep_blocked_max_n": (C.c_int64, [_p]),
    "gsum_toep_blocked_tile_rows": (C.c_int32, [_p]),
    "gsum_toep_gram_blocked": (C.c_int, [_p, _dp, C.c_int64, C.c_int64, _dp, C.c_int64, C.c_int32, _dp, _dp, C.POINTER(C.c_int32)]),
    "gsum_toep_predict_blocked": (C.c_int, [_p, _dp, C.c_int64, _dp, C.c_int64, _dp, C.c_int32, _dp, _dp, _dp, _dp, _dp, C.POINTER(C.c_int32)]),
    "gsum_toep_blocked_times": (C.c_int, [_p, _dp, C.c_int32]),
    "gsum_toep_grad_blocked": (C.c_int, [_p, _dp, C.c_int64, C.c_int64, _dp, C.c_int64, _dp, C.c_int64, C.c_int32, _dp, _dp, C.POINTER(C.c_int32),
                                         _dp, _dp]),
    "gsum_toep_solve_blocked": (C.c_int, [_p, _dp, C.c_int64, C.c_int64, _dp, C.c_int64, _dp, _dp, C.POINTER(C.c_int32)]),
    "gsum_toep_loo_blocked": (C.c_int, [_p, _dp, C.c_int64, C.c_int64, _dp, C.c_int64, _dp, _dp, C.POINTER(C.c_int32)]),
    "gsum_toep_levinson_times": (C.c_int, [_p, _dp, C.c_int32]),
}
PHASES = ("h2d", "schur", "gram", "d2h")
GRAD_PHASES = ("h2d", "schur", "levinson", "gram", "diagsums", "solve", "contract", "d2h")    # of grad and solve (gsum_toep_grad_times)
POST_PHASES = ("h2d", "schur", "levinson", "sums", "cov", "solve", "d2h")                     # of predict and loo (gsum_toep_post_times)
PANEL_PHASES = ("h2d", "recursion", "diag", "update", "sums", "cov", "d2h")                     # of the panel route (gsum_toep_panel_times)
BLOCKED_PHASES = ("h2d", "lead", "tiles", "diag", "update", "sums", "cov", "d2h")               # of the blocked route (gsum_toep_blocked_times)
# of grad, solve and loo with method="blocked" (gsum_toep_levinson_times)
LEVINSON_PHASES = ("h2d", "lead", "tiles", "diag", "update", "levinson", "gram", "diagsums", "solve", "contract", "d2h")
METHODS = ("columns", "panel", "blocked")                              # the device schedules of gram and predict
GRAD_METHODS = ("columns", "blocked")                                  # ... of grad, solve and loo
_GRAD = {"columns": "gsum_toep_grad", "blocked": "gsum_toep_grad_blocked"}
_SOLVE = {"columns": "gsum_toep_solve", "blocked": "gsum_toep_solve_blocked"}
_LOO = {"columns": "gsum_toep_loo", "blocked": "gsum_toep_loo_blocked"}
_GRAM = {"columns": "gsum_toep_gram", "panel": "gsum_toep_gram_panel", "blocked": "gsum_toep_gram_blocked"}
_PREDICT = {"columns": "gsum_toep_predict", "panel": "gsum_toep_predict_panel", "blocked": "gsum_toep_predict_blocked"}
MAX_COLS = 16                                                          # GSUM_TOEP_MAX_COLS


def load_library(path: str | None = None):
    """dlopen libgsum_toep.so and attach the prototypes.  Raises if it is absent (``python -m gsum_amd.build`` builds it)."""
    return _sidelib.load(LIB_PATH, PROTOTYPES, path)


def _check(lib, rc):
    _sidelib.check(lib, rc, "gsum_toep_last_error")


def max_n(method="columns"):
    """The largest n ``DeviceToeplitz.gram`` takes with ``method`` (needs no device)."""
    lib = load_library()
    return int(lib.gsum_toep_blocked_max_n(None) if check_method(method) == "blocked" else lib.gsum_toep_max_n(None))


def panel_width():
    """The columns of L per panel on the panel route (needs no device)."""
    return int(load_library().gsum_toep_panel_width(None))


def blocked_tile_rows():
    """The rows a tile of the blocked route owns (needs no device)."""
    return int(load_library().gsum_toep_blocked_tile_rows(None))


def check_method(method, name="method"):
    """The one check of ``method=`` / ``toeplitz_method=`` (``name``).  The keyword selects a device schedule, not an arithmetic:
    ``backend='cpu'`` accepts every value and runs its one code."""
    if not isinstance(method, str) or method not in METHODS:
        raise ValueError(f'{name} must be "columns" or "panel" or "blocked", got {method!r}')
    return method


def check_grad_method(method, name="method"):
    """``check_method`` for what works from x = T^-1 e_0 (``toeplitz_grad``, ``toeplitz_solve``, ``toeplitz_loo`` and their kin), which
    has no panel route: ``name`` is ``method`` or ``toeplitz_grad_method``."""
    if not isinstance(method, str) or method not in GRAD_METHODS:
        raise ValueError(f'{name} must be "columns" or "blocked", got {method!r}')
    return method


class DeviceToeplitz(DeviceHandle):
    """A handle of libgsum_toep.so on one device: its stream and its buffers, which grow with the calls."""

    _free = "gsum_toep_close"
    _last_error = "gsum_toep_last_error"

    def __init__(self, device):
        self._lib = lib = load_library()
        self._lock = threading.Lock()                                  # one call at a time: the buffers belong to the handle
        h = C.c_void_p()
        _check(lib, lib.gsum_toep_open(int(device), C.byref(h)))
        self._h = h

    def _handle(self):
        if self._h is None:
            raise ValueError("the handle is closed")
        return self._h

    def gram(self, t, Z, n_sets, method="columns"):
        """(G (m, n_sets, c, c), sum_log_diag (m,), info (m,) int32) of the first columns t (m, n) and the right-hand sides Z
        (n, n_sets * c): gsum_toep_gram, gsum_toep_gram_panel with ``method="panel"`` or gsum_toep_gram_blocked with ``"blocked"``."""
        fn = getattr(self._lib, _GRAM[check_method(method)])
        t = np.ascontiguousarray(t, dtype=np.float64)
        Zf = np.asfortranarray(Z, dtype=np.float64)
        m, n = t.shape
        cols = Zf.shape[1] // n_sets
        G = np.empty((m, n_sets, cols, cols))
        sld = np.empty(m)
        info = np.empty(m, dtype=np.int32)
        with self._lock:
            _check(self._lib, fn(self._handle(), _d(t), m, n, _d(Zf), n_sets, cols, _d(G), _d(sld), _i32(info)))
        return G, sld, info

    def grad(self, t, dt, Z, n_sets, method="columns"):
        """(G, sum_log_diag, info, trace (m, P), H (m, n_sets, P, c, c)) of the first columns t (m, n), their derivative columns dt
        (m, P, n) and the right-hand sides Z (n, n_sets * c): gsum_toep_grad, or gsum_toep_grad_blocked with ``method="blocked"``."""
        fn = getattr(self._lib, _GRAD[check_grad_method(method)])
        t = np.ascontiguousarray(t, dtype=np.float64)
        dt = np.ascontiguousarray(dt, dtype=np.float64)
        Zf = np.asfortranarray(Z, dtype=np.float64)
        m, n = t.shape
        P = dt.shape[1]
        cols = Zf.shape[1] // n_sets
        G = np.empty((m, n_sets, cols, cols))
        H = np.empty((m, n_sets, P, cols, cols))
        trace = np.empty((m, P))
        sld = np.empty(m)
        info = np.empty(m, dtype=np.int32)
        with self._lock:
            _check(self._lib, fn(self._handle(), _d(t), m, n, _d(dt), P, _d(Zf), n_sets, cols, _d(G), _d(sld), _i32(info), _d(trace), _d(H)))
        return G, sld, info, trace, H

    def solve(self, t, Z, want_x=True, method="columns"):
        """(x (m, n) or None, alpha (m, n, c) or None, info): the first column of the inverse and T^-1 Z (Z None: x alone):
        gsum_toep_solve, or gsum_toep_solve_blocked with ``method="blocked"``."""
        fn = getattr(self._lib, _SOLVE[check_grad_method(method)])
        t = np.ascontiguousarray(t, dtype=np.float64)
        m, n = t.shape
        x = np.empty((m, n)) if want_x else None
        Zf = alpha = None
        ncols = 0
        if Z is not None:
            Zf = np.asfortranarray(Z, dtype=np.float64)
            ncols = Zf.shape[1]
            alpha = np.empty((m, n, ncols))
        info = np.empty(m, dtype=np.int32)
        with self._lock:
            _check(self._lib, fn(self._handle(), _d(t), m, n, None if Zf is None else _d(Zf), ncols, None if x is None else _d(x),
                                 None if alpha is None else _d(alpha), _i32(info)))
        return x, alpha, info

    def predict(self, t, K, Z, want_cov, method="columns"):
        """(quad (q,), cross (q, c), cov (q, q) or None, G (c, c), sum_log_diag, info) of one first column t (n,), the cross-covariance
        columns K (n, q) and the residual columns Z (n, c), c >= 0: gsum_toep_predict, gsum_toep_predict_panel with
        ``method="panel"`` or gsum_toep_predict_blocked with ``"blocked"``."""
        fn = getattr(self._lib, _PREDICT[check_method(method)])
        t = np.ascontiguousarray(t, dtype=np.float64)
        Kf = np.asfortranarray(K, dtype=np.float64)
        Zf = np.asfortranarray(Z, dtype=np.float64)
        n, q, c = t.shape[0], Kf.shape[1], Zf.shape[1]
        quad, cross, G = np.empty(q), np.empty((q, c)), np.empty((c, c))
        cov = np.empty((q, q)) if want_cov else None
        sld = np.empty(1)
        info = np.empty(1, dtype=np.int32)
        with self._lock:
            _check(self._lib, fn(self._handle(), _d(t), n, _d(Kf), q, _d(Zf) if c else None, c, _d(quad), _d(cross) if c else None,
                                 None if cov is None else _d(cov), _d(G) if c else None, _d(sld), _i32(info)))
        return quad, cross, cov, G, float(sld[0]), int(info[0])

    def loo(self, t, Z, method="columns"):
        """(p (m, n), alpha (m, n, c) or None, info): the diagonal of the inverse and T^-1 Z (Z None: p alone): gsum_toep_loo, or
        gsum_toep_loo_blocked with ``method="blocked"``."""
        fn = getattr(self._lib, _LOO[check_grad_method(method)])
        t = np.ascontiguousarray(t, dtype=np.float64)
        m, n = t.shape
        p = np.empty((m, n))
        Zf = alpha = None
        ncols = 0
        if Z is not None:
            Zf = np.asfortranarray(Z, dtype=np.float64)
            ncols = Zf.shape[1]
            alpha = np.empty((m, n, ncols))
        info = np.empty(m, dtype=np.int32)
        with self._lock:
            _check(self._lib, fn(self._handle(), _d(t), m, n, None if Zf is None else _d(Zf), ncols, _d(p), None if alpha is None else _d(alpha),
                                 _i32(info)))
        return p, alpha, info

    def levinson_times(self, reset=False):
        """Device milliseconds spent so far by ``grad``, ``solve`` and ``loo`` with ``method="blocked"``, by phase (LEVINSON_PHASES)."""
        return self._phase_times("gsum_toep_levinson_times", LEVINSON_PHASES, reset)

    def blocked_times(self, reset=False):
        """Device milliseconds spent so far by ``gram`` and ``predict`` with ``method="blocked"``, by phase (BLOCKED_PHASES)."""
        return self._phase_times("gsum_toep_blocked_times", BLOCKED_PHASES, reset)

    def panel_times(self, reset=False):
        """Device milliseconds spent so far by ``gram`` and ``predict`` with ``method="panel"``, by phase (PANEL_PHASES)."""
        return self._phase_times("gsum_toep_panel_times", PANEL_PHASES, reset)

    def post_times(self, reset=False):
        """Device milliseconds spent so far by ``predict`` and ``loo``, by phase (POST_PHASES)."""
        return self._phase_times("gsum_toep_post_times", POST_PHASES, reset)

    def grad_times(self, reset=False):
        """Device milliseconds spent so far by ``grad`` and ``solve``, by phase (GRAD_PHASES)."""
        return self._phase_times("gsum_toep_grad_times", GRAD_PHASES, reset)

    def times(self, reset=False):
        """Device milliseconds (HIP events) spent so far, by phase (PHASES)."""
        return self._phase_times("gsum_toep_times", PHASES, reset)


_handles = {}
_handles_lock = threading.Lock()


def default_handle(device):
    """The process's one handle per device, opened on first use."""
    with _handles_lock:
        if device not in _handles:
            _handles[device] = DeviceToeplitz(device)
        return _handles[device]
