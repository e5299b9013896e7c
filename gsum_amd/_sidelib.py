"""What the ctypes bindings of the side libraries share (_vario_lib.py, _refdist_lib.py, _pointwise_lib.py, _loo_lib.py, _toep_lib.py;
the C++ side of it is csrc/host/sidelib.hip.h): the prototype-attaching loader, the pointer helpers, the return-code check and the
owner of a device handle, with the read-out of its phase clock."""
from __future__ import annotations

import ctypes as C
import os
import threading

_dp = C.POINTER(C.c_double)
_libs = {}                    # default path -> CDLL
_lock = threading.Lock()      # HipGroup.map runs host threads


def attach(lib, prototypes):
    """Set restype / argtypes of every prototype on the CDLL; AttributeError if a symbol is missing."""
    for name, (res, args) in prototypes.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def load(default_path, prototypes, path=None):
    """dlopen ``path`` (not cached) or ``default_path`` (once per process) and attach the prototypes.  Raises if the file is absent."""
    with _lock:
        if path is None and default_path in _libs:
            return _libs[default_path]
        p = path or default_path
        if not os.path.exists(p):
            raise RuntimeError(f"{p} is missing: build it with `python -m gsum_amd.build`")
        lib = attach(C.CDLL(p), prototypes)
        if path is None:
            _libs[default_path] = lib
        return lib


def _d(a):
    return a.ctypes.data_as(_dp) if a is not None else None


def _i32(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _i64(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def check(lib, rc, last_error):
    """A non-zero return code becomes ValueError with the library's message (``last_error``: the name of <library>_last_error)."""
    if rc:
        raise ValueError(getattr(lib, last_error)().decode())


class DeviceHandle:
    """Owner of one device handle ``_h`` of the library ``_lib``, freed by ``_free`` (the name of <library>_free): ``free()`` is
    idempotent, and the context manager and ``__del__`` call it.  A library with a phase clock names its <library>_last_error in
    ``_last_error``; its binding's ``_handle()`` returns the open handle."""

    _free = None
    _last_error = None
    _h = None

    def _phase_times(self, fn_name, phases, reset):
        """{phase: device milliseconds so far} from the library's ``fn_name`` (a <library>_*_times), in the order of ``phases``."""
        ms = (C.c_double * len(phases))()
        check(self._lib, getattr(self._lib, fn_name)(self._handle(), ms, int(bool(reset))), self._last_error)
        return dict(zip(phases, ms))

    def free(self):
        if self._h is not None:
            getattr(self._lib, self._free)(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
