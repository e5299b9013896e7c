"""The one place that resolves ``backend=`` / $GSUM_BACKEND and ``device=`` / $GSUM_DEVICE / $LOCAL_RANK."""
from __future__ import annotations

import os


def resolve_backend(backend):
    """'hip' or 'cpu': the argument, else $GSUM_BACKEND, else 'hip'."""
    backend = backend if backend is not None else os.environ.get("GSUM_BACKEND", "hip")
    if backend not in ("hip", "cpu"):
        raise ValueError("backend must be 'hip' or 'cpu'")
    return backend


def resolve_device(device):
    """The device index: the argument, else $GSUM_DEVICE, else $LOCAL_RANK, else 0."""
    if device is None:
        device = os.environ.get("GSUM_DEVICE", os.environ.get("LOCAL_RANK", "0"))
    return int(device)
