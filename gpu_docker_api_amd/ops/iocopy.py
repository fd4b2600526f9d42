"""Python facade over the _iocopy extension (io_uring copy engine)."""
from __future__ import annotations

import importlib.util
import os
from typing import Optional

_ext = None
_ext_err: Optional[str] = None


def _load():
    global _ext, _ext_err
    if _ext is not None:
        return _ext
    if _ext_err is not None:
        raise ImportError(_ext_err)
    so = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_iocopy.so")
    if not os.path.exists(so):
        _ext_err = f"{so} not built (run ops.build)"
        raise ImportError(_ext_err)
    spec = importlib.util.spec_from_file_location("_iocopy", so)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    _ext = mod
    return mod


def copy_tree(src, dst, *, use_uring: bool = True, use_copy_file_range: bool = True) -> dict:
    """Copy the tree under ``src`` into ``dst`` (str or bytes paths).

    The engine picks its data path per file: the io_uring batch for small
    files, a copy_file_range loop for large or sparse ones, pread/pwrite
    where the kernel refuses copy_file_range. ``use_uring=False`` sends small
    files through the per-file path as well, ``use_copy_file_range=False``
    forces the pread/pwrite bounce."""
    return _load().copy_tree(
        src, dst, use_uring=use_uring, use_copy_file_range=use_copy_file_range
    )


def uring_available() -> bool:
    try:
        return bool(_load().uring_available())
    except ImportError:
        return False
