"""Python facade over the _proclife extension (native container lifecycle:
spawn / reap / directory teardown, csrc/proclife_core.h)."""
from __future__ import annotations

import importlib.util
import os
from typing import Dict, Optional, Sequence

# GDA_NATIVE_LIFECYCLE=0 forces the pure-Python lifecycle path everywhere
# (read once, at import), so both paths stay testable
ENABLED = os.environ.get("GDA_NATIVE_LIFECYCLE", "1").strip().lower() not in (
    "0", "false", "no", "off",
)

_ext = None
_ext_err: Optional[str] = None
_base_env: Optional[Dict[str, str]] = None  # the mapping the module was last given


def _load():
    global _ext, _ext_err
    if _ext is not None:
        return _ext
    if _ext_err is not None:
        raise ImportError(_ext_err)
    so = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_proclife.so")
    if not os.path.exists(so):
        _ext_err = f"{so} not built (run ops.build)"
        raise ImportError(_ext_err)
    try:
        spec = importlib.util.spec_from_file_location("_proclife", so)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    except Exception as e:  # noqa: BLE001 — stale ABI, missing symbol, ...
        _ext_err = f"{so} failed to load: {e}"
        raise ImportError(_ext_err) from e
    _ext = mod
    return mod


def available() -> bool:
    try:
        _load()
        return True
    except ImportError:
        return False


def load_error() -> Optional[str]:
    """Why the extension did not load (None when it did)."""
    return None if available() else _ext_err


def enabled() -> bool:
    """True when the lifecycle should run natively: the extension loads and
    the GDA_NATIVE_LIFECYCLE switch does not force the fallback."""
    return ENABLED and available()


def set_base_env(env: Dict[str, str]) -> int:
    """Snapshot ``env`` as the base every later spawn starts from (encoded
    once, natively). Returns the number of variables kept."""
    global _base_env
    n = _load().set_base_env(env)
    _base_env = env
    return n


def base_env_is(env: Dict[str, str]) -> bool:
    """True when ``env`` (the same object) is the snapshot in effect."""
    return _base_env is env


def spawn(argv: Sequence[str], cwd: str, env_overrides: Dict[str, str], log_path: str):
    """Start ``argv`` as a fresh session leader in ``cwd`` with stdout and
    stderr appended to ``log_path`` and base env + ``env_overrides`` as its
    environment. Returns a Child (pid, starttime, poll(), returncode,
    fileno(), close()). The base env defaults to os.environ at first use."""
    if _base_env is None:
        set_base_env(dict(os.environ))
    return _load().spawn(list(argv), cwd, env_overrides, log_path)


def remove_tree(path: str) -> int:
    """shutil.rmtree(path, ignore_errors=True); returns how many entries
    could not be removed."""
    return _load().remove_tree(path)


def prepare_container_dir(cdir: str, spec_json: str) -> None:
    _load().prepare_container_dir(cdir, spec_json)


def write_file(path: str, data) -> None:
    _load().write_file(path, data)


def proc_starttime(pid: int) -> int:
    return _load().proc_starttime(pid)
