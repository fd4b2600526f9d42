"""Bulk data movers for rolling replacement.

The reference migrates a container's writable layer with a shell tar pipe
(``(cd src; tar c .) | (cd dest; tar x)`` — /root/reference/utils/copy.go:17-27)
and migrates volumes by spinning up a throwaway ubuntu container that runs
``mv`` inside, fire-and-forget (utils/copy.go:74-128). Here:

* the preferred engine is the native io_uring copier (csrc/iocopy_core.h →
  ops._iocopy): queued reads/writes, sparse-aware, preserves
  owner/mode/mtime/symlinks/hardlinks/xattrs (overlayfs whiteouts are device
  nodes + xattrs, which it replicates);
* the fallback is a shell-free tar pipe (two connected subprocesses with
  --xattrs --sparse) — still awaited, never fire-and-forget;
* near-empty layers are copied inline with the same fidelity; what each
  route must preserve is written down in tests/test_copy_engines.py;
* volume migration is a plain host-side move (the daemon can see both
  mountpoints; no helper container needed), also awaited.
"""
from __future__ import annotations

import asyncio
import logging
import os
import shutil
import stat
import subprocess
from typing import Optional

log = logging.getLogger(__name__)

_iocopy = None
_iocopy_err: Optional[str] = None


def _load_iocopy():
    global _iocopy, _iocopy_err
    if _iocopy is not None or _iocopy_err is not None:
        return _iocopy
    try:
        from ..ops import iocopy as mod  # noqa: WPS433

        _iocopy = mod
    except Exception as exc:  # extension not built
        _iocopy_err = str(exc)
        log.info("native iocopy unavailable (%s); using tar fallback", exc)
    return _iocopy


def _tar_supports(flag: str) -> bool:
    try:
        out = subprocess.run(["tar", "--help"], capture_output=True, text=True, timeout=10)
        return flag in out.stdout
    except Exception:
        return False


_TAR_XATTRS: Optional[bool] = None
_TAR_SPARSE: Optional[bool] = None


async def _tar_pipe_copy(src: str, dest: str) -> None:
    """tar -C src -c . | tar -C dest -x  (no shell, awaited, xattrs kept,
    holes kept where tar offers --sparse, modes kept whatever the umask)."""
    global _TAR_XATTRS, _TAR_SPARSE
    if _TAR_XATTRS is None:
        _TAR_XATTRS = _tar_supports("--xattrs")
    if _TAR_SPARSE is None:
        _TAR_SPARSE = _tar_supports("--sparse")
    extra = ["--xattrs", "--acls"] if _TAR_XATTRS else []
    sparse = ["--sparse"] if _TAR_SPARSE else []
    r_fd, w_fd = os.pipe()
    try:
        reader = await asyncio.create_subprocess_exec(
            "tar", "-C", src, *extra, *sparse, "-cf", "-", ".", stdout=w_fd
        )
    finally:
        os.close(w_fd)
    try:
        writer = await asyncio.create_subprocess_exec(
            "tar",
            "-C",
            dest,
            *(extra + ["--xattrs-include=*"] if extra else []),
            "-p",
            "-xf",
            "-",
            stdin=r_fd,
        )
    finally:
        os.close(r_fd)
    rc_w = await writer.wait()
    rc_r = await reader.wait()
    if rc_r != 0 or rc_w != 0:
        raise RuntimeError(f"tar pipe copy {src} -> {dest} failed (tar rc {rc_r}/{rc_w})")


class CopyEngine:
    """Engine selection: 'auto' (io_uring if built, else tar), 'iouring',
    'tar', 'python' (shutil; tests)."""

    def __init__(self, kind: str = "auto") -> None:
        self.kind = kind

    # trees at or below this size are copied inline: engine setup (io_uring
    # ring init / tar fork+exec / thread hop) costs ~1-2 ms, which dominates
    # the rolling-replace latency when the writable layer is near-empty
    SMALL_TREE_BYTES = 1 << 20
    SMALL_TREE_FILES = 32

    @classmethod
    def _small_tree_entries(cls, src: str):
        """Top-level regular files/symlinks totaling <= SMALL_TREE_BYTES, as
        (name, lstat) pairs, or None when the tree needs a real engine:
        subdirectories, special files, large trees, and what the inline copy
        does not carry (names of one inode, holes)."""
        entries = []
        total = 0
        try:
            with os.scandir(src) as it:
                for e in it:
                    if len(entries) >= cls.SMALL_TREE_FILES:
                        return None
                    st = e.stat(follow_symlinks=False)
                    if stat.S_ISLNK(st.st_mode):
                        entries.append((e.name, st))
                        continue
                    if not stat.S_ISREG(st.st_mode):
                        return None
                    if st.st_nlink > 1 or st.st_blocks * 512 < st.st_size:
                        return None
                    total += st.st_size
                    if total > cls.SMALL_TREE_BYTES:
                        return None
                    entries.append((e.name, st))
        except OSError:
            return None
        return entries

    @staticmethod
    def _copy_entry_inline(src: str, dest: str, st: os.stat_result) -> None:
        """One top-level file or symlink with everything the engines keep:
        content, owner, mode, mtime, xattrs. The destination entry is
        replaced, never opened or followed."""
        try:
            os.unlink(dest)
        except FileNotFoundError:
            pass
        if stat.S_ISLNK(st.st_mode):
            os.symlink(os.readlink(src), dest)
        else:
            in_fd = os.open(src, os.O_RDONLY | os.O_CLOEXEC)
            try:
                out_fd = os.open(
                    dest,
                    os.O_WRONLY | os.O_CREAT | os.O_EXCL | os.O_NOFOLLOW | os.O_CLOEXEC,
                    0o600,
                )
                try:
                    left = st.st_size
                    while left > 0:
                        chunk = os.read(in_fd, left)
                        if not chunk:
                            raise OSError(f"{src}: end of file {left} bytes early")
                        view = memoryview(chunk)
                        while view:
                            view = view[os.write(out_fd, view):]
                        left -= len(chunk)
                finally:
                    os.close(out_fd)
            finally:
                os.close(in_fd)
            for name in os.listxattr(src):
                try:
                    os.setxattr(dest, name, os.getxattr(src, name))
                except OSError:
                    pass  # best-effort, as in the native engine: security.*
        try:
            os.chown(dest, st.st_uid, st.st_gid, follow_symlinks=False)
        except OSError:
            pass  # unprivileged
        if not stat.S_ISLNK(st.st_mode):
            os.chmod(dest, stat.S_IMODE(st.st_mode))  # after the chown: keeps setuid
        os.utime(dest, ns=(st.st_atime_ns, st.st_mtime_ns), follow_symlinks=False)

    async def copy_dir(self, src: str, dest: str) -> None:
        if not os.path.isdir(src):
            raise FileNotFoundError(src)
        os.makedirs(dest, exist_ok=True)
        small = self._small_tree_entries(src)
        if small is not None:
            for name, st in small:
                self._copy_entry_inline(
                    os.path.join(src, name), os.path.join(dest, name), st
                )
            return
        kind = self.kind
        if kind == "auto":
            kind = "iouring" if _load_iocopy() is not None else "tar"
        if kind == "iouring":
            mod = _load_iocopy()
            if mod is None:
                raise RuntimeError(f"io_uring engine requested but unavailable: {_iocopy_err}")
            # run in a thread: the native engine blocks its calling thread
            await asyncio.get_running_loop().run_in_executor(
                None, mod.copy_tree, src, dest
            )
        elif kind == "tar":
            await _tar_pipe_copy(src, dest)
        elif kind == "python":
            await asyncio.get_running_loop().run_in_executor(
                None,
                lambda: shutil.copytree(src, dest, symlinks=True, dirs_exist_ok=True),
            )
        else:
            raise ValueError(f"unknown copy engine {kind!r}")

    async def move_contents(self, src: str, dest: str) -> None:
        """Move everything under src into dest (volume resize migration).
        Same-filesystem moves are renames; cross-fs falls back to copy+rm."""
        if not os.path.isdir(src):
            raise FileNotFoundError(src)
        os.makedirs(dest, exist_ok=True)

        def _move() -> None:
            for entry in os.listdir(src):
                shutil.move(os.path.join(src, entry), os.path.join(dest, entry))

        await asyncio.get_running_loop().run_in_executor(None, _move)


async def copy_tree(src: str, dest: str, engine: str = "auto") -> None:
    await CopyEngine(engine).copy_dir(src, dest)


async def move_tree_contents(src: str, dest: str) -> None:
    await CopyEngine().move_contents(src, dest)
