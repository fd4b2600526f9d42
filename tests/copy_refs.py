"""Reference helpers for the copy engine tests: a tree manifest.

A copy is the identity on ``tree_manifest``: the source tree itself is the
reference, and no engine is ever compared with another engine's output.
The walk uses ``lstat`` only and follows nothing, so a symlink that points out
of the tree is recorded as a symlink and never entered.

Per relative path (bytes, so any file name works) an ``Entry`` holds

    type     'file', 'dir', 'symlink', 'fifo', 'socket', 'chr' or 'blk'
    mode     st_mode & 0o7777
    uid, gid
    mtime    st_mtime_ns
    size     st_size (compared for regular files and symlinks only: a
             directory's size is the filesystem's business)
    sha256   of the content, regular files only
    target   symlinks only
    rdev     device nodes only
    xattrs   sorted (name, value) pairs, read without following
    links    (group, st_nlink) for non-directories. ``group`` numbers the
             classes of the partition of paths by (st_dev, st_ino) in
             sorted-path order: two trees agree on it exactly when the same
             names share an inode, whichever name a walk met first.
    blocks   st_blocks (allocation; not part of the default comparison,
             since equal trees may be laid out differently)

``atime`` is left out: reading the source changes it.

Plain module, not a conftest: it changes nothing about collection.
"""
from __future__ import annotations

import hashlib
import os
import stat
from typing import Dict, Iterable, NamedTuple, Optional, Tuple

ALL_FIELDS = (
    "type", "mode", "uid", "gid", "mtime", "size", "sha256", "target", "rdev",
    "xattrs", "links", "blocks",
)
# what a faithful copy preserves
FIELDS = tuple(f for f in ALL_FIELDS if f != "blocks")


class Entry(NamedTuple):
    type: str
    mode: int
    uid: int
    gid: int
    mtime: int
    size: Optional[int]
    sha256: Optional[str]
    target: Optional[bytes]
    rdev: Optional[int]
    xattrs: Tuple[Tuple[str, bytes], ...]
    links: Optional[Tuple[int, int]]
    blocks: int


def _type(mode: int) -> str:
    for test, name in (
        (stat.S_ISREG, "file"), (stat.S_ISDIR, "dir"), (stat.S_ISLNK, "symlink"),
        (stat.S_ISFIFO, "fifo"), (stat.S_ISSOCK, "socket"), (stat.S_ISCHR, "chr"),
        (stat.S_ISBLK, "blk"),
    ):
        if test(mode):
            return name
    raise ValueError(f"unknown file type in mode {mode:o}")


def _sha256(path: bytes) -> str:
    h = hashlib.sha256()
    # O_NOFOLLOW: the entry was a regular file a moment ago; never follow
    fd = os.open(path, os.O_RDONLY | os.O_NOFOLLOW | os.O_CLOEXEC)
    with os.fdopen(fd, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 20), b""):
            h.update(chunk)
    return h.hexdigest()


def _xattrs(path: bytes) -> Tuple[Tuple[str, bytes], ...]:
    try:
        names = os.listxattr(path, follow_symlinks=False)
    except OSError:
        return ()
    return tuple(sorted((n, os.getxattr(path, n, follow_symlinks=False)) for n in names))


def _walk(root: bytes, rel: bytes, out: Dict[bytes, os.stat_result]) -> None:
    with os.scandir(os.path.join(root, rel) if rel else root) as it:
        names = sorted(e.name for e in it)
    for name in names:
        child = os.path.join(rel, name) if rel else name
        st = os.lstat(os.path.join(root, child))
        out[child] = st
        if stat.S_ISDIR(st.st_mode):
            _walk(root, child, out)


def tree_manifest(root) -> Dict[bytes, Entry]:
    """Manifest of everything below ``root`` (the root itself is not in it)."""
    root = os.fsencode(root)
    stats: Dict[bytes, os.stat_result] = {}
    _walk(root, b"", stats)
    groups: Dict[Tuple[int, int], int] = {}
    manifest: Dict[bytes, Entry] = {}
    for rel in sorted(stats):
        st = stats[rel]
        path = os.path.join(root, rel)
        kind = _type(st.st_mode)
        links = None
        if kind != "dir":
            group = groups.setdefault((st.st_dev, st.st_ino), len(groups))
            links = (group, st.st_nlink)
        manifest[rel] = Entry(
            type=kind,
            mode=st.st_mode & 0o7777,
            uid=st.st_uid,
            gid=st.st_gid,
            mtime=st.st_mtime_ns,
            size=st.st_size if kind in ("file", "symlink") else None,
            sha256=_sha256(path) if kind == "file" else None,
            target=os.readlink(path) if kind == "symlink" else None,
            rdev=st.st_rdev if kind in ("chr", "blk") else None,
            xattrs=_xattrs(path),
            links=links,
            blocks=st.st_blocks,
        )
    return manifest


def first_difference(src, dst, fields: Iterable[str] = FIELDS, mtime_unit_ns: int = 1,
                     ignore_symlink_mode: bool = True):
    """None when the manifests agree on ``fields``; else ``(path, field,
    src value, dst value)`` of the first difference in sorted-path order. A
    path only one tree has is reported with field 'missing' or 'extra'.

    ``mtime_unit_ns`` compares mtimes in whole units (10**9: an archive
    format that stores seconds). A symlink's mode bits are the kernel's, not
    the tree's, and are skipped unless asked for."""
    fields = tuple(fields)
    unknown = set(fields) - set(ALL_FIELDS)
    if unknown:
        raise ValueError(f"unknown manifest fields {sorted(unknown)}")
    a = src if isinstance(src, dict) else tree_manifest(src)
    b = dst if isinstance(dst, dict) else tree_manifest(dst)
    for rel in sorted(set(a) | set(b)):
        if rel not in b:
            return rel, "missing", a[rel].type, None
        if rel not in a:
            return rel, "extra", None, b[rel].type
        for field in ALL_FIELDS:  # type first: the rest depends on it
            if field not in fields:
                continue
            va, vb = getattr(a[rel], field), getattr(b[rel], field)
            if field == "mtime":
                va, vb = va // mtime_unit_ns, vb // mtime_unit_ns
            if field == "mode" and ignore_symlink_mode and a[rel].type == "symlink":
                continue
            if va != vb:
                return rel, field, va, vb
    return None


def assert_same_tree(src, dst, fields: Iterable[str] = FIELDS, mtime_unit_ns: int = 1) -> None:
    diff = first_difference(src, dst, fields, mtime_unit_ns)
    if diff is not None:
        rel, field, va, vb = diff
        if field == "sha256":
            field = "sha256 (content)"
        if field == "links":
            field = "links (hardlink partition group, st_nlink)"
        raise AssertionError(f"{rel!r}: {field} differs: source {va!r}, copy {vb!r}")
