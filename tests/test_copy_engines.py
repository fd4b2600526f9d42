"""Copy engines: native io_uring, tar pipe, python — all must preserve a
representative rootfs tree (files, symlinks, sparse files, subdirs).

Below the four first tests the native engine is held to a full-tree manifest
(tests/copy_refs.py): the copy is the identity on it, so the source tree is
the reference. Every native case runs under the three data paths, and
``CopyEngine.copy_dir`` is held to a per-route contract (``CONTRACT``)."""
import hashlib
import json
import os
import stat
import subprocess
import sys

import pytest

import copy_refs as cr
from gpu_docker_api_amd.ops import iocopy
from gpu_docker_api_amd.utils import copy as copy_mod
from gpu_docker_api_amd.utils.copy import CopyEngine
from gpu_docker_api_amd.utils.files import dir_size


def _make_tree(src):
    os.makedirs(src / "sub/deep", exist_ok=True)
    (src / "a.txt").write_text("alpha" * 2000)
    (src / "sub" / "b.bin").write_bytes(os.urandom(300_000))
    (src / "sub" / "deep" / "c.txt").write_text("deep")
    os.symlink("a.txt", src / "lnk")
    with open(src / "sparse.bin", "wb") as f:
        f.write(b"S")
        f.seek(4 * 1024 * 1024)
        f.write(b"E")
    os.chmod(src / "a.txt", 0o640)


def _check_tree(dst):
    assert (dst / "a.txt").read_text() == "alpha" * 2000
    assert (dst / "sub" / "deep" / "c.txt").read_text() == "deep"
    assert os.readlink(dst / "lnk") == "a.txt"
    with open(dst / "sparse.bin", "rb") as f:
        assert f.read(1) == b"S"
        f.seek(4 * 1024 * 1024)
        assert f.read(1) == b"E"
    assert (os.stat(dst / "a.txt").st_mode & 0o777) == 0o640


@pytest.mark.parametrize("engine", ["iouring", "tar", "python"])
def test_copy_dir_engines(tmp_path, run, engine):
    if engine == "iouring" and not iocopy.uring_available():
        # extension built but kernel refuses io_uring: the engine itself
        # falls back internally; still exercise it
        pass
    src, dst = tmp_path / "src", tmp_path / "dst"
    os.makedirs(src)
    _make_tree(src)

    async def main():
        await CopyEngine(engine).copy_dir(str(src), str(dst))

    run(main())
    _check_tree(dst)


def test_iocopy_stats_and_sparse(tmp_path):
    src, dst = tmp_path / "src", tmp_path / "dst"
    os.makedirs(src)
    _make_tree(src)
    stats = iocopy.copy_tree(str(src), str(dst))
    assert stats["files"] == 4
    assert stats["symlinks"] == 1
    # sparse copy must not materialize the hole
    blocks = os.stat(dst / "sparse.bin").st_blocks * 512
    assert blocks < 1024 * 1024, f"sparse file materialized: {blocks} bytes allocated"
    _check_tree(dst / "")


def test_move_contents(tmp_path, run):
    src, dst = tmp_path / "src", tmp_path / "dst"
    os.makedirs(src)
    (src / "x.txt").write_text("x")
    os.makedirs(src / "d")
    (src / "d" / "y.txt").write_text("y")

    async def main():
        await CopyEngine().move_contents(str(src), str(dst))

    run(main())
    assert (dst / "x.txt").read_text() == "x"
    assert (dst / "d" / "y.txt").read_text() == "y"
    assert os.listdir(src) == []


def test_dir_size_counts_allocation(tmp_path):
    (tmp_path / "f.bin").write_bytes(b"z" * 100_000)
    with open(tmp_path / "s.bin", "wb") as f:
        f.seek(50 * 1024 * 1024)
        f.write(b"e")
    sz = dir_size(str(tmp_path))
    # sparse file contributes allocation (~4KB), not 50MB
    assert 100_000 <= sz < 5 * 1024 * 1024


# ---------------------------------------------------------------------------
# The native engine against the manifest oracle
# ---------------------------------------------------------------------------

KIB, MIB = 1024, 1024 * 1024
SMALL_MAX = 256 * KIB  # csrc/iocopy_core.h kSmallCutoff: last size in the ring
RING_DEPTH = 16        # kDepth: files in flight
BATCH_JOBS = 4096      # kBatchJobs: the job list is flushed at this length
CFR_MAX = 8 * MIB      # largest single copy_file_range request, 8 * kChunk

# the three data paths: ring, copy_file_range loop, pread/pwrite. The first
# is the call without arguments, as the daemon makes it.
PATHS = {
    "uring+cfr": {},
    "cfr": {"use_uring": False},
    "pread-pwrite": {"use_uring": False, "use_copy_file_range": False},
}
all_paths = pytest.mark.parametrize("path", list(PATHS))

IS_ROOT = os.geteuid() == 0
needs_root = pytest.mark.skipif(not IS_ROOT, reason="needs root: chown, mknod, trusted.* xattrs")
OWNER = (1000, 1000)


def _native(src, dst, path):
    stats = iocopy.copy_tree(str(src), str(dst), **PATHS[path])
    if path == "uring+cfr":
        assert iocopy.uring_available(), "io_uring refused here: the ring path cannot be tested"
    return stats


def _content(name, n):
    """n bytes derived from the name, so a buffer that lands in another file
    shows as a content difference."""
    return hashlib.shake_256(os.fsencode(name)).digest(n) if n else b""


def _put(path, n, name=None):
    with open(path, "wb") as f:
        f.write(_content(name if name is not None else os.path.basename(path), n))


def _set_mtime(path, ns):
    os.utime(path, ns=(ns, ns), follow_symlinks=False)


def _fresh(tmp_path):
    src, dst = tmp_path / "src", tmp_path / "dst"
    os.makedirs(src)
    return src, dst


def _extents(path):
    """Data extents of a file as the filesystem reports them."""
    out = []
    with open(path, "rb") as f:
        size = os.fstat(f.fileno()).st_size
        pos = 0
        while pos < size:
            try:
                data = os.lseek(f.fileno(), pos, os.SEEK_DATA)
            except OSError:  # ENXIO: nothing but hole behind pos
                break
            hole = os.lseek(f.fileno(), data, os.SEEK_HOLE)
            out.append((data, hole))
            pos = hole
    return out


def _assert_allocation(src, dst, names):
    """Where the source is sparse on this filesystem, the copy may allocate
    the source's allocation plus one block per data extent (extent ends round
    to blocks). Returns the names that were checked."""
    checked = []
    for name in names:
        s, d = os.lstat(os.path.join(src, name)), os.lstat(os.path.join(dst, name))
        if s.st_blocks * 512 >= s.st_size:
            continue  # not sparse here
        bound = s.st_blocks * 512 + s.st_blksize * len(_extents(os.path.join(src, name)))
        print(f"{name}: size {s.st_size}, source allocates {s.st_blocks * 512}, "
              f"copy {d.st_blocks * 512}, bound {bound}")
        assert d.st_blocks * 512 <= bound, (
            f"{name}: hole materialised: copy allocates {d.st_blocks * 512} bytes, "
            f"source {s.st_blocks * 512}, bound {bound}")
        checked.append(name)
    return checked


FILE_SIZES = [0, 1, 4095, 4096, SMALL_MAX - 1, SMALL_MAX, SMALL_MAX + 1, MIB + 1, CFR_MAX + 1]


@all_paths
def test_file_sizes(tmp_path, path):
    src, dst = _fresh(tmp_path)
    for n in FILE_SIZES:
        _put(src / f"f{n}", n)
        _set_mtime(src / f"f{n}", 1_600_000_000_000_000_000 + n)
    stats = _native(src, dst, path)
    for n in FILE_SIZES:  # finding 1 reads as a size mismatch
        assert os.lstat(dst / f"f{n}").st_size == n, f"f{n}: size mismatch"
    cr.assert_same_tree(src, dst)
    assert stats["files"] == len(FILE_SIZES)
    assert stats["bytes"] == sum(FILE_SIZES)
    assert stats["io_uring"] == (path == "uring+cfr")


def _make_sparse(src):
    with open(src / "leading", "wb") as f:
        f.seek(MIB)
        f.write(_content("leading", 64 * KIB))
    with open(src / "interior", "wb") as f:
        f.write(_content("interior-a", 64 * KIB))
        f.seek(MIB + 64 * KIB)
        f.write(_content("interior-b", 64 * KIB))
    with open(src / "trailing", "wb") as f:  # SEEK_DATA behind the data: ENXIO
        f.write(_content("trailing", 64 * KIB))
        f.truncate(MIB + 64 * KIB)
    with open(src / "all-hole", "wb") as f:
        f.truncate(4 * MIB)
    with open(src / "small-leading", "wb") as f:  # below the small/large cut-over
        f.seek(128 * KIB)
        f.write(_content("small-leading", 4 * KIB))
    return ["leading", "interior", "trailing", "all-hole", "small-leading"]


@all_paths
def test_sparse_files(tmp_path, path):
    src, dst = _fresh(tmp_path)
    names = _make_sparse(src)
    _native(src, dst, path)
    cr.assert_same_tree(src, dst)  # logical size and content
    if not _assert_allocation(src, dst, names):
        pytest.skip(f"no sparse allocation on the filesystem of {tmp_path} "
                    f"(st_dev {os.lstat(src).st_dev}): allocation bound not checked")


@all_paths
@pytest.mark.parametrize("count", [RING_DEPTH + 1, 40, BATCH_JOBS + 1])
def test_file_counts(tmp_path, path, count):
    src, dst = _fresh(tmp_path)
    os.makedirs(src / "d")
    total = 0
    for i in range(count):
        # distinct lengths at 40; a few bytes each at 4097
        n = 1 + 97 * i if count <= 40 else 1 + i % 7
        _put(src / "d" / f"n{i:05d}", n)
        total += n
    names = count
    if count > BATCH_JOBS:
        # one inode under two names that sort far apart; it is one job, so
        # the job list still holds one more than a flush
        os.link(src / "d" / "n00000", src / "d" / "zz-second-name")
        os.link(src / "d" / "n00000", src / "zz-third-name")
        names += 2
    stats = _native(src, dst, path)
    cr.assert_same_tree(src, dst)
    assert stats["files"] == names
    assert stats["bytes"] == total


@all_paths
def test_hardlinks(tmp_path, path):
    src, dst = _fresh(tmp_path)
    os.makedirs(src / "a" / "deep")
    os.makedirs(src / "b")
    _put(src / "a" / "pair-1", 1000)
    os.link(src / "a" / "pair-1", src / "a" / "pair-2")
    _put(src / "a" / "deep" / "across-1", 2000)
    os.link(src / "a" / "deep" / "across-1", src / "b" / "across-2")
    _put(src / "three-1", 1000)
    os.link(src / "three-1", src / "a" / "three-2")
    os.link(src / "three-1", src / "b" / "three-3")
    _put(src / "b" / "large-1", SMALL_MAX + 1)
    os.link(src / "b" / "large-1", src / "a" / "large-2")
    _put(src / "single", 10)
    stats = _native(src, dst, path)
    # readdir order is not sorted: assert the partition, not which name came
    # first (finding 2 reads as a difference in 'links')
    cr.assert_same_tree(src, dst, fields=("type", "links"))
    cr.assert_same_tree(src, dst)
    assert stats["files"] == 10  # names
    assert stats["bytes"] == 1000 + 2000 + 1000 + SMALL_MAX + 1 + 10  # each inode once


@all_paths
def test_more_names_of_one_inode_than_a_batch(tmp_path, path):
    """Names waiting for their first name's batch are flushed at the same
    length as the job list: one past it."""
    src, dst = _fresh(tmp_path)
    os.makedirs(src / "d")
    _put(src / "d" / "first", 100)
    for i in range(BATCH_JOBS + 1):
        os.link(src / "d" / "first", src / "d" / f"name{i:05d}")
    _put(src / "other", 7)
    stats = _native(src, dst, path)
    cr.assert_same_tree(src, dst)
    assert os.lstat(dst / "d" / "first").st_nlink == BATCH_JOBS + 2
    assert stats["files"] == BATCH_JOBS + 3
    assert stats["bytes"] == 107


@all_paths
def test_symlinks(tmp_path, path):
    src, dst = _fresh(tmp_path)
    outside = tmp_path / "outside"
    os.makedirs(outside / "sub")
    _put(outside / "sub" / "kept", 100)
    os.makedirs(src / "d")
    _put(src / "d" / "file", 10)
    os.symlink("d/file", src / "relative")
    os.symlink("/etc/hostname", src / "absolute")
    os.symlink("no/such/target", src / "dangling")
    os.symlink(outside, src / "outside-dir")
    long_target = "/".join(["x" * 199] * 20) + "y"
    assert len(long_target) == 4000
    os.symlink(long_target, src / "d" / "long")
    for i, name in enumerate(["relative", "absolute", "dangling", "outside-dir", "d/long"]):
        _set_mtime(src / name, 1_500_000_000_000_000_001 + i)
        if IS_ROOT:
            os.chown(src / name, *OWNER, follow_symlinks=False)
    before = cr.tree_manifest(outside)
    _native(src, dst, path)
    cr.assert_same_tree(src, dst)  # owner and mtime of the symlinks included
    assert os.path.islink(dst / "outside-dir")
    assert cr.first_difference(before, cr.tree_manifest(outside)) is None, (
        "the copy created or changed something under a symlink's target")
    assert len(os.readlink(dst / "d" / "long")) == 4000


@all_paths
def test_special_files(tmp_path, path):
    src, dst = _fresh(tmp_path)
    os.makedirs(src / "d")
    os.mkfifo(src / "d" / "fifo", 0o640)
    os.mknod(src / "sock", stat.S_IFSOCK | 0o755)
    _set_mtime(src / "sock", 1_500_000_000_000_000_007)
    stats = _native(src, dst, path)
    cr.assert_same_tree(src, dst)
    assert stats["specials"] == 2


@needs_root
@all_paths
def test_overlay_whiteout_and_opaque_marker(tmp_path, path):
    src, dst = _fresh(tmp_path)
    os.makedirs(src / "opaque")
    _put(src / "opaque" / "f", 10)
    os.setxattr(src / "opaque", "trusted.overlay.opaque", b"y")
    os.mknod(src / "deleted", stat.S_IFCHR | 0o000, os.makedev(0, 0))  # whiteout
    os.mknod(src / "null", stat.S_IFCHR | 0o666, os.makedev(1, 3))
    _native(src, dst, path)
    cr.assert_same_tree(src, dst)
    m = cr.tree_manifest(dst)
    assert m[b"deleted"].type == "chr" and m[b"deleted"].rdev == os.makedev(0, 0)
    assert m[b"opaque"].xattrs == (("trusted.overlay.opaque", b"y"),)


def _largest_xattr_value(path, name):
    """A 4 KiB value; where the filesystem keeps a value within one block
    (ext4 without ea_inode), the largest of these it takes."""
    for n in (4096, 4000, 3072, 2048):
        try:
            os.setxattr(path, name, _content(name, n))
            return n
        except OSError as exc:
            last = exc
    raise last


@all_paths
def test_xattrs(tmp_path, path):
    src, dst = _fresh(tmp_path)
    os.makedirs(src / "d")
    _put(src / "d" / "small", 10)
    _put(src / "large", SMALL_MAX + 1)
    os.setxattr(src / "d" / "small", "user.empty", b"")
    os.setxattr(src / "d" / "small", "user.note", b"\x00binary\xff")
    os.setxattr(src / "d", "user.on-dir", b"dir")
    os.setxattr(src / "large", "user.note", b"large")
    n = _largest_xattr_value(src / "large", "user.big")
    print(f"largest xattr value taken: {n} bytes")
    assert n >= 2048
    _native(src, dst, path)
    cr.assert_same_tree(src, dst)
    m = cr.tree_manifest(dst)
    assert dict(m[b"d/small"].xattrs)["user.empty"] == b""
    assert len(dict(m[b"large"].xattrs)["user.big"]) == n


@all_paths
def test_modes_and_times(tmp_path, path):
    src, dst = _fresh(tmp_path)
    for name, mode in (("setgid", 0o2750), ("sticky", 0o1777), ("readonly", 0o555)):
        os.makedirs(src / name)
        _put(src / name / "inside", 100, name)
        os.chmod(src / name / "inside", 0o444)
        _set_mtime(src / name / "inside", 1_234_567_890_123_456_789)
    _put(src / "exec", 10)
    os.chmod(src / "exec", 0o755)
    _put(src / "large", SMALL_MAX + 1)
    os.chmod(src / "large", 0o604)
    _set_mtime(src / "large", 987_654_321_000_000_001)
    for name, mode in (("setgid", 0o2750), ("sticky", 0o1777), ("readonly", 0o555)):
        os.chmod(src / name, mode)
    # a directory's mtime, set after it was populated, arrives to the ns
    _set_mtime(src / "setgid", 1_111_111_111_111_111_111)
    _set_mtime(src / "readonly", 999_999_999_999_999_999)
    try:
        _native(src, dst, path)
        cr.assert_same_tree(src, dst)
        assert cr.tree_manifest(dst)[b"setgid"].mtime == 1_111_111_111_111_111_111
        assert cr.tree_manifest(dst)[b"readonly"].mode == 0o555
    finally:
        for tree in (src, dst):
            if os.path.isdir(tree / "readonly"):
                os.chmod(tree / "readonly", 0o755)  # let tmp_path be cleaned up


@needs_root
@all_paths
def test_privileged_modes_and_owner(tmp_path, path):
    src, dst = _fresh(tmp_path)
    os.makedirs(src / "d")
    _put(src / "d" / "unreadable", 100)
    os.chmod(src / "d" / "unreadable", 0o000)
    _put(src / "d" / "setuid", 100)
    os.chown(src / "d" / "setuid", *OWNER)
    os.chmod(src / "d" / "setuid", 0o4755)  # must survive the chown at the destination
    _put(src / "large-owned", SMALL_MAX + 1)
    os.chown(src / "large-owned", *OWNER)
    os.chown(src / "d", OWNER[0], 0)
    _native(src, dst, path)
    cr.assert_same_tree(src, dst)
    st = os.lstat(dst / "d" / "setuid")
    assert (st.st_uid, st.st_gid, st.st_mode & 0o7777) == (*OWNER, 0o4755)


@all_paths
def test_names(tmp_path, path):
    src, dst = _fresh(tmp_path)
    bsrc = os.fsencode(src)
    names = [b"\xff\xfe not utf-8 \x80", b"new\nline", b"-rf", b"--help", b"n" * 255]
    os.mkdir(os.path.join(bsrc, b"dir \xe9"))
    for name in names:
        _put(os.path.join(bsrc, name), 50, name)
        _put(os.path.join(bsrc, b"dir \xe9", name), 60, b"d/" + name)
    _native(src, dst, path)
    cr.assert_same_tree(src, dst)
    assert set(os.listdir(os.fsencode(dst))) == set(names) | {b"dir \xe9"}


@all_paths
def test_non_empty_destination(tmp_path, path):
    src, dst = _fresh(tmp_path)
    victim, outside = tmp_path / "victim", tmp_path / "outside-dir"
    os.makedirs(src / "d")
    os.makedirs(src / "was-link-dir")
    _put(src / "replaced", 500)
    _put(src / "a", 300)
    _put(src / "large", SMALL_MAX + 1)
    _put(src / "d" / "f", 10)
    _put(src / "was-link-dir" / "g", 10)
    os.symlink("a", src / "was-file")
    os.chmod(src / "d", 0o750)

    os.makedirs(dst / "d")
    os.makedirs(outside)
    os.chmod(dst / "d", 0o700)
    (dst / "replaced").write_bytes(b"old content, and longer than the new one" * 100)
    # another name of the old file, outside the tree: a snapshot keeps it
    os.link(dst / "replaced", tmp_path / "snapshot")
    victim.write_bytes(b"victim")
    os.symlink(victim, dst / "a")  # finding 3
    os.symlink(victim, dst / "large")
    os.symlink(outside, dst / "was-link-dir")
    (dst / "was-file").write_bytes(b"file where the source has a symlink")
    (dst / "d" / "f").write_bytes(b"old")

    _native(src, dst, path)
    assert victim.read_bytes() == b"victim", "victim content changed: written through a symlink"
    assert os.listdir(outside) == [], "a directory was filled through a symlink"
    assert (tmp_path / "snapshot").read_bytes().startswith(b"old content"), (
        "an existing file was overwritten in place: its other name changed too")
    cr.assert_same_tree(src, dst)
    assert os.lstat(dst / "d").st_mode & 0o7777 == 0o750


# --- errors ------------------------------------------------------------------

_SHORT_WRITE_CHILD = r"""
import json, os, resource, signal, sys
from gpu_docker_api_amd.ops import iocopy
src, dst, kwargs = sys.argv[1], sys.argv[2], json.loads(sys.argv[3])
signal.signal(signal.SIGXFSZ, signal.SIG_IGN)
resource.setrlimit(resource.RLIMIT_FSIZE, (100_000, 100_000))
out = {"raised": None, "stats": None}
try:
    out["stats"] = iocopy.copy_tree(src, dst, **kwargs)
except Exception as exc:
    out["raised"] = f"{type(exc).__name__}: {exc}"
try:
    out["size"] = os.lstat(os.path.join(dst, "big")).st_size
except OSError:
    out["size"] = None
sys.stdout.write(json.dumps(out))
"""


@all_paths
def test_short_write_raises(tmp_path, path):
    """With SIGXFSZ ignored, a write across RLIMIT_FSIZE is short first and
    EFBIG after: what a full quota volume does before ENOSPC. The limit and
    the signal disposition are process-wide, hence the child."""
    src, dst = _fresh(tmp_path)
    _put(src / "big", 200_000)
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=repo)
    proc = subprocess.run(
        [sys.executable, "-c", _SHORT_WRITE_CHILD, str(src), str(dst), json.dumps(PATHS[path])],
        capture_output=True, text=True, timeout=60, env=env, cwd=repo)
    assert proc.returncode == 0, proc.stderr
    out = json.loads(proc.stdout)
    assert out["raised"] is not None, (
        f"size mismatch: source 200000 bytes, destination {out['size']}, "
        f"and copy_tree returned {out['stats']}")


def _open_fds():
    return len(os.listdir("/proc/self/fd"))


@all_paths
def test_failing_destination_leaks_nothing(tmp_path, path):
    src, dst = _fresh(tmp_path)
    os.makedirs(src / "d1" / "d2")
    for i in range(30):  # more than the ring depth, so reads are in flight
        _put(src / "d1" / "d2" / f"n{i:02d}", 3000 + i)
    os.makedirs(dst / "d1" / "d2" / "n15")  # a directory where the source has a file
    _native(src, tmp_path / "warm", path)
    before = _open_fds()
    with pytest.raises(RuntimeError):
        _native(src, dst, path)
    assert _open_fds() - before == 0, "descriptor count delta after one failing call"
    for _ in range(50):
        with pytest.raises(RuntimeError):
            _native(src, dst, path)
    assert _open_fds() - before == 0, "descriptor count delta after 50 failing calls"
    assert os.path.isdir(dst / "d1" / "d2" / "n15")


@all_paths
def test_bad_source_raises(tmp_path, path):
    src, dst = _fresh(tmp_path)
    _put(src / "file", 10)
    with pytest.raises(RuntimeError):
        _native(tmp_path / "missing", dst, path)
    with pytest.raises(RuntimeError, match="not a directory"):
        _native(src / "file", dst, path)
    os.symlink(src, tmp_path / "link-to-src")
    with pytest.raises(RuntimeError, match="not a directory"):
        _native(tmp_path / "link-to-src", dst, path)
    assert not os.path.lexists(dst)


# ---------------------------------------------------------------------------
# CopyEngine.copy_dir: what each route must preserve
# ---------------------------------------------------------------------------
#
# | Route    | Must preserve                                                   |
# |----------|-----------------------------------------------------------------|
# | iouring  | the full manifest                                               |
# | auto     | as iouring (the native engine is built wherever the tests run)  |
# | tar      | the full manifest, mtime at whole seconds (archive format);     |
# |          | sparse allocation where `tar --help` offers --sparse; sockets   |
# |          | are not archivable and are left out of its tree                 |
# | python   | content, mode, mtime and symlinks; it exists for tests          |
# | inline   | everything the engine selected by `auto` would preserve: the    |
# |          | full manifest. Trees it cannot carry (names sharing an inode,   |
# |          | holes) are declined and go to the engine.                       |
CONTRACT = {
    "iouring": {"fields": cr.FIELDS, "mtime_unit_ns": 1, "specials": ("fifo", "socket"),
                "sparse": True},
    "auto": {"fields": cr.FIELDS, "mtime_unit_ns": 1, "specials": ("fifo", "socket"),
             "sparse": True},
    "tar": {"fields": cr.FIELDS, "mtime_unit_ns": 10**9, "specials": ("fifo",),
            "sparse": copy_mod._tar_supports("--sparse")},
    "python": {"fields": ("type", "size", "sha256", "mode", "mtime", "target"),
               "mtime_unit_ns": 1, "specials": (), "sparse": False},
    "inline": {"fields": cr.FIELDS, "mtime_unit_ns": 1},
}


def _representative_tree(src, specials):
    """A writable layer in small: nested directories, small and large files,
    names sharing an inode, symlinks, xattrs, a sparse file, modes, and as
    root foreign owners and overlayfs markers."""
    os.makedirs(src / "etc" / "conf.d")
    os.makedirs(src / "var" / "empty")
    for i in range(20):
        _put(src / "etc" / "conf.d" / f"{i:02d}.conf", 10 + 300 * i)
    _put(src / "etc" / "passwd", 1500)
    os.chmod(src / "etc" / "passwd", 0o644)
    os.link(src / "etc" / "passwd", src / "etc" / "passwd-")
    _put(src / "var" / "blob", SMALL_MAX + 4097)
    os.link(src / "var" / "blob", src / "blob-again")
    os.symlink("etc/passwd", src / "rel")
    os.symlink("/nonexistent", src / "var" / "dangling")
    os.setxattr(src / "etc" / "passwd", "user.origin", b"layer")
    os.setxattr(src / "var", "user.on-dir", b"")
    with open(src / "var" / "sparse", "wb") as f:
        f.write(b"S")
        f.seek(2 * MIB)
        f.write(b"E")
    if "fifo" in specials:
        os.mkfifo(src / "var" / "fifo")
    if "socket" in specials:
        os.mknod(src / "var" / "sock", stat.S_IFSOCK | 0o600)
    if IS_ROOT:
        os.chown(src / "etc" / "conf.d" / "03.conf", *OWNER)
        os.chown(src / "var" / "blob", *OWNER)
        os.chown(src / "var" / "empty", *OWNER)
        os.chown(src / "rel", *OWNER, follow_symlinks=False)
        os.chmod(src / "etc" / "conf.d" / "03.conf", 0o4750)
        if specials:
            os.mknod(src / "etc" / "whiteout", stat.S_IFCHR, os.makedev(0, 0))
            os.setxattr(src / "var" / "empty", "trusted.overlay.opaque", b"y")
    os.chmod(src / "var" / "empty", 0o2775)
    _set_mtime(src / "rel", 1_500_000_000_000_000_003)
    _set_mtime(src / "etc" / "passwd", 1_600_000_000_123_456_789)
    _set_mtime(src / "etc", 1_400_000_000_999_999_999)


class _Spy:
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *a, **kw):
        self.calls += 1
        return self.fn(*a, **kw)


@pytest.mark.parametrize("route", ["iouring", "auto", "tar", "python"])
def test_copy_dir_contract(tmp_path, run, monkeypatch, route):
    want = CONTRACT[route]
    src, dst = _fresh(tmp_path)
    _representative_tree(src, want["specials"])

    # the route under test is the one that runs: not the inline shortcut, and
    # for tar and python not the native engine either
    def no_inline(*a, **kw):
        raise AssertionError("the inline shortcut took a tree with subdirectories")

    monkeypatch.setattr(CopyEngine, "_copy_entry_inline", staticmethod(no_inline))
    native = _Spy(iocopy.copy_tree)
    monkeypatch.setattr(iocopy, "copy_tree", native)
    tar = _Spy(copy_mod._tar_pipe_copy)
    monkeypatch.setattr(copy_mod, "_tar_pipe_copy", tar)

    async def main():
        await CopyEngine(route).copy_dir(str(src), str(dst))

    run(main())
    assert native.calls == (1 if route in ("iouring", "auto") else 0)
    assert tar.calls == (1 if route == "tar" else 0)
    cr.assert_same_tree(src, dst, fields=want["fields"], mtime_unit_ns=want["mtime_unit_ns"])
    if want["sparse"] and not _assert_allocation(src, dst, ["var/sparse"]):
        print("source not sparse on this filesystem: allocation bound not checked")


def _flat_tree(src):
    for i in range(5):
        _put(src / f"f{i}", 100 + 1000 * i)
        _set_mtime(src / f"f{i}", 1_600_000_000_000_000_001 + i)
    _put(src / "a", 300)
    os.chmod(src / "f1", 0o640)
    os.setxattr(src / "f2", "user.origin", b"layer")
    os.setxattr(src / "f2", "user.empty", b"")
    os.symlink("f1", src / "lnk")
    _set_mtime(src / "lnk", 1_500_000_000_000_000_003)
    if IS_ROOT:
        os.chown(src / "f3", *OWNER)  # finding 5 reads as a uid difference
        os.chmod(src / "f3", 0o4755)
        os.chown(src / "lnk", *OWNER, follow_symlinks=False)


@pytest.mark.parametrize("non_empty", [False, True], ids=["fresh-dst", "non-empty-dst"])
@pytest.mark.parametrize("kind", ["auto", "iouring", "tar", "python"])
def test_inline_shortcut_contract(tmp_path, run, monkeypatch, kind, non_empty):
    """Near-empty layers are the common case of a replace and never reach an
    engine, whichever is configured."""
    src, dst = _fresh(tmp_path)
    _flat_tree(src)
    victim = tmp_path / "victim"
    victim.write_bytes(b"victim")
    if non_empty:
        os.makedirs(dst)
        os.symlink(victim, dst / "a")
        (dst / "f0").write_bytes(b"old" * 1000)

    def no_engine(*a, **kw):
        raise AssertionError("a flat tree of 7 entries went to an engine, not the shortcut")

    monkeypatch.setattr(copy_mod, "_load_iocopy", no_engine)
    monkeypatch.setattr(copy_mod, "_tar_pipe_copy", no_engine)
    monkeypatch.setattr(copy_mod.shutil, "copytree", no_engine)

    async def main():
        await CopyEngine(kind).copy_dir(str(src), str(dst))

    run(main())
    want = CONTRACT["inline"]
    cr.assert_same_tree(src, dst, fields=want["fields"], mtime_unit_ns=want["mtime_unit_ns"])
    assert victim.read_bytes() == b"victim", "victim content changed: written through a symlink"


def _hardlinked_siblings(src):
    _put(src / "one", 1000)
    os.link(src / "one", src / "two")


def _small_sparse(src):
    with open(src / "sparse", "wb") as f:
        f.seek(512 * KIB)
        f.write(b"E")


def _special(src):
    _put(src / "f", 10)
    os.mkfifo(src / "fifo")


@pytest.mark.parametrize("make", [_hardlinked_siblings, _small_sparse, _special],
                         ids=["hardlinked siblings", "sparse file", "fifo"])
def test_inline_shortcut_declines_what_it_cannot_carry(tmp_path, run, monkeypatch, make):
    src, dst = _fresh(tmp_path)
    make(src)
    assert CopyEngine._small_tree_entries(str(src)) is None
    native = _Spy(iocopy.copy_tree)
    monkeypatch.setattr(iocopy, "copy_tree", native)

    async def main():
        await CopyEngine("auto").copy_dir(str(src), str(dst))

    run(main())
    assert native.calls == 1
    cr.assert_same_tree(src, dst)
    _assert_allocation(src, dst, [n for n in os.listdir(src) if n == "sparse"])


def test_copy_dir_rejects_a_missing_source(tmp_path, run):
    async def main():
        await CopyEngine("auto").copy_dir(str(tmp_path / "missing"), str(tmp_path / "dst"))

    with pytest.raises(FileNotFoundError):
        run(main())
