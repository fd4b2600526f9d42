"""CPU tests of tests/copy_refs.py: the manifest comparator passes a faithful
copy and reports every single attribute a copy engine could get wrong, so it
cannot be blind to a field. The faithful copy is made here, in plain Python,
not by any engine under test."""
import contextlib
import os

import pytest

import copy_refs as cr


def _set_user_xattr(path, name, value):
    try:
        os.setxattr(path, name, value, follow_symlinks=False)
    except OSError as exc:
        pytest.skip(f"user xattrs unavailable under the test directory: {exc}")


def _make_tree(src):
    os.makedirs(src / "d" / "e")
    (src / "a.bin").write_bytes(bytes(range(256)) * 8)
    (src / "d" / "b.txt").write_bytes(b"bravo\n")
    (src / "d" / "e" / "c.txt").write_bytes(b"")
    os.link(src / "a.bin", src / "d" / "a-again")
    os.symlink("b.txt", src / "d" / "lnk")
    os.mkfifo(src / "d" / "pipe")
    _set_user_xattr(src / "d" / "b.txt", "user.k", b"value")
    _set_user_xattr(src / "d", "user.dir", b"")
    os.chmod(src / "d" / "b.txt", 0o640)
    os.chmod(src / "d" / "e", 0o2750)
    os.utime(src / "a.bin", ns=(1_600_000_000_123_456_789, 1_600_000_000_123_456_789))
    os.utime(src / "d" / "lnk", ns=(1_500_000_000_000_000_001,) * 2, follow_symlinks=False)
    os.utime(src / "d", ns=(1_400_000_000_999_999_999,) * 2)


def _faithful_copy(src, dst):
    """lstat-only copy in plain Python, small enough to be read as correct."""
    seen = {}
    todo_dirs = []

    def meta(s, d, st):
        for name in os.listxattr(s, follow_symlinks=False):
            os.setxattr(d, name, os.getxattr(s, name, follow_symlinks=False),
                        follow_symlinks=False)
        if os.geteuid() == 0:
            os.chown(d, st.st_uid, st.st_gid, follow_symlinks=False)
        if not os.path.islink(d):
            os.chmod(d, st.st_mode & 0o7777)
        os.utime(d, ns=(st.st_atime_ns, st.st_mtime_ns), follow_symlinks=False)

    def walk(s, d):
        st = os.lstat(s)
        if os.path.isdir(s) and not os.path.islink(s):
            os.mkdir(d)
            for name in os.listdir(s):
                walk(os.path.join(s, name), os.path.join(d, name))
            todo_dirs.append((s, d, st))
        elif os.path.islink(s):
            os.symlink(os.readlink(s), d)
            meta(s, d, st)
        elif os.path.isfile(s):
            key = (st.st_dev, st.st_ino)
            if key in seen:
                os.link(seen[key], d)
                return
            seen[key] = d
            with open(s, "rb") as f, open(d, "wb") as g:
                g.write(f.read())
            meta(s, d, st)
        else:
            os.mknod(d, st.st_mode, st.st_rdev)
            meta(s, d, st)

    walk(str(src), str(dst))
    for s, d, st in reversed(todo_dirs[:-1]):
        meta(s, d, st)


@contextlib.contextmanager
def _keeping(*paths):
    """Restore the mtime of the given paths (the parents of a mutation)."""
    before = [(p, os.lstat(p)) for p in paths]
    yield
    for p, st in before:
        os.utime(p, ns=(st.st_atime_ns, st.st_mtime_ns), follow_symlinks=False)


@pytest.fixture
def trees(tmp_path):
    src, dst = tmp_path / "src", tmp_path / "dst"
    os.makedirs(src)
    _make_tree(src)
    _faithful_copy(src, dst)
    return src, dst


def test_manifest_contents(trees):
    src, _ = trees
    m = cr.tree_manifest(src)
    assert sorted(m) == [b"a.bin", b"d", b"d/a-again", b"d/b.txt", b"d/e", b"d/e/c.txt",
                         b"d/lnk", b"d/pipe"]
    assert m[b"a.bin"].type == "file" and m[b"a.bin"].size == 2048
    assert m[b"a.bin"].mtime == 1_600_000_000_123_456_789
    assert m[b"a.bin"].links == m[b"d/a-again"].links == (0, 2)
    assert m[b"d/b.txt"].links == (1, 1) and m[b"d/b.txt"].mode == 0o640
    assert m[b"d/b.txt"].xattrs == (("user.k", b"value"),)
    assert m[b"d"].type == "dir" and m[b"d"].links is None and m[b"d"].sha256 is None
    assert m[b"d"].xattrs == (("user.dir", b""),)
    assert m[b"d/e"].mode == 0o2750
    assert m[b"d/lnk"].type == "symlink" and m[b"d/lnk"].target == b"b.txt"
    assert m[b"d/lnk"].mtime == 1_500_000_000_000_000_001
    assert m[b"d/pipe"].type == "fifo"
    assert m[b"d/e/c.txt"].sha256 == (
        "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855")


def test_faithful_copy_passes(trees):
    src, dst = trees
    assert cr.first_difference(src, dst) is None
    cr.assert_same_tree(src, dst)
    cr.assert_same_tree(src, dst, fields=cr.ALL_FIELDS[:3])
    with pytest.raises(ValueError):
        cr.first_difference(src, dst, fields=("colour",))


def test_manifest_follows_nothing(tmp_path):
    outside = tmp_path / "outside"
    os.makedirs(outside / "deep")
    (outside / "deep" / "secret").write_bytes(b"s")
    root = tmp_path / "root"
    os.makedirs(root)
    os.symlink(outside, root / "out")
    os.symlink("/nonexistent/target", root / "dangling")
    m = cr.tree_manifest(root)
    assert sorted(m) == [b"dangling", b"out"]
    assert m[b"out"].target == os.fsencode(outside)


def _one_byte(dst):
    p = dst / "a.bin"
    with _keeping(p):
        with open(p, "r+b") as f:
            f.seek(1000)
            f.write(b"\xff")


def _mode(dst):
    os.chmod(dst / "d" / "b.txt", 0o600)


def _uid(dst):
    os.chown(dst / "d" / "b.txt", 1000, -1)


def _mtime_1ns(dst):
    st = os.lstat(dst / "a.bin")
    os.utime(dst / "a.bin", ns=(st.st_atime_ns, st.st_mtime_ns + 1))


def _dir_mtime_1ns(dst):
    st = os.lstat(dst / "d")
    os.utime(dst / "d", ns=(st.st_atime_ns, st.st_mtime_ns - 1))


def _symlink_mtime(dst):
    os.utime(dst / "d" / "lnk", ns=(1, 1_500_000_000_000_000_002), follow_symlinks=False)


def _xattr_value(dst):
    os.setxattr(dst / "d" / "b.txt", "user.k", b"valuf")


def _xattr_dropped(dst):
    os.removexattr(dst / "d", "user.dir")


def _symlink_target(dst):
    p = dst / "d" / "lnk"
    st = os.lstat(p)
    with _keeping(dst / "d"):
        os.unlink(p)
        os.symlink("c.txt", p)  # same length
        os.utime(p, ns=(st.st_atime_ns, st.st_mtime_ns), follow_symlinks=False)


def _split_hardlink(dst):
    p = dst / "d" / "a-again"
    st = os.lstat(p)
    data = p.read_bytes()
    with _keeping(dst / "d"):
        os.unlink(p)
        p.write_bytes(data)
        os.utime(p, ns=(st.st_atime_ns, st.st_mtime_ns))
        os.chmod(p, st.st_mode & 0o7777)


def _extra(dst):
    with _keeping(dst / "d"):
        (dst / "d" / "zz-extra").write_bytes(b"")


def _missing(dst):
    with _keeping(dst / "d" / "e"):
        os.unlink(dst / "d" / "e" / "c.txt")


def _file_to_symlink(dst):
    p = dst / "d" / "b.txt"
    with _keeping(dst / "d"):
        os.unlink(p)
        os.symlink("e/c.txt", p)


def _fifo_to_file(dst):
    p = dst / "d" / "pipe"
    with _keeping(dst / "d"):
        os.unlink(p)
        p.write_bytes(b"")


MUTATIONS = [
    ("one byte of content", _one_byte, b"a.bin", "sha256"),
    ("mode", _mode, b"d/b.txt", "mode"),
    ("uid", _uid, b"d/b.txt", "uid"),
    ("file mtime by 1 ns", _mtime_1ns, b"a.bin", "mtime"),
    ("directory mtime by 1 ns", _dir_mtime_1ns, b"d", "mtime"),
    ("symlink mtime by 1 ns", _symlink_mtime, b"d/lnk", "mtime"),
    ("xattr value", _xattr_value, b"d/b.txt", "xattrs"),
    ("xattr dropped from a directory", _xattr_dropped, b"d", "xattrs"),
    ("symlink target", _symlink_target, b"d/lnk", "target"),
    ("split hardlink", _split_hardlink, b"a.bin", "links"),
    ("extra entry", _extra, b"d/zz-extra", "extra"),
    ("missing entry", _missing, b"d/e/c.txt", "missing"),
    ("file turned into a symlink", _file_to_symlink, b"d/b.txt", "type"),
    ("fifo turned into a file", _fifo_to_file, b"d/pipe", "type"),
]


@pytest.mark.parametrize("what,mutate,path,field", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_every_single_mutation_is_reported(trees, what, mutate, path, field):
    src, dst = trees
    if field == "uid" and os.geteuid() != 0:
        pytest.skip("chown needs root")
    mutate(dst)
    diff = cr.first_difference(src, dst)
    assert diff is not None, f"comparator is blind to: {what}"
    assert diff[:2] == (path, field), diff
    with pytest.raises(AssertionError) as err:
        cr.assert_same_tree(src, dst)
    assert repr(path) in str(err.value) and field in str(err.value)
    # ... and leaving the field out of the comparison hides exactly that
    if field not in ("extra", "missing", "type"):
        rest = [f for f in cr.FIELDS if f != field]
        assert cr.first_difference(src, dst, fields=rest) is None


def test_mtime_unit_is_the_only_slack(trees):
    src, dst = trees
    st = os.lstat(dst / "a.bin")
    os.utime(dst / "a.bin", ns=(st.st_atime_ns, st.st_mtime_ns - 123_456_789))
    assert cr.first_difference(src, dst)[:2] == (b"a.bin", "mtime")
    assert cr.first_difference(src, dst, mtime_unit_ns=10**9) is None
    os.utime(dst / "a.bin", ns=(st.st_atime_ns, st.st_mtime_ns - 10**9))
    assert cr.first_difference(src, dst, mtime_unit_ns=10**9)[:2] == (b"a.bin", "mtime")


def test_blocks_field_is_opt_in(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    os.makedirs(a)
    os.makedirs(b)
    with open(a / "f", "wb") as f:
        f.truncate(1 << 20)
    (b / "f").write_bytes(bytes(1 << 20))
    st = os.lstat(a / "f")
    os.utime(b / "f", ns=(st.st_atime_ns, st.st_mtime_ns))
    assert cr.first_difference(a, b) is None
    if os.lstat(a / "f").st_blocks != os.lstat(b / "f").st_blocks:
        assert cr.first_difference(a, b, fields=cr.ALL_FIELDS)[:2] == (b"f", "blocks")
