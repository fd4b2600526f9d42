"""Native container lifecycle (csrc/proclife_core.h via ops/proclife.py):
spawn, reap, directory teardown, and its equivalence with the Python path
of runtime/proc.py. No GPU involved; the extension must be built."""
import asyncio
import gc
import json
import os
import signal
import stat
import subprocess
import sys
import time

import pytest

from gpu_docker_api_amd.models.etcd import ContainerSpec
from gpu_docker_api_amd.ops import proclife
from gpu_docker_api_amd.runtime.proc import ProcRuntime
from gpu_docker_api_amd.xerrors import ContainerNotExist

BASE_ENV = {
    "PATH": "/usr/local/bin:/usr/bin:/bin",
    "KEEP": "kept",
    "OVERRIDE_ME": "base",
    "EMPTY_IN_BASE": "",
}


@pytest.fixture
def box(tmp_path):
    """A rootfs dir, a log path and a known base environment; every child
    started through ``box.spawn`` is killed and reaped afterwards."""

    class Box:
        rootfs = tmp_path / "rootfs"
        log = tmp_path / "console.log"
        children = []

        def spawn(self, argv, env=None, cwd=None):
            c = proclife.spawn(argv, str(cwd or self.rootfs), env or {}, str(self.log))
            self.children.append(c)
            return c

    b = Box()
    b.children = []
    b.rootfs.mkdir()
    proclife.set_base_env(dict(BASE_ENV))
    try:
        yield b
    finally:
        for c in b.children:
            if c.poll() is None:
                try:
                    os.killpg(c.pid, signal.SIGKILL)
                except ProcessLookupError:
                    pass
                c.wait(5)
            c.close()
        # the next ProcRuntime re-snapshots its own base
        proclife.set_base_env(dict(os.environ))


def _spec(name, cmd=None, env=None):
    s = ContainerSpec()
    s.config = {"Image": "", "Env": list(env or []), "Cmd": list(cmd or [])}
    s.host_config = {}
    s.container_name = name
    return s


def _my_children():
    """pids whose parent is this process, zombies included."""
    me, out = os.getpid(), set()
    for entry in os.listdir("/proc"):
        if not entry.isdigit():
            continue
        try:
            with open(f"/proc/{entry}/stat") as f:
                fields = f.read().rsplit(") ", 1)[1].split()
        except (OSError, IndexError):
            continue
        if int(fields[1]) == me:
            out.add(int(entry))
    return out


def _fds():
    """Open descriptors of this process. Leak checks compare sets (nothing
    NEW may appear) after a gc.collect(): a descriptor some earlier test
    left to the garbage collector may close at any time."""
    gc.collect()
    out = set()
    for name in os.listdir("/proc/self/fd"):
        try:
            os.readlink(f"/proc/self/fd/{name}")  # skips the listing's own fd
        except OSError:
            continue
        out.add(int(name))
    return out


def _live_group_members(pgid):
    n = 0
    for entry in os.listdir("/proc"):
        if not entry.isdigit():
            continue
        try:
            if os.getpgid(int(entry)) != pgid:
                continue
            with open(f"/proc/{entry}/stat") as f:
                state = f.read().rsplit(") ", 1)[1].split()[0]
        except (OSError, IndexError):
            continue
        if state not in ("Z", "X"):
            n += 1
    return n


def _environ(pid):
    """The child's environment entries. posix_spawn returns as soon as the
    child is past exec's point of no return, a moment before the kernel
    publishes the new image's environ/exe/comm: wait for them to appear."""
    entries = []

    def read():
        with open(f"/proc/{pid}/environ", "rb") as f:
            entries[:] = [e for e in f.read().split(b"\0") if e]
        return bool(entries)

    assert _wait_for(read)
    return entries


def _wait_for(pred, timeout=3.0):
    deadline = time.monotonic() + timeout
    while time.monotonic() < deadline:
        if pred():
            return True
        time.sleep(0.005)
    return pred()


# ------------------------------------------------------------------- spawn
def test_child_is_session_and_group_leader_in_rootfs(box):
    c = box.spawn(["sleep", "30"])
    assert c.pid > 0 and c.fileno() >= 0
    assert os.getsid(c.pid) == c.pid
    assert os.getpgid(c.pid) == c.pid
    assert os.readlink(f"/proc/{c.pid}/cwd") == str(box.rootfs)


def test_environment_is_base_plus_overrides(box):
    over = {
        "OVERRIDE_ME": "new",          # replaces a base key
        "WITH_EQ": "a=b=c",            # value containing '='
        "EMPTY": "",                   # empty value
        "ROCR_VISIBLE_DEVICES": "GPU-0123",
    }
    c = box.spawn(["sleep", "30"], env=over)
    entries = _environ(c.pid)
    got = dict(e.decode().split("=", 1) for e in entries)
    want = dict(BASE_ENV)
    want.update(over)
    assert got == want
    assert len(entries) == len(want)  # no key twice
    # dict.update order: base keys keep their place, new keys are appended
    assert [e.decode().split("=", 1)[0] for e in entries] == list(want)


def test_last_duplicate_override_wins(box):
    c = box.spawn(["sleep", "30"], env=[("A", "1"), ("KEEP", "x"), ("A", "2"), ("KEEP", "y")])
    got = dict(e.decode().split("=", 1) for e in _environ(c.pid))
    assert got["A"] == "2" and got["KEEP"] == "y"


def test_illegal_environment_name_is_rejected(box):
    with pytest.raises(ValueError):
        box.spawn(["sleep", "30"], env={"A=B": "x"})


def test_stdout_and_stderr_append_to_the_log(box):
    c = box.spawn(["sh", "-c", "echo out; echo err >&2"])
    assert c.wait(5) == 0
    assert box.log.read_text() == "out\nerr\n"
    c2 = box.spawn(["sh", "-c", "echo out2; echo err2 >&2"])  # a second container
    assert c2.wait(5) == 0
    assert box.log.read_text() == "out\nerr\nout2\nerr2\n"


def test_inheritable_parent_descriptor_does_not_leak(box):
    r, w = os.pipe()
    try:
        os.set_inheritable(r, True)
        os.set_inheritable(w, True)
        c = box.spawn(["sleep", "30"])
        fds = sorted(int(x) for x in os.listdir(f"/proc/{c.pid}/fd"))
        assert fds == [0, 1, 2]
        assert os.readlink(f"/proc/{c.pid}/fd/1") == str(box.log)
        assert os.readlink(f"/proc/{c.pid}/fd/2") == str(box.log)
        assert os.readlink(f"/proc/{c.pid}/fd/0") == os.readlink("/proc/self/fd/0")
    finally:
        os.close(r)
        os.close(w)


def test_bare_name_resolves_through_the_childs_path(box, tmp_path):
    tools = tmp_path / "tools"
    tools.mkdir()
    tool = tools / "only-in-child-path"
    tool.write_text("#!/bin/sh\necho from-tool\n")
    tool.chmod(0o755)
    assert "only-in-child-path" not in os.listdir("/usr/bin")
    c = box.spawn(["only-in-child-path"], env={"PATH": f"/nonexistent:{tools}:/usr/bin:/bin"})
    assert c.wait(5) == 0
    assert box.log.read_text() == "from-tool\n"
    # plain `sleep` comes from the child's PATH too
    c = box.spawn(["sleep", "30"], env={"PATH": "/usr/bin:/bin"})
    assert _wait_for(
        lambda: os.path.basename(os.readlink(f"/proc/{c.pid}/exe"))
        in ("sleep", "coreutils", "busybox")
    )
    # ... and is not found when that PATH does not have it
    with pytest.raises(FileNotFoundError):
        box.spawn(["sleep", "30"], env={"PATH": str(tools)})


def test_name_with_slash_resolves_relative_to_cwd(box):
    tool = box.rootfs / "tool"
    tool.write_text("#!/bin/sh\necho relative-tool\n")
    tool.chmod(0o755)
    c = box.spawn(["./tool"])
    assert c.wait(5) == 0
    assert box.log.read_text() == "relative-tool\n"


def test_failed_spawns_raise_and_leak_nothing(box):
    noexec = box.rootfs / "noexec"
    noexec.write_text("#!/bin/sh\n")
    noexec.chmod(0o644)
    with pytest.raises(FileNotFoundError):
        box.spawn(["no-such-command-anywhere"])
    with pytest.raises(FileNotFoundError):
        box.spawn(["/no/such/dir/binary"])
    with pytest.raises(PermissionError):
        box.spawn(["./noexec"])
    with pytest.raises(FileNotFoundError) as ei:
        box.spawn(["sleep", "1"], cwd=box.rootfs / "missing")
    assert ei.value.filename == str(box.rootfs / "missing")

    fds, kids = _fds(), _my_children()
    for i in range(200):
        with pytest.raises(OSError):
            box.spawn(["./noexec"] if i % 2 else ["no-such-command-anywhere"])
    for _ in range(200):
        c = proclife.spawn(["true"], str(box.rootfs), {}, str(box.log))
        assert c.wait(5) == 0
        c.close()
    assert _fds() - fds == set()
    assert _my_children() == kids


def test_dropped_running_child_is_reaped_later(box):
    kids = _my_children()
    c = proclife.spawn(["sleep", "30"], str(box.rootfs), {}, str(box.log))
    pid = c.pid
    del c  # still running: goes on the orphan list, descriptor closed
    os.killpg(pid, signal.SIGKILL)
    assert _wait_for(lambda: open(f"/proc/{pid}/stat").read().rsplit(") ", 1)[1][0] == "Z")
    proclife.spawn(["true"], str(box.rootfs), {}, str(box.log)).wait(5)  # next spawn reaps it
    assert not os.path.exists(f"/proc/{pid}")
    assert _my_children() == kids


def test_starttime_matches_proc_stat(box):
    c = box.spawn(["sleep", "30"])
    assert c.starttime > 0
    assert c.starttime == ProcRuntime._proc_stat(c.pid)[1]
    assert proclife.proc_starttime(c.pid) == c.starttime
    # comm containing ") " must not confuse the parse
    sleep_path = next(p for p in ("/usr/bin/sleep", "/bin/sleep") if os.path.exists(p))
    os.symlink(sleep_path, box.rootfs / "we ird) x")
    c2 = box.spawn(["./we ird) x", "30"])
    assert _wait_for(lambda: "(we ird) x)" in open(f"/proc/{c2.pid}/stat").read())
    assert c2.starttime > 0
    assert c2.starttime == ProcRuntime._proc_stat(c2.pid)[1]
    # gone / zombie: no identity, as _proc_stat
    os.killpg(c2.pid, signal.SIGKILL)
    assert _wait_for(lambda: ProcRuntime._proc_stat(c2.pid)[1] is None)
    assert proclife.proc_starttime(c2.pid) == 0


# -------------------------------------------------------------------- reap
def test_poll_and_close_are_idempotent(box):
    c = box.spawn(["sleep", "30"])
    assert c.poll() is None and c.returncode is None
    os.kill(c.pid, signal.SIGTERM)
    assert c.wait(5) == -signal.SIGTERM
    assert c.poll() == -signal.SIGTERM and c.poll() == -signal.SIGTERM
    assert c.returncode == -signal.SIGTERM
    c.close()
    c.close()
    assert c.fileno() == -1
    assert c.poll() == -signal.SIGTERM


def test_stop_awaits_the_pidfd_without_sleeping(tmp_path, run, monkeypatch):
    async def main():
        rt = ProcRuntime(base_dir=str(tmp_path), use_cgroups=False, native=True)
        await rt.create(_spec("c-1", cmd=["sleep", "30"]))
        await rt.start("c-1")
        child = rt._procs["c-1"].popen
        assert not isinstance(child, subprocess.Popen)
        assert child.poll() is None
        fd = child.fileno()
        await asyncio.sleep(0.01)  # park the supervisor task in its own sleep

        sleeps = []
        real_sleep = asyncio.sleep

        async def recording_sleep(delay, *a, **kw):
            sleeps.append(delay)
            return await real_sleep(delay, *a, **kw)

        monkeypatch.setattr(asyncio, "sleep", recording_sleep)
        await rt.stop("c-1")
        monkeypatch.setattr(asyncio, "sleep", real_sleep)
        assert sleeps == [], f"stop() slept: {sleeps}"
        assert child.poll() == -signal.SIGTERM
        loop = asyncio.get_running_loop()
        assert loop.remove_reader(fd) is False  # nothing left registered
        assert rt._procs["c-1"].exit_waiters == []
        st = await rt.inspect("c-1")
        assert not st.running and st.pid == 0
        # a second stop and a second remove are harmless
        await rt.stop("c-1")
        await rt.remove("c-1")
        with pytest.raises(ContainerNotExist):
            await rt.remove("c-1")
        assert not os.path.exists(tmp_path / "containers" / "c-1")
        await rt.close()

    run(main())


def test_concurrent_stops_share_one_reader(tmp_path, run):
    async def main():
        rt = ProcRuntime(base_dir=str(tmp_path), use_cgroups=False, native=True)
        await rt.create(_spec("c-1", cmd=["sleep", "30"]))
        await rt.start("c-1")
        p = rt._procs["c-1"]
        fd = p.popen.fileno()
        await asyncio.wait_for(asyncio.gather(rt.stop("c-1"), rt.stop("c-1")), 5)
        assert p.popen.poll() == -signal.SIGTERM
        assert p.exit_waiters == []
        assert asyncio.get_running_loop().remove_reader(fd) is False
        await rt.close()

    run(main())


def test_term_ignoring_container_is_killed_and_group_swept(tmp_path, run):
    async def main():
        rt = ProcRuntime(base_dir=str(tmp_path), use_cgroups=False, native=True)
        await rt.create(
            _spec("c-1", cmd=["sh", "-c", 'trap "" TERM; sleep 30 & echo ready; sleep 30'])
        )
        await rt.start("c-1")
        p = rt._procs["c-1"]
        pgid, fd = p.popen.pid, p.popen.fileno()
        log = tmp_path / "containers" / "c-1" / "console.log"
        assert _wait_for(lambda: log.exists() and "ready" in log.read_text())
        assert _live_group_members(pgid) >= 2
        t0 = time.monotonic()
        await rt.stop("c-1", timeout=0.2)
        took = time.monotonic() - t0
        assert 0.2 <= took < 2.0, took  # waited the timeout out, then SIGKILL
        assert p.popen.poll() == -signal.SIGKILL
        assert _wait_for(lambda: _live_group_members(pgid) == 0), "group survived stop"
        assert asyncio.get_running_loop().remove_reader(fd) is False
        await rt.close()

    run(main())


def test_cancelled_stop_removes_its_reader(tmp_path, run):
    async def main():
        rt = ProcRuntime(base_dir=str(tmp_path), use_cgroups=False, native=True)
        await rt.create(_spec("c-1", cmd=["sh", "-c", 'trap "" TERM; echo ready; sleep 30']))
        await rt.start("c-1")
        p = rt._procs["c-1"]
        fd = p.popen.fileno()
        log = tmp_path / "containers" / "c-1" / "console.log"
        assert _wait_for(lambda: log.exists() and "ready" in log.read_text())
        task = asyncio.ensure_future(rt.stop("c-1", timeout=30))
        await asyncio.sleep(0.02)
        assert p.exit_waiters  # parked on the pidfd
        task.cancel()
        with pytest.raises(asyncio.CancelledError):
            await task
        assert p.exit_waiters == []
        assert asyncio.get_running_loop().remove_reader(fd) is False
        os.killpg(p.popen.pid, signal.SIGKILL)  # TERM is ignored: do not wait remove()'s timeout out
        await rt.remove("c-1")
        await rt.close()

    run(main())


def test_sigstopped_container_stops(tmp_path, run):
    async def main():
        rt = ProcRuntime(base_dir=str(tmp_path), use_cgroups=False, native=True)
        await rt.create(_spec("c-1", cmd=["sleep", "30"]))
        await rt.start("c-1")
        await rt.pause("c-1")
        p = rt._procs["c-1"]
        assert ProcRuntime._proc_stat(p.popen.pid)[0] in ("T", "t")
        await asyncio.wait_for(rt.stop("c-1", timeout=3), 2)
        assert p.popen.poll() == -signal.SIGTERM
        await rt.close()

    run(main())


# ------------------------------------------------------------- remove_tree
def test_remove_tree_removes_everything(tmp_path):
    root = tmp_path / "tree"
    (root / "a" / "b" / "c").mkdir(parents=True)
    (root / "a" / "f1").write_text("x")
    (root / "a" / "b" / "f2").write_text("yy")
    os.link(root / "a" / "f1", root / "a" / "b" / "c" / "hard")
    os.link(root / "a" / "f1", root / "hard2")
    os.symlink("/nonexistent/target", root / "a" / "dangling")
    (root / "locked").write_text("z")
    os.chmod(root / "locked", 0)
    (root / "empty").mkdir()
    assert proclife.remove_tree(str(root)) == 0
    assert not os.path.lexists(root)
    assert os.listdir(tmp_path) == []


def test_remove_tree_never_follows_symlinks(tmp_path):
    outside = tmp_path / "outside"
    (outside / "sub").mkdir(parents=True)
    (outside / "keep.txt").write_text("keep")
    (outside / "sub" / "keep2.txt").write_text("keep2")
    root = tmp_path / "tree"
    root.mkdir()
    os.symlink(outside, root / "link")
    os.symlink(outside / "keep.txt", root / "filelink")
    assert proclife.remove_tree(str(root)) == 0
    assert not os.path.lexists(root)
    assert (outside / "keep.txt").read_text() == "keep"
    assert (outside / "sub" / "keep2.txt").read_text() == "keep2"

    # path itself a symlink to a directory: nothing is removed (as rmtree)
    rootlink = tmp_path / "rootlink"
    os.symlink(outside, rootlink)
    assert proclife.remove_tree(str(rootlink)) == 1
    assert os.path.islink(rootlink)
    assert (outside / "keep.txt").read_text() == "keep"
    assert (outside / "sub" / "keep2.txt").read_text() == "keep2"


def test_remove_tree_missing_path_is_a_noop(tmp_path):
    assert proclife.remove_tree(str(tmp_path / "never-existed")) == 0
    assert os.listdir(tmp_path) == []


def test_remove_tree_deeper_than_path_max(tmp_path):
    root = tmp_path / "deep"
    root.mkdir()
    seg = "d" * 100
    fd = os.open(root, os.O_RDONLY | os.O_DIRECTORY)
    try:
        for _ in range(60):
            os.mkdir(seg, dir_fd=fd)
            os.close(os.open("f", os.O_WRONLY | os.O_CREAT, 0o644, dir_fd=fd))
            nxt = os.open(seg, os.O_RDONLY | os.O_DIRECTORY, dir_fd=fd)
            os.close(fd)
            fd = nxt
    finally:
        os.close(fd)
    assert 60 * 101 > os.pathconf("/", "PC_PATH_MAX")
    fds = _fds()
    assert proclife.remove_tree(str(root)) == 0
    assert not os.path.lexists(root)
    assert _fds() - fds == set()


def test_remove_tree_counts_what_it_cannot_remove(tmp_path):
    if os.geteuid() == 0:
        # root ignores directory permissions: use a regular file as the path
        f = tmp_path / "plain"
        f.write_text("x")
        assert proclife.remove_tree(str(f)) == 1  # not a directory: refused, as rmtree
        assert f.read_text() == "x"
        return
    root = tmp_path / "tree"
    (root / "ro").mkdir(parents=True)
    (root / "ro" / "stuck").write_text("x")
    os.chmod(root / "ro", stat.S_IRUSR | stat.S_IXUSR)
    try:
        assert proclife.remove_tree(str(root)) >= 1
        assert (root / "ro" / "stuck").exists()
    finally:
        os.chmod(root / "ro", 0o755)


# ------------------------------------------------------------- small files
def test_prepare_container_dir_and_write_file(tmp_path):
    cdir = tmp_path / "containers" / "c-1"
    proclife.prepare_container_dir(str(cdir), '{"k": "vé"}')
    assert (cdir / "rootfs").is_dir()
    assert json.loads((cdir / "spec.json").read_text(encoding="utf-8")) == {"k": "vé"}
    proclife.prepare_container_dir(str(cdir), "{}")  # exists already: rewritten, no error
    assert (cdir / "spec.json").read_text() == "{}"
    proclife.write_file(str(cdir / "meta.json"), '{"pid": 1}')
    proclife.write_file(str(cdir / "meta.json"), "{}")  # truncates
    assert (cdir / "meta.json").read_text() == "{}"
    mode = stat.S_IMODE(os.stat(cdir / "meta.json").st_mode)
    um = os.umask(0)
    os.umask(um)
    assert mode == 0o666 & ~um
    with pytest.raises(FileNotFoundError):
        proclife.write_file(str(tmp_path / "no-dir" / "x"), "x")
    (tmp_path / "file").write_text("x")
    with pytest.raises(OSError):
        proclife.prepare_container_dir(str(tmp_path / "file" / "c"), "{}")


# ------------------------------------------------------------- equivalence
def _listing(base):
    out = {}
    for root, dirs, files in os.walk(base):
        for n in dirs + files:
            full = os.path.join(root, n)
            kind = "link" if os.path.islink(full) else "dir" if os.path.isdir(full) else "file"
            out[os.path.relpath(full, base)] = kind
    return out


def _shape(obj):
    return {k: type(v).__name__ for k, v in obj.items()}


def _lifecycle(base_dir, native):
    """create -> start -> rolling replace (create+start v2, remove v1) ->
    stop -> delete; returns everything observable."""
    seen = {"states": [], "listings": [], "spec": None, "meta": []}

    async def main():
        rt = ProcRuntime(base_dir=str(base_dir), use_cgroups=False, native=native)
        assert (rt._nat is not None) == native

        async def snap(name):
            st = await rt.inspect(name)
            seen["states"].append(
                None if st is None else (st.name, st.status, st.running, st.paused, st.pid > 0)
            )
            seen["listings"].append(_listing(base_dir))

        def meta(name):
            with open(os.path.join(base_dir, "containers", name, "meta.json")) as f:
                seen["meta"].append(_shape(json.load(f)))

        env = ["FOO=bar", "X=a=b"]
        await rt.create(_spec("rs-1", cmd=["sh", "-c", "echo hello; exec sleep 30"], env=env))
        await snap("rs-1")
        await rt.start("rs-1")
        assert isinstance(rt._procs["rs-1"].popen, subprocess.Popen) != native
        await snap("rs-1")
        meta("rs-1")
        with open(os.path.join(base_dir, "containers", "rs-1", "spec.json")) as f:
            seen["spec"] = _shape(json.load(f))
        await rt.create(_spec("rs-2", cmd=["sleep", "30"], env=env))
        await snap("rs-2")
        await rt.start("rs-2")
        await snap("rs-2")
        await rt.remove("rs-1", force=True)
        await snap("rs-1")
        await rt.pause("rs-2")
        await snap("rs-2")
        await rt.unpause("rs-2")
        await snap("rs-2")
        await rt.stop("rs-2")
        await snap("rs-2")
        meta("rs-2")
        await rt.remove("rs-2", force=True)
        await snap("rs-2")
        await rt.close()

    asyncio.run(main())
    return seen


def test_native_and_python_paths_are_equivalent(tmp_path):
    native = _lifecycle(tmp_path / "native", True)
    python = _lifecycle(tmp_path / "python", False)
    assert native["states"] == python["states"]
    assert native["listings"] == python["listings"]
    assert native["spec"] == python["spec"] and native["spec"]
    assert native["meta"] == python["meta"] and len(native["meta"]) == 2
    assert native["listings"][-1] == {"containers": "dir", "volumes": "dir",
                                      "images": "dir", "trash": "dir"}


def test_environment_switch_forces_the_python_path():
    code = (
        "from gpu_docker_api_amd.runtime import proc; "
        "from gpu_docker_api_amd.ops import proclife; "
        "print(proc.NATIVE_LIFECYCLE, proclife.available())"
    )
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for value in ("0", "1"):
        env = dict(os.environ, GDA_NATIVE_LIFECYCLE=value, PYTHONPATH=root)
        outs.append(
            subprocess.run([sys.executable, "-c", code], env=env, capture_output=True,
                           text=True, check=True).stdout.split()
        )
    assert outs == [["False", "True"], ["True", "True"]]
