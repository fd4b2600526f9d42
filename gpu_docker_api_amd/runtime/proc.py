"""Native process runtime ("proc").

A lightweight container runtime with no dockerd dependency: each container is
a supervised host process group with

* a private rootfs directory (materialized from the image store) that plays
  the role of the overlay2 writable layer — migration/commit operate on it
  exactly like the docker driver's UpperDir
  (/root/reference/utils/copy.go:48-54);
* GPU isolation via ``ROCR_VISIBLE_DEVICES``/``HIP_VISIBLE_DEVICES`` computed
  from the allocated GPU UUIDs — the ROCm-native equivalent of device
  injection, enforced by the ROCm runtime itself;
* best-effort cgroup-v2 limits (memory.max, cpuset.cpus) when the daemon may
  write /sys/fs/cgroup;
* volumes as directories "bound" into the rootfs by symlink.

This is what runs on dockerd-less MI355X boxes (gpurun, bench.py): the
control-plane latency being measured — schedule → materialize → spawn →
running — is real work, not a stub.

Processes are stopped by exact PID/process-group only (never by pattern).
"""
from __future__ import annotations

import asyncio
import json
import logging
import os
import shutil
import signal
import subprocess
import time
import uuid as uuidlib
from typing import Dict, List, Optional

from ..models.etcd import ContainerSpec
from ..ops import proclife
from ..utils.names import safe_subpath
from ..xerrors import ContainerExisted, ContainerNotExist, VolumeExisted
from .base import ContainerState, GpuResolver, RuntimeDriver, VolumeState
from .devices import visible_device_env

log = logging.getLogger(__name__)

CGROUP_ROOT = "/sys/fs/cgroup"
DEFAULT_CMD = ["sleep", "infinity"]

# spawn/reap/teardown run in ops/_proclife.so when it is built and
# GDA_NATIVE_LIFECYCLE does not force the Python path (ops/proclife.py)
NATIVE_LIFECYCLE = proclife.enabled()
if proclife.ENABLED and not NATIVE_LIFECYCLE:  # never a silent fallback
    log.warning("native lifecycle module not loaded (%s): using the Python path",
                proclife.load_error())


class _Proc:
    def __init__(self, state: ContainerState, spec: ContainerSpec) -> None:
        self.state = state
        self.spec = spec
        # a subprocess.Popen or a native proclife Child: only .pid and
        # .poll() are used (plus .fileno() on a Child, to await its exit)
        self.popen = None
        self.cgroup: Optional[str] = None
        # restart policy (reference containers run unless-stopped,
        # services/replicaset.go:73-75; dockerd enforces it there — here the
        # supervisor task does)
        self.restart_policy: str = (
            (spec.host_config.get("RestartPolicy") or {}).get("Name", "") or "no"
        )
        self.manually_stopped = False
        self.restarts = 0
        # crash-loop backoff (docker semantics: delay doubles per prompt
        # death, resets after a stable run)
        self.next_restart_at = 0.0
        self.last_start_at = 0.0
        # daemon-restart reattachment: leader pid + its /proc starttime
        # (detects pid reuse) for containers adopted without a Popen handle
        self.attached_pid = 0
        self.attached_start = 0
        self.was_started = False
        self.start_ticks = 0  # cached /proc starttime of the live leader
        # futures of the stop() calls awaiting the leader's exit on its pidfd
        # (one loop reader serves them all: add_reader keeps one per fd)
        self.exit_waiters: List[asyncio.Future] = []


class ProcRuntime(RuntimeDriver):
    owns_rootfs = True

    def __init__(
        self,
        base_dir: str = "",
        gpu_resolver: Optional[GpuResolver] = None,
        use_cgroups: bool = True,
        loop_volumes: bool = False,
        native: Optional[bool] = None,
    ) -> None:
        # native=False forces the Python lifecycle path for this runtime,
        # None follows the module default
        if native is None:
            native = NATIVE_LIFECYCLE
        self._nat = proclife if native and proclife.available() else None
        self.base = base_dir or os.path.join(os.getcwd(), ".state", "procrt")
        for sub in ("containers", "volumes", "images", "trash"):
            os.makedirs(os.path.join(self.base, sub), exist_ok=True)
        self.gpu_resolver: GpuResolver = gpu_resolver or (lambda _u: None)
        self.use_cgroups = use_cgroups
        # loop-device quota enforcement is OPT-IN: mounts outlive the
        # process, so only long-lived daemons should create them
        self.loop_volumes = loop_volumes
        self._procs: Dict[str, _Proc] = {}
        self.volumes: Dict[str, VolumeState] = {}
        self._supervisor: Optional[asyncio.Task] = None

        self._load_volumes()
        self._load_containers()
        try:  # adopt/resurrect across daemon restarts when a loop exists
            asyncio.get_running_loop()
            if self._procs:
                self._ensure_supervisor()
        except RuntimeError:
            pass

    # -------------------------------------------------------------- supervisor
    def _ensure_supervisor(self) -> None:
        if self._supervisor is None or self._supervisor.done():
            self._supervisor = asyncio.get_running_loop().create_task(
                self._supervise_loop()
            )

    async def _supervise_loop(self) -> None:
        """Enforce restart policies: a container whose process died (and was
        not stopped through the API) is restarted when its policy is
        'always' or 'unless-stopped'."""
        while True:
            await asyncio.sleep(0.2)
            for name, p in list(self._procs.items()):
                self._refresh(p)
                if (
                    not p.state.running
                    and p.state.status == "exited"
                    and not p.manually_stopped
                    and p.restart_policy in ("always", "unless-stopped")
                    and (p.popen is not None or p.was_started)
                ):
                    now = time.monotonic()
                    if now < p.next_restart_at:
                        continue
                    # exponential crash-loop backoff (docker: 100 ms
                    # doubling, capped; reset after >=10 s of stable run)
                    if p.last_start_at and now - p.last_start_at >= 10.0:
                        p.restarts = 0
                    delay = min(0.1 * (2 ** min(p.restarts, 8)), 30.0)
                    p.next_restart_at = now + delay
                    try:
                        p.restarts += 1
                        await self.start(name)
                    except Exception:  # noqa: BLE001 — keep supervising
                        pass

    # ------------------------------------------------------------------ util
    def _cdir(self, name: str) -> str:
        # containment-checked: these paths feed rmtree
        return safe_subpath(os.path.join(self.base, "containers"), name)

    def _vdir(self, name: str) -> str:
        return safe_subpath(os.path.join(self.base, "volumes"), name)

    def _image_dir(self, ref: str) -> str:
        return safe_subpath(
            os.path.join(self.base, "images"), ref.replace("/", "_").replace(":", "_")
        )

    def _load_volumes(self) -> None:
        vroot = os.path.join(self.base, "volumes")
        for name in os.listdir(vroot):
            mp = os.path.join(vroot, name, "_data")
            optf = os.path.join(vroot, name, "opts.json")
            opts = {}
            if os.path.exists(optf):
                try:
                    opts = json.load(open(optf))
                except Exception:
                    opts = {}
            if os.path.isdir(mp):
                img = os.path.join(vroot, name, "volume.img")
                if (
                    opts.get("enforced") == "loop"
                    and os.path.exists(img)
                    and not os.path.ismount(mp)
                ):
                    # daemon restart: re-attach the loop-backed volume
                    rc = subprocess.run(
                        ["mount", "-o", "loop", img, mp],
                        stdout=subprocess.DEVNULL,
                        stderr=subprocess.DEVNULL,
                    ).returncode
                    if rc != 0:
                        # quota silently becoming advisory is a lie to the
                        # API — record the degradation so volume info can
                        # surface it
                        opts["enforced"] = "none"
                        opts["degraded"] = "remount-failed"
                        log.warning(
                            "volume %s: loop remount failed; size quota now advisory", name
                        )
                        try:
                            with open(optf, "w") as f:
                                json.dump(opts, f)
                        except OSError:
                            pass
                self.volumes[name] = VolumeState(name=name, mountpoint=mp, options=opts)

    @staticmethod
    def _proc_stat(pid: int):
        """(state_char, starttime) of a pid, or (None, None). starttime
        (clock ticks since boot) is the stable identity that survives pid
        reuse; zombies (Z — dead but unreaped by their original parent,
        which may have been the previous daemon's popen) count as gone."""
        try:
            with open(f"/proc/{pid}/stat") as f:
                fields = f.read().rsplit(") ", 1)[1].split()
                if fields[0] in ("Z", "X"):
                    return None, None
                return fields[0], int(fields[19])
        except (OSError, IndexError, ValueError):
            return None, None

    @classmethod
    def _proc_starttime(cls, pid: int) -> Optional[int]:
        return cls._proc_stat(pid)[1]

    def _alive(self, p: _Proc) -> bool:
        if p.popen is not None:
            return p.popen.poll() is None
        if p.attached_pid:
            return self._proc_starttime(p.attached_pid) == p.attached_start
        return False

    def _leader_pid(self, p: _Proc) -> int:
        if p.popen is not None:
            return p.popen.pid
        return p.attached_pid

    def _refresh(self, p: _Proc) -> None:
        if p.state.running and not self._alive(p):
            p.state.running = False
            p.state.status = "exited"
            p.state.pid = 0
            p.attached_pid = 0
            self._write_meta(p)

    def _write_meta(self, p: _Proc) -> None:
        """Persist runtime identity next to spec.json so a daemon restart
        can adopt still-running containers (dockerd containers survive the
        daemon; round 1's proc runtime forgot everything)."""
        try:
            meta = {
                "id": p.state.id,
                "pid": self._leader_pid(p) if p.state.running else 0,
                "starttime": p.start_ticks if p.state.running else 0,
                "running": p.state.running,
                "restarts": p.restarts,
            }
            path = os.path.join(self._cdir(p.state.name), "meta.json")
            if self._nat is not None:
                self._nat.write_file(path, json.dumps(meta))
            else:
                with open(path, "w") as f:
                    json.dump(meta, f)
        except OSError:
            pass

    def _load_containers(self) -> None:
        # crash leftovers from deferred deletion (and legacy in-place
        # .deleting renames) are finished here
        trash = os.path.join(self.base, "trash")
        for entry in os.listdir(trash):
            shutil.rmtree(os.path.join(trash, entry), ignore_errors=True)
        croot = os.path.join(self.base, "containers")
        for name in sorted(os.listdir(croot)):
            if ".deleting-" in name:
                shutil.rmtree(os.path.join(croot, name), ignore_errors=True)
                continue
            specf = os.path.join(croot, name, "spec.json")
            if not os.path.isfile(specf):
                continue
            try:
                spec = ContainerSpec.deserialize(open(specf).read())
            except Exception:
                continue
            meta = {}
            try:
                meta = json.load(open(os.path.join(croot, name, "meta.json")))
            except Exception:
                pass
            rootfs = os.path.join(croot, name, "rootfs")
            st = ContainerState(
                id=meta.get("id", ""),
                name=name,
                image=spec.image,
                status="exited",
                env=list(spec.env),
                gpu_uuids=list(spec.gpu_uuids),
                cpuset_cpus=spec.cpuset_cpus,
                memory=spec.memory_bytes,
                port_bindings=dict(spec.host_config.get("PortBindings") or {}),
                upper_dir=rootfs,
                binds=list(spec.host_config.get("Binds") or []),
            )
            p = _Proc(st, spec)
            p.restarts = int(meta.get("restarts", 0) or 0)
            pid = int(meta.get("pid", 0) or 0)
            if meta.get("running") and pid:
                if self._proc_starttime(pid) == meta.get("starttime"):
                    # the workload outlived the daemon: adopt it live
                    p.attached_pid = pid
                    p.attached_start = int(meta["starttime"])
                    p.start_ticks = p.attached_start
                    p.was_started = True
                    # treat adoption as a fresh stable-run baseline so a
                    # later death gets normal (not stale) backoff
                    p.last_start_at = time.monotonic()
                    st.pid = pid
                    st.running = True
                    # a SIGSTOPped group adopts as paused, not running
                    state_char = self._proc_stat(pid)[0]
                    if state_char in ("T", "t"):
                        st.paused, st.status = True, "paused"
                    else:
                        st.status = "running"
                else:
                    # it died while unsupervised; the restart policy decides
                    # whether the supervisor resurrects it (docker restarts
                    # unless-stopped containers on daemon start, without
                    # carrying the previous daemon's crash-loop backoff)
                    p.restarts = 0
                    p.was_started = True
                    p.manually_stopped = False
            else:
                p.manually_stopped = True
            self._procs[name] = p

    # ------------------------------------------------------------ containers
    async def create(self, spec: ContainerSpec) -> str:
        name = spec.container_name
        if name in self._procs:
            raise ContainerExisted(name)
        cid = uuidlib.uuid4().hex[:12]
        cdir = self._cdir(name)
        rootfs = os.path.join(cdir, "rootfs")
        seed = self._image_dir(spec.image) if spec.image else ""
        seeded = bool(seed) and os.path.isdir(seed)
        binds = list(spec.host_config.get("Binds") or [])
        # nothing to materialize (the common case): the native module makes
        # the directories and writes spec.json in one call further down
        one_call = self._nat is not None and not seeded and not binds
        if not one_call:
            os.makedirs(rootfs, exist_ok=True)
        if seeded:
            # image materialization can be large: off the event loop
            await asyncio.get_running_loop().run_in_executor(
                None, lambda: shutil.copytree(seed, rootfs, dirs_exist_ok=True)
            )
        # bind volumes/host dirs into the rootfs by symlink
        for b in binds:
            src, _, dest = b.partition(":")
            dest = dest.split(":")[0]
            if not src or not dest:
                continue
            vol = self.volumes.get(src)
            src_path = vol.mountpoint if vol else src
            link = os.path.join(rootfs, dest.lstrip("/"))
            os.makedirs(os.path.dirname(link), exist_ok=True)
            if not os.path.lexists(link):
                os.symlink(src_path, link)
        st = ContainerState(
            id=cid,
            name=name,
            image=spec.image,
            status="created",
            env=list(spec.env),
            gpu_uuids=list(spec.gpu_uuids),
            cpuset_cpus=spec.cpuset_cpus,
            memory=spec.memory_bytes,
            port_bindings=dict(spec.host_config.get("PortBindings") or {}),
            upper_dir=rootfs,
            binds=binds,
        )
        p = _Proc(st, spec)
        if one_call:
            self._nat.prepare_container_dir(cdir, spec.serialize())
        self._procs[name] = p
        if self._nat is None:
            with open(os.path.join(cdir, "spec.json"), "w") as f:
                f.write(spec.serialize())
        elif not one_call:
            self._nat.write_file(os.path.join(cdir, "spec.json"), spec.serialize())
        # meta (pid identity) is written at start(); a created-not-started
        # container needs none
        return cid

    def _get(self, name: str) -> _Proc:
        if name not in self._procs:
            raise ContainerNotExist(name)
        return self._procs[name]

    _base_env: Optional[Dict[str, str]] = None

    @staticmethod
    def _base_snapshot() -> Dict[str, str]:
        # snapshot os.environ once: copying ~100 vars per container start
        # showed up in the cycle CPU profile
        if ProcRuntime._base_env is None:
            ProcRuntime._base_env = dict(os.environ)
        return ProcRuntime._base_env

    def _env_overrides(self, p: _Proc) -> Dict[str, str]:
        """What a container's environment adds to the base: the visible
        device variables, then the spec's Env (later entries win)."""
        env = dict(visible_device_env(p.state.gpu_uuids, self.gpu_resolver))
        for e in p.state.env:
            k, _, v = e.partition("=")
            env[k] = v
        return env

    def _env_for(self, p: _Proc) -> Dict[str, str]:
        env = dict(self._base_snapshot())
        env.update(self._env_overrides(p))
        return env

    def _spawn_native(self, name: str, p: _Proc, cmd: List[str]):
        # the base environment is encoded once inside the module; a spawn
        # carries only the overrides and the merge happens natively
        base = self._base_snapshot()
        if not self._nat.base_env_is(base):
            self._nat.set_base_env(base)
        return self._nat.spawn(
            cmd,
            p.state.upper_dir,
            self._env_overrides(p),
            os.path.join(self._cdir(name), "console.log"),
        )

    @staticmethod
    def _enable_controllers(path: str) -> None:
        """cgroup v2: child limits only work when the parent delegates the
        controllers (+memory +cpuset in cgroup.subtree_control)."""
        ctrl_file = os.path.join(path, "cgroup.subtree_control")
        avail_file = os.path.join(path, "cgroup.controllers")
        try:
            with open(avail_file) as f:
                avail = set(f.read().split())
            want = [c for c in ("memory", "cpuset") if c in avail]
            for c in want:  # one at a time: a single EINVAL must not kill both
                try:
                    with open(ctrl_file, "w") as f:
                        f.write(f"+{c}")
                except OSError:
                    pass
        except OSError:
            pass

    def _setup_cgroup(self, name: str, p: _Proc, pid: int) -> None:
        if not self.use_cgroups:
            return
        parent = os.path.join(CGROUP_ROOT, "gda")
        cg = os.path.join(parent, name)
        try:
            self._enable_controllers(CGROUP_ROOT)
            os.makedirs(parent, exist_ok=True)
            self._enable_controllers(parent)
            os.makedirs(cg, exist_ok=True)
            if p.state.memory > 0:
                with open(os.path.join(cg, "memory.max"), "w") as f:
                    f.write(str(p.state.memory))
            if p.state.cpuset_cpus:
                with open(os.path.join(cg, "cpuset.cpus"), "w") as f:
                    f.write(p.state.cpuset_cpus)
            mems = p.spec.host_config.get("CpusetMems", "")
            if mems:
                try:
                    with open(os.path.join(cg, "cpuset.mems"), "w") as f:
                        f.write(mems)
                except OSError:
                    pass  # node went away / not delegated: cpus still bound
            with open(os.path.join(cg, "cgroup.procs"), "w") as f:
                f.write(str(pid))
            p.cgroup = cg
        except OSError:
            p.cgroup = None  # best-effort: not permitted in this environment

    async def start(self, name: str) -> None:
        p = self._get(name)
        self._refresh(p)
        p.manually_stopped = False
        self._ensure_supervisor()
        if p.state.running:
            return
        cmd = list(p.spec.config.get("Cmd") or []) or DEFAULT_CMD
        # spawn inline: fork+exec is ~0.7 ms; offloading it to an executor
        # (shared pool in round 1: 109 -> 71 cycles/s; a DEDICATED 2-thread
        # pool re-measured in round 2: 256 -> 211 single-tenant, 258 -> 243
        # at 8 tenants, bench p50 4.5 -> 5.0 ms) loses more to the thread
        # hop than the freed loop time buys — keep it inline
        if self._nat is not None:
            # vfork+execve, pidfd and the /proc start time in one native call
            p.popen = self._spawn_native(name, p, cmd)
            start_ticks = p.popen.starttime
        else:
            logf = open(os.path.join(self._cdir(name), "console.log"), "ab")
            try:
                p.popen = subprocess.Popen(
                    cmd,
                    cwd=p.state.upper_dir,
                    env=self._env_for(p),
                    stdout=logf,
                    stderr=subprocess.STDOUT,
                    start_new_session=True,  # own pgid: exact-target signalling
                )
            finally:
                logf.close()
            start_ticks = self._proc_starttime(p.popen.pid) or 0
        p.attached_pid = 0
        p.was_started = True
        p.last_start_at = time.monotonic()
        p.start_ticks = start_ticks
        p.state.pid = p.popen.pid
        p.state.running, p.state.paused, p.state.status = True, False, "running"
        self._setup_cgroup(name, p, p.popen.pid)
        self._write_meta(p)

    def _signal_group(self, p: _Proc, sig: int) -> None:
        if not self._alive(p):
            return
        try:
            os.killpg(os.getpgid(self._leader_pid(p)), sig)
        except ProcessLookupError:
            pass

    @staticmethod
    def _has_pidfd(p: _Proc) -> bool:
        return p.popen is not None and not isinstance(p.popen, subprocess.Popen)

    async def _await_exit(self, p: _Proc, fd: int, timeout: float) -> bool:
        """Wait until the child behind pidfd ``fd`` has exited or ``timeout``
        seconds have passed; True when it is gone (and reaped). The reader
        and the timeout handle always come off the loop again."""
        loop = asyncio.get_running_loop()
        fut = loop.create_future()

        def wake(futs) -> None:
            for f in futs:
                if not f.done():
                    f.set_result(None)

        waiters = p.exit_waiters
        if not waiters:
            loop.add_reader(fd, wake, waiters)
        waiters.append(fut)
        timer = loop.call_later(timeout, wake, (fut,))
        try:
            await fut
        finally:
            timer.cancel()
            waiters.remove(fut)
            if not waiters:
                loop.remove_reader(fd)
        return not self._alive(p)

    async def _poll_exit(self, p: _Proc, timeout: float) -> None:
        """Polling reap for children without a pidfd: the Python path's
        Popen, and processes adopted after a daemon restart."""
        # most processes exit within microseconds of SIGTERM, but
        # asyncio.sleep(dt) rounds up to the epoll timer granularity
        # (~1 ms). sleep(0) yields to ready tasks WITHOUT arming a
        # timer, so this poll loop is both sub-ms for the common case
        # and cooperative under concurrency (a blocking spin here
        # measurably cut 8-tenant throughput)
        spin_until = time.monotonic() + 0.002
        while time.monotonic() < spin_until and self._alive(p):
            await asyncio.sleep(0)
        deadline = time.monotonic() + timeout
        delay = 0.001  # timer-based backoff for the slow case
        while time.monotonic() < deadline and self._alive(p):
            await asyncio.sleep(delay)
            delay = min(delay * 2, 0.02)
        if self._alive(p):
            self._signal_group(p, signal.SIGKILL)
            # reap without blocking the event loop: a process stuck in
            # D-state I/O would otherwise stall every handler for 5 s
            # 
            kill_deadline = time.monotonic() + 5
            while time.monotonic() < kill_deadline and self._alive(p):
                await asyncio.sleep(0.005)

    async def stop(self, name: str, timeout: int = 10, _removing: bool = False) -> None:
        p = self._get(name)
        p.manually_stopped = True
        self._refresh(p)
        if self._alive(p):
            self._signal_group(p, signal.SIGTERM)
            # a paused (SIGSTOPped) group keeps SIGTERM pending forever:
            # continue it so termination can be delivered (docker semantics)
            self._signal_group(p, signal.SIGCONT)
            child_fd = p.popen.fileno() if self._has_pidfd(p) else -1
            if child_fd >= 0:
                # natively spawned: the pidfd turns readable the moment the
                # leader exits, so the handler sleeps in the loop's own epoll
                # and wakes exactly then — no polling, no timer granularity
                if not await self._await_exit(p, child_fd, timeout):
                    self._signal_group(p, signal.SIGKILL)
                    await self._await_exit(p, child_fd, 5)
            else:
                await self._poll_exit(p, timeout)
        leader = self._leader_pid(p)
        if leader:
            # the leader is gone; sweep any group stragglers (orphaned
            # children). pgid == leader pid (start_new_session).
            try:
                os.killpg(leader, signal.SIGKILL)
            except (ProcessLookupError, PermissionError):
                pass
        p.state.running, p.state.paused, p.state.status = False, False, "exited"
        p.state.pid = 0
        p.attached_pid = 0
        if not _removing:  # the container dir is deleted next anyway
            self._write_meta(p)

    async def pause(self, name: str) -> None:
        p = self._get(name)
        if p.cgroup:
            try:
                with open(os.path.join(p.cgroup, "cgroup.freeze"), "w") as f:
                    f.write("1")
                p.state.paused, p.state.status = True, "paused"
                return
            except OSError:
                pass
        self._signal_group(p, signal.SIGSTOP)
        # the stop lands when the leader is next scheduled, not when kill()
        # returns: wait (bounded) until /proc shows it, so "paused" is true
        # by the time it is reported — a daemon restarted right after would
        # otherwise adopt the container as running
        leader = self._leader_pid(p)
        for _ in range(50):
            if not leader or self._proc_stat(leader)[0] in ("T", "t", None):
                break
            await asyncio.sleep(0.002)
        p.state.paused, p.state.status = True, "paused"

    async def unpause(self, name: str) -> None:
        p = self._get(name)
        if p.cgroup:
            try:
                with open(os.path.join(p.cgroup, "cgroup.freeze"), "w") as f:
                    f.write("0")
                p.state.paused, p.state.status = False, "running"
                return
            except OSError:
                pass
        self._signal_group(p, signal.SIGCONT)
        p.state.paused, p.state.status = False, "running"

    async def restart(self, name: str, timeout: int = 10) -> None:
        await self.stop(name, timeout)
        await self.start(name)

    async def remove(self, name: str, force: bool = True) -> None:
        p = self._get(name)
        self._refresh(p)
        if p.state.running:
            if not force:
                raise RuntimeError(f"{name} is running")
            await self.stop(name, timeout=2, _removing=True)
        if p.cgroup:
            try:
                os.rmdir(p.cgroup)
            except OSError:
                pass
        self._procs.pop(name, None)
        cdir = self._cdir(name)
        # Deletion is INLINE and synchronous, by measurement: an executor
        # rmtree steals the GIL from the loop in 5 ms slices (bench p50
        # 4.8 -> 6.1 ms), and two deferred designs (fire-and-forget thread,
        # supervisor-batched rm -rf) both lost their backpressure — a 60 s
        # chaos soak spiraled its last quarter to 42 ms p50 as the doomed
        # backlog outgrew the deleter. Inline is self-limiting and held
        # 252 cycles/s flat over the same soak for ~0.07 ms extra p50.
        if self._nat is not None:
            self._nat.remove_tree(cdir)  # containment-checked by _cdir
        else:
            shutil.rmtree(cdir, ignore_errors=True)

    async def inspect(self, name: str) -> Optional[ContainerState]:
        p = self._procs.get(name)
        if p is None:
            return None
        self._refresh(p)
        return p.state

    async def list(self, all: bool = True) -> List[ContainerState]:
        for p in self._procs.values():
            self._refresh(p)
        return [p.state for p in self._procs.values() if all or p.state.running]

    async def execute_rc(self, name: str, cmd: List[str], workdir: str = ""):
        p = self._get(name)
        self._refresh(p)
        if not p.state.running:
            raise RuntimeError(f"{name} is not running")
        cwd = (
            os.path.join(p.state.upper_dir, workdir.lstrip("/"))
            if workdir
            else p.state.upper_dir
        )
        os.makedirs(cwd, exist_ok=True)
        proc = await asyncio.create_subprocess_exec(
            *cmd,
            cwd=cwd,
            env=self._env_for(p),
            stdout=subprocess.PIPE,
            stderr=subprocess.STDOUT,
        )
        out, _ = await proc.communicate()
        return out.decode(errors="replace"), proc.returncode

    async def stats(self, name: str) -> Dict:
        """Process-group resource usage: cgroup v2 figures when the group
        has one (exact), else /proc of the leader process."""
        p = self._get(name)
        self._refresh(p)
        out: Dict = {"running": p.state.running, "cpuSeconds": 0.0,
                     "memoryBytes": 0, "pids": 0, "restarts": p.restarts}
        if not p.state.running or not self._leader_pid(p):
            return out
        if p.cgroup:
            try:
                with open(os.path.join(p.cgroup, "cpu.stat")) as f:
                    for line in f:
                        if line.startswith("usage_usec"):
                            out["cpuSeconds"] = round(int(line.split()[1]) / 1e6, 3)
                with open(os.path.join(p.cgroup, "memory.current")) as f:
                    out["memoryBytes"] = int(f.read())
                with open(os.path.join(p.cgroup, "cgroup.procs")) as f:
                    out["pids"] = len(f.read().split())
                return out
            except OSError:
                pass
        try:
            pid = self._leader_pid(p)
            with open(f"/proc/{pid}/stat") as f:
                fields = f.read().rsplit(") ", 1)[1].split()
                # utime (11) + stime (12) after the comm field, in ticks
                ticks = int(fields[11]) + int(fields[12])
                out["cpuSeconds"] = round(ticks / os.sysconf("SC_CLK_TCK"), 3)
            with open(f"/proc/{pid}/status") as f:
                for line in f:
                    if line.startswith("VmRSS:"):
                        out["memoryBytes"] = int(line.split()[1]) * 1024
                        break
            out["pids"] = 1
        except (OSError, IndexError, ValueError):
            pass
        return out

    async def logs(self, name: str, tail: int = 200) -> str:
        p = self._get(name)
        path = os.path.join(self._cdir(p.state.name), "console.log")
        try:
            with open(path, "rb") as f:
                f.seek(0, os.SEEK_END)
                size = f.tell()
                # cap the read at the last MiB; tail-line slicing follows
                f.seek(max(0, size - (1 << 20)))
                data = f.read()
        except OSError:
            return ""
        lines = data.decode(errors="replace").splitlines()
        return "\n".join(lines[-tail:]) + ("\n" if lines else "")

    async def image_import(self, ref: str, src_path: str) -> str:
        if not os.path.isdir(src_path):
            raise FileNotFoundError(src_path)
        dest = self._image_dir(ref)

        def _snapshot():
            shutil.rmtree(dest, ignore_errors=True)
            shutil.copytree(src_path, dest, symlinks=True)

        await asyncio.get_running_loop().run_in_executor(None, _snapshot)
        return ref

    async def image_list(self) -> List[Dict]:
        iroot = os.path.join(self.base, "images")
        out = []
        for entry in sorted(os.listdir(iroot)):
            path = os.path.join(iroot, entry)
            if os.path.isdir(path):
                out.append({"ref": entry, "path": path})
        return out

    async def commit(self, name: str, image: str, tag: str = "") -> str:
        p = self._get(name)
        ref = f"{image}:{tag}" if tag else image
        dest = self._image_dir(ref)
        src = p.state.upper_dir

        def _snapshot():
            shutil.rmtree(dest, ignore_errors=True)
            shutil.copytree(src, dest, symlinks=True)

        await asyncio.get_running_loop().run_in_executor(None, _snapshot)
        return ref

    # --------------------------------------------------------------- volumes
    #
    # Sized volumes are backed by a sparse image file + loop mount (ext4):
    # writes beyond the size fail with ENOSPC — real quota enforcement, the
    # analog of the docker driver's overlay2-on-xfs project quotas
    # (reference requires that host setup, docs/volume-size-scale-en.md).
    # Falls back to a plain directory where mounting isn't permitted
    # (unprivileged dev boxes); the recorded size is then advisory.

    async def _try_loop_volume(self, vdir: str, mp: str, size_str: str) -> bool:
        from ..models.memory import to_bytes

        if not self.loop_volumes or not os.path.exists("/dev/loop-control"):
            return False
        try:
            size = to_bytes(size_str)
        except Exception:
            return False
        img = os.path.join(vdir, "volume.img")
        try:
            with open(img, "wb") as f:
                f.truncate(size)
            proc = await asyncio.create_subprocess_exec(
                "mkfs.ext4", "-q", "-F", img,
                stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
            )
            if await proc.wait() != 0:
                raise OSError("mkfs failed")
            proc = await asyncio.create_subprocess_exec(
                "mount", "-o", "loop", img, mp,
                stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
            )
            if await proc.wait() != 0:
                raise OSError("mount failed")
            return True
        except OSError:
            try:
                os.unlink(img)
            except OSError:
                pass
            return False

    async def volume_create(
        self, name: str, driver_opts: Optional[Dict[str, str]] = None
    ) -> VolumeState:
        if name in self.volumes:
            raise VolumeExisted(name)
        vdir = self._vdir(name)
        mp = os.path.join(vdir, "_data")
        os.makedirs(mp, exist_ok=True)
        opts = dict(driver_opts or {})
        if opts.get("size"):
            opts["enforced"] = "loop" if await self._try_loop_volume(vdir, mp, opts["size"]) else "none"
        with open(os.path.join(vdir, "opts.json"), "w") as f:
            json.dump(opts, f)
        vs = VolumeState(name=name, mountpoint=mp, options=opts)
        self.volumes[name] = vs
        return vs

    async def volume_remove(self, name: str, force: bool = True) -> None:
        vs = self.volumes.pop(name, None)
        vdir = self._vdir(name)
        if vs is not None and vs.options.get("enforced") == "loop":
            proc = await asyncio.create_subprocess_exec(
                "umount", "-l", vs.mountpoint,
                stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
            )
            await proc.wait()
            if os.path.ismount(vs.mountpoint):
                # never rmtree through a still-attached mount: that deletes
                # the volume's live data instead of the backing dir
                self.volumes[name] = vs
                raise RuntimeError(f"volume {name}: unmount failed, not removing")
        shutil.rmtree(vdir, ignore_errors=True)

    async def volume_inspect(self, name: str) -> Optional[VolumeState]:
        return self.volumes.get(name)

    async def close(self) -> None:
        if self._supervisor is not None:
            self._supervisor.cancel()
            self._supervisor = None
        for name in list(self._procs):
            p = self._procs[name]
            if p.popen is not None and p.popen.poll() is None:
                await self.stop(name, timeout=2)
