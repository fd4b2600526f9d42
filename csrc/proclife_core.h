// Container process lifecycle on raw syscalls: spawn, reap, directory
// teardown and the two small files the proc runtime writes per container.
//
// This is the host work of one replicaSet cycle (runtime/proc.py). Python's
// subprocess.Popen re-encodes ~100 environment variables, builds an error
// pipe and walks its own fd bookkeeping for every spawn; shutil.rmtree
// walks a 3-file directory through os.scandir objects. The same kernel work
// is a vfork+execve, a pidfd and a handful of unlinkat calls.
//
// No pybind11 in here: csrc/proclife.cpp binds it, csrc/proclife_selftest.cpp
// drives it stand-alone under the host sanitizers. Errors are reported as
// errno values, never thrown.
#pragma once

#ifndef _GNU_SOURCE
#define _GNU_SOURCE
#endif

#include <cerrno>
#include <cstdio>
#include <csignal>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include <dirent.h>
#include <fcntl.h>
#include <poll.h>
#include <sys/stat.h>
#include <sys/syscall.h>
#include <sys/types.h>
#include <sys/wait.h>
#include <unistd.h>

namespace proclife {

using KV = std::pair<std::string, std::string>;

// ---------------------------------------------------------------------------
// Environment: the base is encoded once; a spawn merges a few overrides
// ---------------------------------------------------------------------------

class BaseEnv {
 public:
  // Same result as dict(kv): a repeated key keeps its first position and
  // takes the last value.
  void set(const std::vector<KV>& kv) {
    entries_.clear();
    index_.clear();
    entries_.reserve(kv.size());
    for (const auto& e : kv) {
      auto it = index_.find(e.first);
      if (it == index_.end()) {
        index_.emplace(e.first, entries_.size());
        entries_.push_back(e.first + "=" + e.second);
      } else {
        entries_[it->second] = e.first + "=" + e.second;
      }
    }
  }
  size_t size() const { return entries_.size(); }
  const std::vector<std::string>& entries() const { return entries_; }
  long find(const std::string& key) const {
    auto it = index_.find(key);
    return it == index_.end() ? -1 : static_cast<long>(it->second);
  }

 private:
  std::vector<std::string> entries_;  // "KEY=VALUE", dict order
  std::unordered_map<std::string, size_t> index_;
};

// base + overrides with dict.update semantics: an override replaces a base
// key in place, a new key is appended, the last duplicate wins.
class MergedEnv {
 public:
  MergedEnv(const BaseEnv& base, const std::vector<KV>& overrides) {
    const auto& be = base.entries();
    slots_.reserve(be.size() + overrides.size() + 1);
    for (const auto& s : be) slots_.push_back(s.c_str());
    owned_.reserve(overrides.size());  // no reallocation: c_str() stays valid
    std::vector<std::pair<const std::string*, size_t>> added;  // new key -> slot
    for (const auto& o : overrides) {
      owned_.push_back(o.first + "=" + o.second);
      const char* entry = owned_.back().c_str();
      long at = base.find(o.first);
      if (at < 0) {
        for (const auto& a : added)
          if (*a.first == o.first) at = static_cast<long>(a.second);
      }
      if (at >= 0) {
        slots_[static_cast<size_t>(at)] = entry;
      } else {
        added.emplace_back(&o.first, slots_.size());
        slots_.push_back(entry);
      }
    }
    slots_.push_back(nullptr);
  }
  char* const* envp() const { return const_cast<char* const*>(slots_.data()); }
  // value of KEY in the merged environment, or nullptr
  const char* get(const char* key) const {
    size_t n = std::strlen(key);
    for (const char* e : slots_)
      if (e && std::strncmp(e, key, n) == 0 && e[n] == '=') return e + n + 1;
    return nullptr;
  }

 private:
  std::vector<std::string> owned_;
  std::vector<const char*> slots_;
};

// ---------------------------------------------------------------------------
// /proc/<pid>/stat
// ---------------------------------------------------------------------------

// Field 22 (starttime, clock ticks since boot), parsed after the LAST ") "
// because comm may itself contain ") ". 0 when the pid is gone, a zombie
// (Z/X) or the line does not parse — what ProcRuntime._proc_stat reports as
// "no identity".
inline unsigned long long read_starttime(pid_t pid, char* state_out = nullptr) {
  char path[48];
  std::snprintf(path, sizeof path, "/proc/%d/stat", static_cast<int>(pid));
  int fd = ::open(path, O_RDONLY | O_CLOEXEC);
  if (fd < 0) return 0;
  char buf[2048];
  size_t len = 0;
  for (;;) {
    ssize_t n = ::read(fd, buf + len, sizeof buf - 1 - len);
    if (n < 0 && errno == EINTR) continue;
    if (n <= 0) break;
    len += static_cast<size_t>(n);
    if (len == sizeof buf - 1) break;
  }
  ::close(fd);
  buf[len] = '\0';
  const char* after = nullptr;
  for (size_t i = 0; i + 1 < len; ++i)
    if (buf[i] == ')' && buf[i + 1] == ' ') after = buf + i + 2;
  if (!after) return 0;
  // after: "S ppid pgrp ..." — state is field 0, starttime field 19
  char state = *after;
  if (state_out) *state_out = state;
  if (state == 'Z' || state == 'X' || state == '\0') return 0;
  const char* p = after;
  for (int field = 0; field < 19; ++field) {
    while (*p && *p != ' ' && *p != '\n') ++p;
    while (*p == ' ') ++p;
    if (!*p) return 0;
  }
  char* end = nullptr;
  errno = 0;
  unsigned long long v = std::strtoull(p, &end, 10);
  if (end == p || errno) return 0;
  return v;
}

// ---------------------------------------------------------------------------
// Child: pid + pidfd + start-time identity
// ---------------------------------------------------------------------------

#ifndef P_PIDFD
#define P_PIDFD 3
#endif

namespace detail {
// Children dropped while still running: reaped opportunistically at the
// next spawn so they never stay zombies (subprocess keeps the same list).
inline std::mutex& orphan_mu() {
  static std::mutex m;
  return m;
}
inline std::vector<pid_t>& orphans() {
  static std::vector<pid_t> v;
  return v;
}
inline void reap_orphans() {
  std::lock_guard<std::mutex> g(orphan_mu());
  auto& v = orphans();
  for (size_t i = 0; i < v.size();) {
    int st;
    pid_t r = ::waitpid(v[i], &st, WNOHANG);
    if (r == v[i] || (r < 0 && errno == ECHILD)) {
      v[i] = v.back();
      v.pop_back();
    } else {
      ++i;
    }
  }
}
}  // namespace detail

struct Child {
  pid_t pid = -1;
  int pidfd = -1;
  unsigned long long starttime = 0;
  bool exited = false;
  int returncode = 0;

  Child() = default;
  Child(const Child&) = delete;
  Child& operator=(const Child&) = delete;
  Child(Child&& o) noexcept { *this = std::move(o); }
  Child& operator=(Child&& o) noexcept {
    if (this != &o) {
      release();
      pid = o.pid, pidfd = o.pidfd, starttime = o.starttime;
      exited = o.exited, returncode = o.returncode;
      o.pid = -1, o.pidfd = -1, o.exited = true;
    }
    return *this;
  }
  ~Child() { release(); }

  // Non-blocking reap. true once the child has exited; returncode is then
  // the exit status, or -signal (subprocess convention). Idempotent.
  bool poll() {
    if (exited || pid <= 0) return exited;
    siginfo_t info;
    for (;;) {
      std::memset(&info, 0, sizeof info);
      int r = pidfd >= 0
                  ? ::waitid(static_cast<idtype_t>(P_PIDFD), static_cast<id_t>(pidfd), &info,
                             WEXITED | WNOHANG)
                  : ::waitid(P_PID, static_cast<id_t>(pid), &info, WEXITED | WNOHANG);
      if (r == 0) break;
      if (errno == EINTR) continue;
      // ECHILD: reaped elsewhere (SIGCHLD ignored, foreign waitpid); the
      // status is lost — report 0 as subprocess does
      exited = true;
      returncode = 0;
      return true;
    }
    if (info.si_pid == 0) return false;  // still running
    exited = true;
    returncode = info.si_code == CLD_EXITED ? info.si_status : -info.si_status;
    return true;
  }

  // Block until exit or timeout_ms (<0: forever). true once exited.
  bool wait(int timeout_ms) {
    if (poll()) return true;
    if (pidfd >= 0) {
      struct pollfd pfd = {pidfd, POLLIN, 0};
      for (;;) {
        int r = ::poll(&pfd, 1, timeout_ms);
        if (r < 0 && errno == EINTR) continue;
        break;
      }
      return poll();
    }
    // no pidfd (pre-5.3 kernel): coarse polling
    for (int waited = 0; timeout_ms < 0 || waited < timeout_ms; ++waited) {
      if (poll()) return true;
      ::usleep(1000);
    }
    return poll();
  }

  void close_fd() {
    if (pidfd >= 0) {
      ::close(pidfd);
      pidfd = -1;
    }
  }

  // Destructor body: never blocks, never leaves a zombie behind for good.
  void release() {
    if (pid > 0 && !exited && !poll()) {
      std::lock_guard<std::mutex> g(detail::orphan_mu());
      detail::orphans().push_back(pid);
    }
    close_fd();
    pid = -1;
  }
};

// ---------------------------------------------------------------------------
// spawn
// ---------------------------------------------------------------------------

struct SpawnError {
  int err = 0;           // errno; 0 on success
  std::string filename;  // what the errno is about (argv[0], cwd or log)
};

namespace detail {

#ifndef SYS_close_range
#define SYS_close_range 436
#endif

// Everything the child needs, laid out before vfork: between vfork and
// execve the child runs in the daemon's own address space and may only make
// async-signal-safe calls — no allocation, no locks, no C++ runtime.
struct ChildPlan {
  int logfd;
  const char* cwd;
  char* const* argv;
  char* const* envp;
  const char* const* candidates;  // executable paths to try, null-terminated
  const sigset_t* sigmask;        // the caller's mask, restored before exec
  int max_fd;                     // bound of the close loop without close_range
  volatile int* err;              // errno of the step that failed
  volatile int* stage;            // 1: chdir, 2: exec, 3: anything else
};

[[noreturn]] __attribute__((noinline)) inline void child_exec(const ChildPlan& p) {
  // No handler may ever run in here (it would run on the daemon's memory):
  // the caller has every signal blocked; put all handled signals back to
  // their default before the mask is restored. SIGPIPE and SIGXFSZ, which
  // Python ignores, get their defaults back too — an ignored disposition
  // survives exec (Popen's restore_signals).
  struct sigaction dfl;
  std::memset(&dfl, 0, sizeof dfl);
  dfl.sa_handler = SIG_DFL;
  for (int sig = 1; sig < NSIG; ++sig) {
    struct sigaction cur;
    if (::sigaction(sig, nullptr, &cur) != 0 || cur.sa_handler == SIG_DFL) continue;
    if (cur.sa_handler == SIG_IGN && sig != SIGPIPE && sig != SIGXFSZ) continue;
    ::sigaction(sig, &dfl, nullptr);
  }
  int stage = 3;
  do {
    if (::setsid() < 0) break;  // own session and process group
    if (::dup2(p.logfd, 1) < 0 || ::dup2(p.logfd, 2) < 0) break;
    stage = 1;
    if (::chdir(p.cwd) != 0) break;
    stage = 3;
    if (::sigprocmask(SIG_SETMASK, p.sigmask, nullptr) != 0) break;
    // stdin, stdout, stderr and nothing else (Popen's close_fds=True)
    if (::syscall(SYS_close_range, 3U, ~0U, 0U) != 0)
      for (int fd = 3; fd < p.max_fd; ++fd) ::close(fd);
    // _posixsubprocess order: try every candidate; the first errno that is
    // not ENOENT/ENOTDIR wins, else the last one
    stage = 2;
    int saved = 0;
    for (const char* const* c = p.candidates; *c; ++c) {
      ::execve(*c, p.argv, p.envp);
      if (errno != ENOENT && errno != ENOTDIR && saved == 0) saved = errno;
    }
    if (saved) errno = saved;
  } while (false);
  *p.err = errno ? errno : EINVAL;  // the parent reads this: memory is shared
  *p.stage = stage;
  ::_exit(127);
}

// The vfork itself, in a frame of its own: no local of spawn() is live
// across the point that returns twice.
__attribute__((noinline)) inline pid_t vfork_child(const ChildPlan& plan, int* vfork_errno) {
  pid_t pid = ::vfork();
  if (pid == 0) child_exec(plan);  // never returns
  *vfork_errno = errno;
  return pid;
}

}  // namespace detail

// Start argv as a fresh process in its own session and process group, with
// cwd as working directory, stdout+stderr appended to log_path, stdin
// inherited, every other descriptor closed, and exactly base+overrides as
// environment. argv[0] is resolved as subprocess.Popen resolves it: a name
// without a slash is searched in the CHILD environment's PATH, a name with
// one is taken relative to the child's cwd.
//
// The child is made with vfork: it borrows the caller's address space until
// it execs, so nothing is copied however large the daemon is, the caller
// resumes only once the exec has succeeded or failed, and a failure's errno
// comes back through plain memory (no error pipe); the failed child is
// reaped before returning. posix_spawn does the same with a freshly mapped
// child stack, and mapping and unmapping that per spawn in a many-threaded
// process cost more than the spawn. The daemon itself never execs.
inline SpawnError spawn(const std::vector<std::string>& argv, const std::string& cwd,
                        const BaseEnv& base, const std::vector<KV>& overrides,
                        const std::string& log_path, Child* out) {
  SpawnError res;
  if (argv.empty()) {
    res.err = EINVAL;
    return res;
  }
  detail::reap_orphans();
  MergedEnv env(base, overrides);

  std::vector<char*> cargv;
  cargv.reserve(argv.size() + 1);
  for (const auto& a : argv) cargv.push_back(const_cast<char*>(a.c_str()));
  cargv.push_back(nullptr);

  // executable candidates; one that does not exist costs a stat here, not
  // an execve in the child
  std::vector<std::string> cands;
  int skipped_err = ENOENT;
  const std::string& name = argv[0];
  if (name.find('/') != std::string::npos) {
    cands.push_back(name);
  } else {
    const char* path = env.get("PATH");
    std::string dirs = path ? path : "/bin:/usr/bin";
    for (size_t pos = 0;;) {
      size_t colon = dirs.find(':', pos);
      std::string dir = dirs.substr(pos, colon == std::string::npos ? colon : colon - pos);
      std::string cand = dir.empty() ? name : dir + "/" + name;
      std::string probe = cand[0] == '/' ? cand : cwd + "/" + cand;
      struct stat st;
      if (::stat(probe.c_str(), &st) != 0 && (errno == ENOENT || errno == ENOTDIR))
        skipped_err = errno;
      else
        cands.push_back(std::move(cand));
      if (colon == std::string::npos) break;
      pos = colon + 1;
    }
  }
  std::vector<const char*> cptrs;
  cptrs.reserve(cands.size() + 1);
  for (const auto& c : cands) cptrs.push_back(c.c_str());
  cptrs.push_back(nullptr);

  int logfd = ::open(log_path.c_str(), O_WRONLY | O_CREAT | O_APPEND | O_CLOEXEC, 0666);
  if (logfd < 0) {
    res.err = errno, res.filename = log_path;
    return res;
  }
  if (logfd < 3) {  // daemon started with a std stream closed: move out of the way
    int moved = ::fcntl(logfd, F_DUPFD_CLOEXEC, 3);
    int e = errno;
    ::close(logfd);
    if (moved < 0) {
      res.err = e, res.filename = log_path;
      return res;
    }
    logfd = moved;
  }

  volatile int child_err = 0, child_stage = 0;
  pid_t pid = -1;
  int err = 0;
  if (cands.empty()) {
    // nothing on PATH by that name — but Popen reports a missing cwd first
    struct stat st;
    if (::stat(cwd.c_str(), &st) != 0) {
      err = errno, child_stage = 1;
    } else {
      err = skipped_err, child_stage = 2;
    }
  } else {
    long open_max = ::sysconf(_SC_OPEN_MAX);
    sigset_t all, old;
    sigfillset(&all);
    pthread_sigmask(SIG_SETMASK, &all, &old);
    detail::ChildPlan plan = {logfd,        cwd.c_str(), cargv.data(),
                              env.envp(),   cptrs.data(), &old,
                              open_max > 0 && open_max < 65536 ? static_cast<int>(open_max) : 65536,
                              &child_err,   &child_stage};
    int vfork_err = 0;
    pid = detail::vfork_child(plan, &vfork_err);
    pthread_sigmask(SIG_SETMASK, &old, nullptr);
    if (pid < 0) {
      err = vfork_err, child_stage = 3;
    } else if (child_err != 0) {
      err = child_err;
      int st;
      while (::waitpid(pid, &st, 0) < 0 && errno == EINTR) {
      }
    }
  }
  ::close(logfd);

  if (err != 0) {
    res.err = err;
    // as Popen: name the cwd when the chdir is what failed
    res.filename = child_stage == 1 ? cwd : child_stage == 2 ? argv[0] : std::string();
    return res;
  }
  Child c;
  c.pid = pid;
  c.pidfd = static_cast<int>(::syscall(SYS_pidfd_open, pid, 0));  // CLOEXEC by definition
  c.starttime = read_starttime(pid);
  *out = std::move(c);
  return res;
}

// ---------------------------------------------------------------------------
// remove_tree: shutil.rmtree(path, ignore_errors=True)
// ---------------------------------------------------------------------------

namespace detail {

constexpr int kDirFlags = O_RDONLY | O_DIRECTORY | O_NOFOLLOW | O_CLOEXEC;

// Empties the directory behind dfd (takes ownership of dfd). Everything is
// relative to a descriptor, so path length never matters and a symlink is
// unlinked, never entered.
inline long empty_dir(int dfd) {
  DIR* d = ::fdopendir(dfd);
  if (!d) {
    ::close(dfd);
    return 1;
  }
  // list first, then remove: no reliance on readdir-after-unlink behaviour
  std::vector<std::pair<std::string, unsigned char>> names;
  for (;;) {
    errno = 0;
    struct dirent* e = ::readdir(d);
    if (!e) break;
    const char* n = e->d_name;
    if (n[0] == '.' && (n[1] == '\0' || (n[1] == '.' && n[2] == '\0'))) continue;
    names.emplace_back(n, e->d_type);
  }
  long failed = errno ? 1 : 0;
  for (auto& ent : names) {
    const char* n = ent.first.c_str();
    bool is_dir = ent.second == DT_DIR;
    if (ent.second == DT_UNKNOWN) {
      struct stat st;
      is_dir = ::fstatat(dfd, n, &st, AT_SYMLINK_NOFOLLOW) == 0 && S_ISDIR(st.st_mode);
    }
    if (is_dir) {
      int sub = ::openat(dfd, n, kDirFlags);
      if (sub < 0) {
        ++failed;
        continue;
      }
      failed += empty_dir(sub);
      if (::unlinkat(dfd, n, AT_REMOVEDIR) != 0) ++failed;
    } else if (::unlinkat(dfd, n, 0) != 0) {
      ++failed;
    }
  }
  ::closedir(d);  // closes dfd
  return failed;
}

}  // namespace detail

// Number of entries that could not be removed (0: the tree is gone, or was
// never there). A path that is a symlink, or no directory, is left alone
// and counts as one failure, as rmtree refuses it.
inline long remove_tree(const char* path) {
  int dfd = ::open(path, detail::kDirFlags);
  if (dfd < 0) return errno == ENOENT ? 0 : 1;
  long failed = detail::empty_dir(dfd);
  if (::rmdir(path) != 0) ++failed;
  return failed;
}

// ---------------------------------------------------------------------------
// small files
// ---------------------------------------------------------------------------

// open(path, "w") + write + close. Returns errno.
inline int write_file(const char* path, const char* data, size_t len) {
  int fd = ::open(path, O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0666);
  if (fd < 0) return errno;
  while (len > 0) {
    ssize_t n = ::write(fd, data, len);
    if (n < 0) {
      if (errno == EINTR) continue;
      int e = errno;
      ::close(fd);
      return e;
    }
    data += n, len -= static_cast<size_t>(n);
  }
  return ::close(fd) != 0 ? errno : 0;
}

// os.makedirs(path, exist_ok=True). Returns errno.
inline int make_dirs(const std::string& path) {
  if (::mkdir(path.c_str(), 0777) == 0) return 0;
  if (errno == EEXIST) {
    struct stat st;
    return (::stat(path.c_str(), &st) == 0 && S_ISDIR(st.st_mode)) ? 0 : EEXIST;
  }
  if (errno != ENOENT) return errno;
  size_t end = path.find_last_not_of('/');
  size_t slash = end == std::string::npos ? end : path.rfind('/', end);
  if (slash == std::string::npos || slash == 0) return ENOENT;
  if (int e = make_dirs(path.substr(0, slash))) return e;
  if (::mkdir(path.c_str(), 0777) == 0 || errno == EEXIST) return 0;
  return errno;
}

// mkdir -p cdir/rootfs, then write cdir/spec.json. Returns errno; *failed
// names the path the errno is about.
inline int prepare_container_dir(const std::string& cdir, const char* spec, size_t len,
                                 std::string* failed) {
  std::string rootfs = cdir + "/rootfs";
  if (int e = make_dirs(rootfs)) {
    *failed = rootfs;
    return e;
  }
  std::string specf = cdir + "/spec.json";
  if (int e = write_file(specf.c_str(), spec, len)) {
    *failed = specf;
    return e;
  }
  return 0;
}

}  // namespace proclife
