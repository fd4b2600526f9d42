// Stand-alone self-test of csrc/proclife_core.h, meant to be built with the
// host sanitizers and run on a CPU:
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-omit-frame-pointer
//       csrc/proclife_selftest.cpp -o /tmp/proclife_selftest && /tmp/proclife_selftest
//
// It drives a few hundred spawn / kill / reap / remove_tree rounds plus the
// failure paths and then checks that the process holds the same number of
// descriptors and no child it did not have before. Exit status 0 = clean.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>

#include "proclife_core.h"

namespace pl = proclife;

static int g_failed = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                          \
    }                                                                      \
  } while (0)

static int count_fds() {
  DIR* d = ::opendir("/proc/self/fd");
  if (!d) return -1;
  int n = 0;
  while (struct dirent* e = ::readdir(d))
    if (e->d_name[0] != '.') ++n;
  ::closedir(d);
  return n - 1;  // the listing's own descriptor
}

static bool have_children() {
  siginfo_t info;
  std::memset(&info, 0, sizeof info);
  return ::waitid(P_ALL, 0, &info, WEXITED | WNOHANG | WNOWAIT) == 0;  // ECHILD: none
}

static std::string slurp(const std::string& path) {
  std::ifstream f(path);
  std::stringstream ss;
  ss << f.rdbuf();
  return ss.str();
}

static void build_tree(const std::string& root) {
  CHECK(pl::make_dirs(root + "/a/b/c") == 0);
  CHECK(pl::write_file((root + "/a/f1").c_str(), "x", 1) == 0);
  CHECK(pl::write_file((root + "/a/b/f2").c_str(), "yy", 2) == 0);
  CHECK(::link((root + "/a/f1").c_str(), (root + "/a/b/c/hard").c_str()) == 0);
  CHECK(::symlink("/nonexistent/target", (root + "/a/dangling").c_str()) == 0);
  CHECK(pl::write_file((root + "/locked").c_str(), "z", 1) == 0);
  CHECK(::chmod((root + "/locked").c_str(), 0) == 0);
}

int main() {
  char tmpl[] = "/tmp/proclife-selftest-XXXXXX";
  const char* made = ::mkdtemp(tmpl);
  if (!made) {
    std::perror("mkdtemp");
    return 2;
  }
  const std::string top = made;

  pl::BaseEnv base;
  base.set({{"PATH", "/usr/local/bin:/usr/bin:/bin"}, {"KEEP", "1"}, {"OVER", "base"}});

  // warm up once so lazily created descriptors (none expected) are counted
  { pl::Child warm; }
  const int fds_before = count_fds();
  CHECK(!have_children());

  // --- env merge ----------------------------------------------------------
  {
    pl::MergedEnv env(base, {{"OVER", "a=b"}, {"NEW", ""}, {"NEW", "last"}, {"OVER", "final"}});
    CHECK(std::string(env.get("OVER")) == "final");
    CHECK(std::string(env.get("NEW")) == "last");
    CHECK(std::string(env.get("KEEP")) == "1");
    CHECK(env.get("ABSENT") == nullptr);
    int n = 0;
    for (char* const* e = env.envp(); *e; ++e) ++n;
    CHECK(n == 4);
  }

  // --- spawn / signal / reap ---------------------------------------------
  for (int round = 0; round < 200; ++round) {
    const std::string cdir = top + "/c" + std::to_string(round);
    std::string failed;
    CHECK(pl::prepare_container_dir(cdir, "{}", 2, &failed) == 0);
    pl::Child c;
    pl::SpawnError e = pl::spawn({"sleep", "30"}, cdir + "/rootfs", base,
                                 {{"ROUND", std::to_string(round)}}, cdir + "/console.log", &c);
    CHECK(e.err == 0);
    if (e.err) break;
    CHECK(c.pid > 0 && c.pidfd >= 0 && c.starttime > 0);
    CHECK(::getsid(c.pid) == c.pid && ::getpgid(c.pid) == c.pid);
    CHECK(!c.poll());
    CHECK(pl::read_starttime(c.pid) == c.starttime);
    if (round % 3 == 0) {
      // leave it to the destructor + orphan list (reaped at a later spawn)
      CHECK(::kill(-c.pid, SIGKILL) == 0);
    } else {
      CHECK(::kill(-c.pid, round % 2 ? SIGTERM : SIGKILL) == 0);
      CHECK(c.wait(5000));
      CHECK(c.returncode == (round % 2 ? -SIGTERM : -SIGKILL));
      CHECK(c.poll() && c.poll());  // idempotent
      c.close_fd();
      c.close_fd();
    }
    CHECK(pl::remove_tree(cdir.c_str()) == 0);
    struct stat st;
    CHECK(::lstat(cdir.c_str(), &st) != 0 && errno == ENOENT);
  }

  // exit status and output redirection
  {
    const std::string cdir = top + "/out";
    std::string failed;
    CHECK(pl::prepare_container_dir(cdir, "{}", 2, &failed) == 0);
    for (int i = 0; i < 2; ++i) {
      pl::Child c;
      pl::SpawnError e = pl::spawn({"sh", "-c", "echo out; echo err >&2; exit 7"}, cdir + "/rootfs",
                                   base, {}, cdir + "/console.log", &c);
      CHECK(e.err == 0);
      CHECK(c.wait(5000) && c.returncode == 7);
    }
    CHECK(slurp(cdir + "/console.log") == "out\nerr\nout\nerr\n");  // appended, not truncated
    CHECK(pl::remove_tree(cdir.c_str()) == 0);
  }

  // --- failure paths -------------------------------------------------------
  {
    const std::string cdir = top + "/bad";
    std::string failed;
    CHECK(pl::prepare_container_dir(cdir, "{}", 2, &failed) == 0);
    CHECK(pl::write_file((cdir + "/rootfs/noexec").c_str(), "#!/bin/sh\n", 10) == 0);
    CHECK(::chmod((cdir + "/rootfs/noexec").c_str(), 0644) == 0);
    for (int round = 0; round < 200; ++round) {
      pl::Child c;
      pl::SpawnError e;
      switch (round % 5) {
        case 0:
          e = pl::spawn({"definitely-not-a-command"}, cdir + "/rootfs", base, {},
                        cdir + "/console.log", &c);
          CHECK(e.err == ENOENT);
          break;
        case 1:
          e = pl::spawn({"./noexec"}, cdir + "/rootfs", base, {}, cdir + "/console.log", &c);
          CHECK(e.err == EACCES);
          break;
        case 2:
          e = pl::spawn({"/no/such/binary"}, cdir + "/rootfs", base, {}, cdir + "/console.log", &c);
          CHECK(e.err == ENOENT);
          break;
        case 3:
          e = pl::spawn({"sleep", "1"}, cdir + "/missing-cwd", base, {}, cdir + "/console.log", &c);
          CHECK(e.err == ENOENT && e.filename == cdir + "/missing-cwd");
          break;
        default:
          e = pl::spawn({"sleep", "1"}, cdir + "/rootfs", base, {}, cdir + "/no-dir/console.log",
                        &c);
          CHECK(e.err == ENOENT);
          break;
      }
      CHECK(c.pid == -1 && c.pidfd == -1);
    }
    CHECK(pl::remove_tree(cdir.c_str()) == 0);
  }

  // --- remove_tree ---------------------------------------------------------
  for (int round = 0; round < 50; ++round) {
    const std::string root = top + "/tree";
    build_tree(root);
    CHECK(pl::remove_tree(root.c_str()) == 0);
    struct stat st;
    CHECK(::lstat(root.c_str(), &st) != 0);
  }
  {
    // a symlink inside goes, its target stays; a symlinked root is refused
    const std::string outside = top + "/outside", root = top + "/tree2";
    CHECK(pl::make_dirs(outside) == 0 && pl::make_dirs(root) == 0);
    CHECK(pl::write_file((outside + "/keep").c_str(), "k", 1) == 0);
    CHECK(::symlink(outside.c_str(), (root + "/link").c_str()) == 0);
    CHECK(pl::remove_tree(root.c_str()) == 0);
    CHECK(slurp(outside + "/keep") == "k");
    CHECK(::symlink(outside.c_str(), (top + "/rootlink").c_str()) == 0);
    CHECK(pl::remove_tree((top + "/rootlink").c_str()) == 1);
    CHECK(slurp(outside + "/keep") == "k");
    CHECK(::unlink((top + "/rootlink").c_str()) == 0);
    CHECK(pl::remove_tree((top + "/never-existed").c_str()) == 0);
    CHECK(pl::remove_tree(outside.c_str()) == 0);
  }
  {
    // deeper than PATH_MAX: 60 levels of 100-character names
    const std::string root = top + "/deep", seg(100, 'd');
    CHECK(pl::make_dirs(root) == 0);
    int fd = ::open(root.c_str(), O_RDONLY | O_DIRECTORY | O_CLOEXEC);
    CHECK(fd >= 0);
    for (int level = 0; level < 60 && fd >= 0; ++level) {
      CHECK(::mkdirat(fd, seg.c_str(), 0777) == 0);
      int file = ::openat(fd, "f", O_WRONLY | O_CREAT | O_CLOEXEC, 0666);
      CHECK(file >= 0);
      if (file >= 0) ::close(file);
      int next = ::openat(fd, seg.c_str(), O_RDONLY | O_DIRECTORY | O_CLOEXEC);
      ::close(fd);
      fd = next;
    }
    if (fd >= 0) ::close(fd);
    CHECK(pl::remove_tree(root.c_str()) == 0);
    struct stat st;
    CHECK(::lstat(root.c_str(), &st) != 0);
  }

  // --- nothing left behind -------------------------------------------------
  pl::detail::reap_orphans();
  for (int i = 0; i < 200 && have_children(); ++i) {  // SIGKILLed orphans still dying
    ::usleep(5000);
    pl::detail::reap_orphans();
  }
  CHECK(!have_children());
  CHECK(pl::detail::orphans().empty());
  CHECK(count_fds() == fds_before);
  CHECK(pl::remove_tree(top.c_str()) == 0);

  if (g_failed) {
    std::fprintf(stderr, "proclife selftest: %d check(s) FAILED\n", g_failed);
    return 1;
  }
  std::printf("proclife selftest OK\n");
  return 0;
}
