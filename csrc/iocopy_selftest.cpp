// Stand-alone self-test of csrc/iocopy_core.h, meant to be built with the
// host sanitizers and run on a CPU:
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-omit-frame-pointer
//       csrc/iocopy_selftest.cpp -o /tmp/iocopy_selftest && /tmp/iocopy_selftest
//
// It copies a small tree through the three data paths (ring, copy_file_range
// loop, pread/pwrite) and compares sizes, content and link counts; drives the
// failing-destination case and checks that the process holds the same number
// of descriptors afterwards; and forces a short write under RLIMIT_FSIZE in a
// forked child, where every path has to throw. LeakSanitizer covers DIR
// handles and slot buffers at exit. Exit status 0 = clean.
#include <cstdio>
#include <cstdlib>
#include <csignal>
#include <fstream>
#include <sstream>

#include <sys/resource.h>
#include <sys/wait.h>

#include "iocopy_core.h"

static int g_failed = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                          \
    }                                                                      \
  } while (0)

static const iocopy::Options kPaths[3] = {{true, true}, {false, true}, {false, false}};

static int count_fds() {
  DIR* d = ::opendir("/proc/self/fd");
  if (!d) return -1;
  int n = 0;
  while (struct dirent* e = ::readdir(d))
    if (e->d_name[0] != '.') ++n;
  ::closedir(d);
  return n - 1;  // the listing's own descriptor
}

static std::string slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  std::stringstream ss;
  ss << f.rdbuf();
  return ss.str();
}

// content derived from the name, so a swapped buffer shows
static std::string content(const std::string& name, size_t len) {
  std::string out(len, '\0');
  unsigned x = 2166136261u;
  for (char c : name) x = (x ^ (unsigned char)c) * 16777619u;
  for (size_t i = 0; i < len; ++i) {
    x = x * 1664525u + 1013904223u;
    out[i] = (char)(x >> 24);
  }
  return out;
}

static void put(const std::string& path, const std::string& name, size_t len) {
  std::ofstream f(path, std::ios::binary);
  const std::string c = content(name, len);
  f.write(c.data(), (std::streamsize)c.size());
  f.close();
  CHECK(f.good());
}

static void rm_rf(const std::string& path) {
  struct stat st;
  if (::lstat(path.c_str(), &st) != 0) return;
  if (S_ISDIR(st.st_mode)) {
    ::chmod(path.c_str(), 0700);
    if (DIR* d = ::opendir(path.c_str())) {
      while (struct dirent* e = ::readdir(d)) {
        std::string n(e->d_name);
        if (n != "." && n != "..") rm_rf(path + "/" + n);
      }
      ::closedir(d);
    }
    ::rmdir(path.c_str());
  } else {
    ::unlink(path.c_str());
  }
}

static const size_t kSizes[] = {0, 1, 4095, 4096, 262143, 262144, 262145, (1u << 20) + 1};

static void build_tree(const std::string& root) {
  CHECK(::mkdir(root.c_str(), 0755) == 0);
  CHECK(::mkdir((root + "/sub").c_str(), 0555 | 0200) == 0);
  for (size_t len : kSizes) put(root + "/f" + std::to_string(len), "f" + std::to_string(len), len);
  for (int i = 0; i < 40; ++i)  // more than the ring depth in flight
    put(root + "/sub/m" + std::to_string(i), "m" + std::to_string(i), 100 + 37 * (size_t)i);
  CHECK(::link((root + "/f4095").c_str(), (root + "/sub/hard").c_str()) == 0);
  CHECK(::link((root + "/f262145").c_str(), (root + "/sub/hard-large").c_str()) == 0);
  CHECK(::symlink("../f1", (root + "/sub/lnk").c_str()) == 0);
  int fd = ::open((root + "/sparse").c_str(), O_WRONLY | O_CREAT | O_CLOEXEC, 0644);
  CHECK(fd >= 0);
  CHECK(::pwrite(fd, "S", 1, 0) == 1);
  CHECK(::pwrite(fd, "E", 1, 4 << 20) == 1);
  ::close(fd);
  CHECK(::chmod((root + "/sub").c_str(), 0555) == 0);  // must still be fillable
}

static void compare(const std::string& src, const std::string& dst) {
  DIR* d = ::opendir(src.c_str());
  CHECK(d != nullptr);
  if (!d) return;
  while (struct dirent* e = ::readdir(d)) {
    std::string n(e->d_name);
    if (n == "." || n == "..") continue;
    struct stat a, b;
    CHECK(::lstat((src + "/" + n).c_str(), &a) == 0);
    if (::lstat((dst + "/" + n).c_str(), &b) != 0) {
      std::fprintf(stderr, "missing %s/%s\n", dst.c_str(), n.c_str());
      ++g_failed;
      continue;
    }
    CHECK((a.st_mode & S_IFMT) == (b.st_mode & S_IFMT));
    CHECK((a.st_mode & 07777) == (b.st_mode & 07777) || S_ISLNK(a.st_mode));
    if (S_ISDIR(a.st_mode)) {
      compare(src + "/" + n, dst + "/" + n);
    } else if (S_ISREG(a.st_mode)) {
      CHECK(a.st_size == b.st_size);
      CHECK(a.st_nlink == b.st_nlink);
      CHECK(a.st_mtim.tv_sec == b.st_mtim.tv_sec && a.st_mtim.tv_nsec == b.st_mtim.tv_nsec);
      CHECK(slurp(src + "/" + n) == slurp(dst + "/" + n));
    }
  }
  ::closedir(d);
}

// The short write: with SIGXFSZ ignored, a write across RLIMIT_FSIZE returns
// a short count first and EFBIG after it, as a full quota volume does before
// ENOSPC. Process-wide settings, hence the child.
static int short_write_child(const std::string& top) {
  ::signal(SIGXFSZ, SIG_IGN);
  struct rlimit lim = {100000, 100000};
  if (::setrlimit(RLIMIT_FSIZE, &lim) != 0) return 3;
  int bad = 0;
  for (int p = 0; p < 3; ++p) {
    const std::string dst = top + "/short-dst" + std::to_string(p);
    bool threw = false;
    try {
      iocopy::copy_tree(top + "/short-src", dst, kPaths[p]);
    } catch (const std::runtime_error& e) {
      threw = true;
    }
    struct stat st;
    bool is_short = ::lstat((dst + "/big").c_str(), &st) != 0 || st.st_size < 200000;
    if (!threw) {
      std::fprintf(stderr, "path %d: no exception, destination %s\n", p,
                   is_short ? "short" : "complete");
      ++bad;
    }
  }
  return bad ? 1 : 0;
}

int main() {
  char tmpl[] = "/tmp/iocopy-selftest-XXXXXX";
  const char* made = ::mkdtemp(tmpl);
  if (!made) {
    std::perror("mkdtemp");
    return 2;
  }
  const std::string top = made;
  const std::string src = top + "/src";
  build_tree(src);

  (void)iocopy::uring_available();
  const int fds_before = count_fds();

  // --- the three data paths ------------------------------------------------
  for (int p = 0; p < 3; ++p) {
    const std::string dst = top + "/dst" + std::to_string(p);
    try {
      iocopy::CopyStats s = iocopy::copy_tree(src, dst, kPaths[p]);
      CHECK(s.files == sizeof(kSizes) / sizeof(kSizes[0]) + 40 + 2 + 1);
      CHECK(s.symlinks == 1 && s.dirs == 1);
      CHECK(s.used_uring == (p == 0 && iocopy::uring_available()));
      compare(src, dst);
      struct stat st;
      CHECK(::lstat((dst + "/sparse").c_str(), &st) == 0 && st.st_size == (4 << 20) + 1);
      // a second run onto the filled destination replaces every entry
      iocopy::copy_tree(src, dst, kPaths[p]);
      compare(src, dst);
    } catch (const std::runtime_error& e) {
      std::fprintf(stderr, "path %d: %s\n", p, e.what());
      ++g_failed;
    }
    CHECK(count_fds() == fds_before);
  }

  // --- failing destination: a directory where the source has a file ---------
  for (int p = 0; p < 3; ++p) {
    const std::string dst = top + "/blocked" + std::to_string(p);
    CHECK(::mkdir(dst.c_str(), 0755) == 0 && ::mkdir((dst + "/sub").c_str(), 0755) == 0);
    CHECK(::mkdir((dst + "/sub/m20").c_str(), 0755) == 0);
    for (int round = 0; round < 20; ++round) {
      bool threw = false;
      try {
        iocopy::copy_tree(src, dst, kPaths[p]);
      } catch (const std::runtime_error&) {
        threw = true;
      }
      CHECK(threw);
      CHECK(count_fds() == fds_before);
    }
  }
  {
    bool threw = false;
    try {
      iocopy::copy_tree(top + "/never-existed", top + "/x");
    } catch (const std::runtime_error&) {
      threw = true;
    }
    CHECK(threw);
    threw = false;
    try {
      iocopy::copy_tree(src + "/f1", top + "/x");
    } catch (const std::runtime_error&) {
      threw = true;
    }
    CHECK(threw);
  }

  // --- short write ---------------------------------------------------------
  CHECK(::mkdir((top + "/short-src").c_str(), 0755) == 0);
  put(top + "/short-src/big", "big", 200000);
  std::fflush(nullptr);
  pid_t pid = ::fork();
  if (pid == 0) std::exit(short_write_child(top));  // exit(): LeakSanitizer runs there too
  int status = 0;
  CHECK(pid > 0 && ::waitpid(pid, &status, 0) == pid);
  CHECK(WIFEXITED(status) && WEXITSTATUS(status) == 0);

  CHECK(count_fds() == fds_before);
  rm_rf(top);

  if (g_failed) {
    std::fprintf(stderr, "iocopy selftest: %d check(s) FAILED\n", g_failed);
    return 1;
  }
  std::printf("iocopy selftest OK\n");
  return 0;
}
