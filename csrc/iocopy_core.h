// Native bulk copy engine: io_uring small-file batching + in-kernel
// copy_file_range for large files (raw syscalls — liburing is not present).
//
// Replaces the reference's two data movers (SURVEY.md §2.4 row "Data
// migration"): the shell tar pipe for the container writable layer
// (the reference's utils/copy.go:17-27) and the throwaway-ubuntu-container
// `mv` for volumes (utils/copy.go:74-128). Design, from measuring a
// rootfs-shaped tree (thousands of 4 KiB files + a few GiB of large files):
//
//   * LARGE files are copied with extent-aware copy_file_range — fully
//     in-kernel (reflink/server-side copy capable), no user-space bounce;
//     holes found via SEEK_DATA/SEEK_HOLE are never touched. Small files that
//     have holes take this path too.
//   * SMALL files (<= 256 KiB) dominate syscall count, not bytes: they are
//     batched through ONE io_uring — up to 16 files in flight, each a READ
//     then a WRITE (resubmitted until the whole length has moved) —
//     amortizing ring submissions across files.
//   * metadata preserved everywhere: mode/uid/gid/mtime, symlinks, hardlinks
//     (within one call), device nodes (overlayfs whiteouts are 0:0 char
//     devices), xattrs (overlayfs opaque markers).
//   * graceful fallback at every level: no io_uring (seccomp/EPERM) ->
//     copy_file_range loop; no copy_file_range (EXDEV on old kernels) ->
//     pread/pwrite. Options can force either fallback.
//   * the copy never leaves the destination tree: an existing destination
//     entry that is not a directory is unlinked, never opened or followed.
//   * a file never arrives shorter than its lstat size without an exception,
//     and an exception leaves no descriptor, DIR handle or in-flight ring
//     request behind.
//
// No pybind11 in here: csrc/iocopy.cpp binds it as
// gpu_docker_api_amd.ops._iocopy, csrc/iocopy_selftest.cpp drives it
// stand-alone under the host sanitizers. Errors are thrown as
// std::runtime_error.
#pragma once

#ifndef _GNU_SOURCE
#define _GNU_SOURCE
#endif

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <climits>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include <dirent.h>
#include <fcntl.h>
#include <linux/io_uring.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/syscall.h>
#include <sys/types.h>
#include <sys/xattr.h>
#include <unistd.h>

namespace iocopy {

struct Options {
  bool use_uring = true;            // false: small files go file by file
  bool use_copy_file_range = true;  // false: pread/pwrite bounce
};

struct CopyStats {
  unsigned long long files = 0, dirs = 0, symlinks = 0, specials = 0;
  unsigned long long bytes = 0;  // each inode once
  bool used_uring = false;
};

namespace detail {

[[noreturn]] inline void die(const std::string& what) {
  throw std::runtime_error(what + ": " + std::strerror(errno));
}

constexpr size_t kChunk = 1 << 20;           // 1 MiB large-file bounce chunk
constexpr unsigned kDepth = 16;              // files in flight in the ring
constexpr size_t kSmallCutoff = 256 * 1024;  // <= this: batched via io_uring
constexpr size_t kBatchJobs = 4096;          // bound memory for the job list

// Descriptors and DIR handles close on every way out of a scope.
class Fd {
 public:
  Fd() = default;
  explicit Fd(int fd) : fd_(fd) {}
  Fd(const Fd&) = delete;
  Fd& operator=(const Fd&) = delete;
  Fd(Fd&& o) noexcept : fd_(o.fd_) { o.fd_ = -1; }
  Fd& operator=(Fd&& o) noexcept {
    if (this != &o) {
      reset();
      fd_ = o.fd_;
      o.fd_ = -1;
    }
    return *this;
  }
  ~Fd() { reset(); }
  void reset() {
    if (fd_ >= 0) ::close(fd_);
    fd_ = -1;
  }
  int get() const { return fd_; }
  bool ok() const { return fd_ >= 0; }

 private:
  int fd_ = -1;
};

struct DirCloser {
  void operator()(DIR* d) const {
    if (d) ::closedir(d);
  }
};
using Dir = std::unique_ptr<DIR, DirCloser>;

// ---------------------------------------------------------------------------
// Minimal io_uring wrapper (setup/enter via raw syscalls)
// ---------------------------------------------------------------------------

inline int sys_io_uring_setup(unsigned entries, struct io_uring_params* p) {
  return (int)syscall(__NR_io_uring_setup, entries, p);
}
inline int sys_io_uring_enter(int fd, unsigned to_submit, unsigned min_complete,
                              unsigned flags) {
  return (int)syscall(__NR_io_uring_enter, fd, to_submit, min_complete, flags,
                      nullptr, 0);
}

class Ring {
 public:
  static constexpr unsigned kEntries = 64;

  Ring() = default;
  Ring(const Ring&) = delete;
  Ring& operator=(const Ring&) = delete;

  bool init() {
    std::memset(&params_, 0, sizeof(params_));
    fd_ = sys_io_uring_setup(kEntries, &params_);
    if (fd_ < 0) return false;

    sring_sz_ = params_.sq_off.array + params_.sq_entries * sizeof(unsigned);
    cring_sz_ = params_.cq_off.cqes + params_.cq_entries * sizeof(io_uring_cqe);
    bool single_mmap = params_.features & IORING_FEAT_SINGLE_MMAP;
    if (single_mmap && cring_sz_ > sring_sz_) sring_sz_ = cring_sz_;

    sq_ptr_ = mmap(nullptr, sring_sz_, PROT_READ | PROT_WRITE,
                   MAP_SHARED | MAP_POPULATE, fd_, IORING_OFF_SQ_RING);
    if (sq_ptr_ == MAP_FAILED) return false;
    cq_ptr_ = single_mmap
                  ? sq_ptr_
                  : mmap(nullptr, cring_sz_, PROT_READ | PROT_WRITE,
                         MAP_SHARED | MAP_POPULATE, fd_, IORING_OFF_CQ_RING);
    if (cq_ptr_ == MAP_FAILED) return false;
    sqes_sz_ = params_.sq_entries * sizeof(io_uring_sqe);
    sqes_ = (io_uring_sqe*)mmap(nullptr, sqes_sz_,
                                PROT_READ | PROT_WRITE, MAP_SHARED | MAP_POPULATE,
                                fd_, IORING_OFF_SQES);
    if (sqes_ == MAP_FAILED) return false;

    auto* sq = (char*)sq_ptr_;
    sq_tail_ = (std::atomic<unsigned>*)(sq + params_.sq_off.tail);
    sq_mask_ = *(unsigned*)(sq + params_.sq_off.ring_mask);
    sq_array_ = (unsigned*)(sq + params_.sq_off.array);
    auto* cq = (char*)cq_ptr_;
    cq_head_ = (std::atomic<unsigned>*)(cq + params_.cq_off.head);
    cq_tail_ = (std::atomic<unsigned>*)(cq + params_.cq_off.tail);
    cq_mask_ = *(unsigned*)(cq + params_.cq_off.ring_mask);
    cqes_ = (io_uring_cqe*)(cq + params_.cq_off.cqes);
    ok_ = true;
    return true;
  }

  bool ok() const { return ok_; }

  void queue(unsigned op, int fd, void* buf, unsigned len, off_t off,
             unsigned long long user_data) {
    unsigned tail = sq_tail_->load(std::memory_order_relaxed);
    unsigned idx = tail & sq_mask_;
    io_uring_sqe* sqe = &sqes_[idx];
    std::memset(sqe, 0, sizeof(*sqe));
    sqe->opcode = op;
    sqe->fd = fd;
    sqe->addr = (unsigned long long)buf;
    sqe->len = len;
    sqe->off = (unsigned long long)off;
    sqe->user_data = user_data;
    sq_array_[idx] = idx;
    sq_tail_->store(tail + 1, std::memory_order_release);
    ++pending_submit_;
  }

  // Hands the queued SQEs to the kernel and optionally waits for `wait`
  // completions. False with errno set when the kernel refuses.
  bool try_submit(unsigned wait) {
    if (pending_submit_ == 0 && wait == 0) return true;
    for (;;) {
      int ret = sys_io_uring_enter(fd_, pending_submit_, wait,
                                   wait ? IORING_ENTER_GETEVENTS : 0);
      if (ret >= 0) {
        pending_submit_ -= std::min<unsigned>(pending_submit_, (unsigned)ret);
        return true;
      }
      if (errno != EINTR) return false;
    }
  }

  void submit(unsigned wait) {
    if (!try_submit(wait)) die("io_uring_enter");
  }

  bool pop(unsigned long long* user_data, int* res) {
    unsigned head = cq_head_->load(std::memory_order_relaxed);
    if (head == cq_tail_->load(std::memory_order_acquire)) return false;
    io_uring_cqe* cqe = &cqes_[head & cq_mask_];
    *user_data = cqe->user_data;
    *res = cqe->res;
    cq_head_->store(head + 1, std::memory_order_release);
    return true;
  }

  void wait_one() { submit(1); }

  // Error path: submits what is still queued and reaps until `outstanding`
  // requests have completed, so the kernel holds no pointer into a slot
  // buffer any more. False if the kernel refuses to be waited on.
  bool drain(unsigned outstanding) {
    unsigned long long ud;
    int res;
    while (outstanding > 0) {
      if (pop(&ud, &res)) {
        --outstanding;
        continue;
      }
      if (!try_submit(1)) return false;
    }
    return true;
  }

  ~Ring() {
    // closing the fd does NOT unmap the rings — without these munmaps a
    // long-lived daemon leaks ~2 pages per copy_tree call (found as ~8.6
    // KB/cycle RSS creep in a 15-minute churn soak)
    if (sqes_ != nullptr && sqes_ != MAP_FAILED) munmap(sqes_, sqes_sz_);
    if (cq_ptr_ != nullptr && cq_ptr_ != MAP_FAILED && cq_ptr_ != sq_ptr_)
      munmap(cq_ptr_, cring_sz_);
    if (sq_ptr_ != nullptr && sq_ptr_ != MAP_FAILED) munmap(sq_ptr_, sring_sz_);
    if (fd_ >= 0) close(fd_);
  }

 private:
  int fd_ = -1;
  bool ok_ = false;
  io_uring_params params_{};
  void* sq_ptr_ = nullptr;
  void* cq_ptr_ = nullptr;
  size_t sring_sz_ = 0;
  size_t cring_sz_ = 0;
  size_t sqes_sz_ = 0;
  io_uring_sqe* sqes_ = nullptr;
  std::atomic<unsigned>* sq_tail_ = nullptr;
  unsigned sq_mask_ = 0;
  unsigned* sq_array_ = nullptr;
  std::atomic<unsigned>* cq_head_ = nullptr;
  std::atomic<unsigned>* cq_tail_ = nullptr;
  unsigned cq_mask_ = 0;
  io_uring_cqe* cqes_ = nullptr;
  unsigned pending_submit_ = 0;
};

// ---------------------------------------------------------------------------
// Metadata
// ---------------------------------------------------------------------------

inline void copy_xattrs(const std::string& src, const std::string& dst) {
  ssize_t list_sz = llistxattr(src.c_str(), nullptr, 0);
  if (list_sz <= 0) return;
  std::vector<char> names(list_sz);
  list_sz = llistxattr(src.c_str(), names.data(), names.size());
  if (list_sz <= 0) return;
  std::vector<char> value;
  for (char* p = names.data(); p < names.data() + list_sz;) {
    std::string name(p);
    p += name.size() + 1;
    ssize_t vs = lgetxattr(src.c_str(), name.c_str(), nullptr, 0);
    if (vs < 0) continue;
    value.resize(vs);
    vs = lgetxattr(src.c_str(), name.c_str(), value.data(), value.size());
    if (vs < 0) continue;
    // best-effort: security.* may need privileges we lack
    (void)lsetxattr(dst.c_str(), name.c_str(), value.data(), vs, 0);
  }
}

inline void copy_meta(const std::string& dst, const struct stat& st) {
  int rc = lchown(dst.c_str(), st.st_uid, st.st_gid);
  (void)rc;
  // after the chown, which clears setuid/setgid
  if (!S_ISLNK(st.st_mode)) (void)chmod(dst.c_str(), st.st_mode & 07777);
  struct timespec times[2] = {st.st_atim, st.st_mtim};
  (void)utimensat(AT_FDCWD, dst.c_str(), times, AT_SYMLINK_NOFOLLOW);
}

// The destination entry is replaced, never opened: whatever non-directory
// is there (a regular file that may have other names, a symlink that may
// point out of the tree) is unlinked, and the new file is created with
// O_EXCL | O_NOFOLLOW. A directory in the way fails with EEXIST.
inline Fd create_dst_file(const std::string& dst) {
  if (unlink(dst.c_str()) != 0 && errno != ENOENT && errno != EISDIR && errno != EPERM)
    die("unlink " + dst);
  Fd fd(open(dst.c_str(), O_WRONLY | O_CREAT | O_EXCL | O_NOFOLLOW | O_CLOEXEC, 0600));
  if (!fd.ok()) die("open " + dst);
  return fd;
}

// Directories are created owner-writable so that they can be filled whatever
// the source's mode is; the final mode arrives with the deferred metadata.
// A non-directory in the way (a symlink above all) is replaced.
inline void make_dst_dir(const std::string& dst) {
  if (mkdir(dst.c_str(), 0700) == 0) return;
  if (errno != EEXIST) die("mkdir " + dst);
  struct stat have;
  if (lstat(dst.c_str(), &have) != 0) die("lstat " + dst);
  if (S_ISDIR(have.st_mode)) {
    if ((have.st_mode & 0700) != 0700)
      (void)chmod(dst.c_str(), (have.st_mode & 07777) | 0700);
    return;
  }
  if (unlink(dst.c_str()) != 0) die("unlink " + dst);
  if (mkdir(dst.c_str(), 0700) != 0) die("mkdir " + dst);
}

// ---------------------------------------------------------------------------
// Large-file copy: extent-aware, in-kernel
// ---------------------------------------------------------------------------

inline std::vector<std::pair<off_t, off_t>> data_extents(int fd, off_t size) {
  std::vector<std::pair<off_t, off_t>> out;
  off_t pos = 0;
  while (pos < size) {
    off_t data = lseek(fd, pos, SEEK_DATA);
    if (data < 0) {
      if (errno == ENXIO) break;          // trailing hole
      out.push_back({pos, size});         // SEEK_DATA unsupported: whole file
      break;
    }
    if (data >= size) break;
    off_t hole = lseek(fd, data, SEEK_HOLE);
    if (hole < 0 || hole > size) hole = size;
    out.push_back({data, hole});
    pos = hole;
  }
  return out;
}

inline void copy_data_large(int in_fd, int out_fd, off_t size, const std::string& name,
                            bool use_cfr) {
  auto extents = data_extents(in_fd, size);
  if (ftruncate(out_fd, size) != 0) die("ftruncate " + name);
  std::vector<char> buf;
  for (auto [start, end] : extents) {
    off_t off = start;
    while (off < end) {
      size_t want = (size_t)std::min<off_t>((off_t)(8 * kChunk), end - off);
      if (use_cfr) {
        off_t off_out = off;
        ssize_t n = copy_file_range(in_fd, &off, out_fd, &off_out, want, 0);
        if (n > 0) continue;  // both offsets advanced by the kernel
        // EXDEV / unsupported / an error: the bounce below either works or
        // names the error
        use_cfr = false;
      }
      // plain pread/pwrite with explicit offsets
      if (buf.empty()) buf.resize(kChunk);
      ssize_t r = pread(in_fd, buf.data(), std::min(want, kChunk), off);
      if (r < 0) {
        if (errno == EINTR) continue;
        die("pread " + name);
      }
      if (r == 0)
        throw std::runtime_error("pread " + name + ": end of file at " + std::to_string(off) +
                                 " of " + std::to_string(size));
      ssize_t w = 0;
      while (w < r) {
        ssize_t k = pwrite(out_fd, buf.data() + w, r - w, off + w);
        if (k < 0) {
          if (errno == EINTR) continue;
          die("pwrite " + name);
        }
        if (k == 0) throw std::runtime_error("pwrite " + name + ": wrote nothing");
        w += k;
      }
      off += r;
    }
  }
}

// ---------------------------------------------------------------------------
// Small-file copy: batched across files through one io_uring
// ---------------------------------------------------------------------------

struct FileJob {
  std::string src, dst;
  struct stat st;
};

struct Slot {
  std::unique_ptr<char[]> buf;
  Fd in_fd, out_fd;
  size_t len = 0;   // the file's length
  size_t done = 0;  // bytes of the current phase that have moved
  size_t job_idx = 0;
  bool reading = false;
};

inline void finish_file(const FileJob& job) {
  copy_xattrs(job.src, job.dst);
  copy_meta(job.dst, job.st);
}

inline void copy_file_direct(const FileJob& job, bool use_cfr) {
  Fd in_fd(open(job.src.c_str(), O_RDONLY | O_CLOEXEC));
  if (!in_fd.ok()) die("open " + job.src);
  Fd out_fd = create_dst_file(job.dst);
  copy_data_large(in_fd.get(), out_fd.get(), job.st.st_size, job.dst, use_cfr);
  in_fd.reset();
  out_fd.reset();
  finish_file(job);
}

// The slots of one batch. Members are destroyed in reverse order, and the
// destructor body runs before any of them: on an exception it first reaps
// every request the kernel still holds, and only then are the descriptors
// closed and the buffers freed. If the kernel cannot be waited on, the
// buffers are given up (leaked) instead of freed under a pending read.
struct Batch {
  Ring& ring;
  std::vector<Slot> slots;
  unsigned in_flight = 0;  // queued or submitted, completion not yet popped

  explicit Batch(Ring& r) : ring(r), slots(kDepth) {
    for (auto& s : slots) s.buf.reset(new char[kSmallCutoff]);
  }
  ~Batch() {
    if (in_flight > 0 && !ring.drain(in_flight))
      for (auto& s : slots) (void)s.buf.release();
  }
};

inline void copy_small_batch(Ring& ring, const std::vector<FileJob>& jobs,
                             CopyStats& stats, const Options& opt) {
  if (!ring.ok()) {
    for (const auto& j : jobs) copy_file_direct(j, opt.use_copy_file_range);
    return;
  }
  stats.used_uring = stats.used_uring || !jobs.empty();
  Batch batch(ring);
  std::vector<unsigned> free_slots;
  for (unsigned i = 0; i < kDepth; ++i) free_slots.push_back(i);

  size_t next_job = 0;

  auto start_next = [&]() -> bool {
    if (next_job >= jobs.size() || free_slots.empty()) return false;
    const FileJob& job = jobs[next_job];
    unsigned si = free_slots.back();
    Slot& s = batch.slots[si];
    s.in_fd = Fd(open(job.src.c_str(), O_RDONLY | O_CLOEXEC));
    if (!s.in_fd.ok()) die("open " + job.src);
    s.out_fd = create_dst_file(job.dst);
    s.job_idx = next_job++;
    s.len = (size_t)job.st.st_size;
    s.done = 0;
    if (s.len == 0) {  // nothing to move
      s.in_fd.reset();
      s.out_fd.reset();
      finish_file(job);
      return true;
    }
    free_slots.pop_back();
    s.reading = true;
    ring.queue(IORING_OP_READ, s.in_fd.get(), s.buf.get(), (unsigned)s.len, 0, si);
    ++batch.in_flight;
    return true;
  };

  while (start_next()) {
  }
  ring.submit(0);

  while (batch.in_flight > 0) {
    unsigned long long ud;
    int res;
    if (!ring.pop(&ud, &res)) {
      ring.wait_one();
      continue;
    }
    --batch.in_flight;
    Slot& s = batch.slots[ud];
    const FileJob& job = jobs[s.job_idx];
    if (res < 0) {
      errno = -res;
      die(s.reading ? "io_uring read " + job.src : "io_uring write " + job.dst);
    }
    if (res == 0)  // the file shrank, or the device takes no more
      throw std::runtime_error((s.reading ? "io_uring read " + job.src
                                          : "io_uring write " + job.dst) +
                               ": stopped at " + std::to_string(s.done) + " of " +
                               std::to_string(s.len) + " bytes");
    s.done += (size_t)res;
    if (s.done < s.len) {  // short read or write: go on where it stopped
      ring.queue(s.reading ? IORING_OP_READ : IORING_OP_WRITE,
                 s.reading ? s.in_fd.get() : s.out_fd.get(), s.buf.get() + s.done,
                 (unsigned)(s.len - s.done), (off_t)s.done, ud);
      ++batch.in_flight;
      ring.submit(0);
    } else if (s.reading) {
      s.reading = false;
      s.done = 0;
      ring.queue(IORING_OP_WRITE, s.out_fd.get(), s.buf.get(), (unsigned)s.len, 0, ud);
      ++batch.in_flight;
      ring.submit(0);
    } else {
      s.in_fd.reset();
      s.out_fd.reset();
      finish_file(job);
      free_slots.push_back((unsigned)ud);
      while (start_next()) {
      }
      ring.submit(0);
    }
  }
}

// ---------------------------------------------------------------------------
// Tree walk
// ---------------------------------------------------------------------------

struct Walker {
  Ring& ring;
  Options opt;
  std::map<std::pair<dev_t, ino_t>, std::string> hardlinks;  // inode -> first dst name
  std::vector<FileJob> small;
  // further names of small files: their first name exists only once its
  // batch has been written
  std::vector<std::pair<std::string, FileJob>> deferred_links;
  std::vector<std::pair<std::string, struct stat>> dir_meta;
  CopyStats stats;

  Walker(Ring& r, const Options& o) : ring(r), opt(o) {}

  // A filesystem that cannot link (or has run out of links) gets a second
  // copy of the data rather than a failed migration; anything else raises.
  void make_link(const std::string& first, const FileJob& job) {
    if (unlink(job.dst.c_str()) != 0 && errno != ENOENT && errno != EISDIR && errno != EPERM)
      die("unlink " + job.dst);
    if (link(first.c_str(), job.dst.c_str()) == 0) return;
    if (errno != EPERM && errno != EMLINK && errno != EXDEV && errno != EOPNOTSUPP)
      die("link " + job.dst);
    copy_file_direct(job, opt.use_copy_file_range);
    stats.bytes += (unsigned long long)job.st.st_size;
  }

  void flush_small() {
    copy_small_batch(ring, small, stats, opt);
    small.clear();
    for (const auto& l : deferred_links) make_link(l.first, l.second);
    deferred_links.clear();
  }

  void walk_children(const std::string& src, const std::string& dst) {
    Dir d(opendir(src.c_str()));
    if (!d) die("opendir " + src);
    while (dirent* e = readdir(d.get())) {
      std::string n(e->d_name);
      if (n == "." || n == "..") continue;
      walk(src + "/" + n, dst + "/" + n);
    }
  }

  void walk(const std::string& src, const std::string& dst) {
    struct stat st;
    if (lstat(src.c_str(), &st) != 0) die("lstat " + src);

    if (S_ISDIR(st.st_mode)) {
      make_dst_dir(dst);
      ++stats.dirs;
      walk_children(src, dst);
      copy_xattrs(src, dst);
      dir_meta.push_back({dst, st});  // applied last (mtime survives fills)
      return;
    }

    if (S_ISLNK(st.st_mode)) {
      std::vector<char> target(st.st_size ? st.st_size + 1 : PATH_MAX);
      ssize_t n = readlink(src.c_str(), target.data(), target.size() - 1);
      if (n < 0) die("readlink " + src);
      target[n] = 0;
      (void)unlink(dst.c_str());
      if (symlink(target.data(), dst.c_str()) != 0) die("symlink " + dst);
      copy_meta(dst, st);
      ++stats.symlinks;
      return;
    }

    if (S_ISCHR(st.st_mode) || S_ISBLK(st.st_mode) || S_ISFIFO(st.st_mode) ||
        S_ISSOCK(st.st_mode)) {
      // overlayfs whiteouts are 0:0 char devices — must be replicated
      (void)unlink(dst.c_str());
      if (mknod(dst.c_str(), st.st_mode, st.st_rdev) != 0) {
        ++stats.specials;  // unprivileged: cannot mknod; skip
        return;
      }
      copy_xattrs(src, dst);
      copy_meta(dst, st);
      ++stats.specials;
      return;
    }

    // regular file
    const bool sparse = (off_t)st.st_blocks * 512 < st.st_size;
    const bool is_small = (size_t)st.st_size <= kSmallCutoff && !sparse;
    ++stats.files;
    if (st.st_nlink > 1) {
      auto key = std::make_pair(st.st_dev, st.st_ino);
      auto it = hardlinks.find(key);
      if (it != hardlinks.end()) {
        if (is_small) {
          deferred_links.push_back({it->second, {src, dst, st}});
          if (deferred_links.size() >= kBatchJobs) flush_small();
        } else
          make_link(it->second, {src, dst, st});
        return;
      }
      hardlinks[key] = dst;
    }
    stats.bytes += (unsigned long long)st.st_size;
    if (is_small) {
      small.push_back({src, dst, st});
      if (small.size() >= kBatchJobs) flush_small();
      return;
    }
    copy_file_direct({src, dst, st}, opt.use_copy_file_range);
  }
};

}  // namespace detail

inline CopyStats copy_tree(const std::string& src, const std::string& dst,
                           const Options& opt = Options()) {
  using namespace detail;
  struct stat st;
  if (lstat(src.c_str(), &st) != 0) die("lstat " + src);
  if (!S_ISDIR(st.st_mode)) throw std::runtime_error(src + " is not a directory");

  Ring ring;
  if (opt.use_uring) (void)ring.init();  // failure => per-file fallback paths

  bool made_root = mkdir(dst.c_str(), 0700) == 0;
  if (!made_root && errno != EEXIST) die("mkdir " + dst);

  Walker w(ring, opt);
  w.walk_children(src, dst);
  w.flush_small();
  copy_xattrs(src, dst);
  for (auto it = w.dir_meta.rbegin(); it != w.dir_meta.rend(); ++it)
    copy_meta(it->first, it->second);
  // an existing destination root keeps its own mode, as before
  if (made_root) (void)chmod(dst.c_str(), st.st_mode & 07777);
  return w.stats;
}

inline bool uring_available() {
  detail::Ring r;
  return r.init();
}

}  // namespace iocopy
