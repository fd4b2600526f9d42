// HBM pattern memory test for the GPU burn-in (MI355X / gfx950).
//
// The throughput tiers of /gpus/validate never look at the data they move.
// This file writes a seeded pattern over a buffer, reads it back and reports
// every 64-bit word that differs: a weak HBM stack, a stuck bit or an
// aliasing address line shows here and nowhere else.
//
// The unit is the 64-bit word. Word g (a global u64 index: base_word plus
// the position in the buffer) holds, for a u64 seed:
//
//   fmix32(h): h^=h>>16; h*=0x85EBCA6B; h^=h>>13; h*=0xC2B2AE35; h^=h>>16
//
//   "addr":  w = g ^ seed                     (address-in-address: aliasing)
//   "rand":  x = g ^ seed; a = (u32)x; b = (u32)(x >> 32)
//            lo = fmix32(a + b*0x9E3779B9)
//            hi = fmix32(~a + b*0x85EBCA77 + 0x27D4EB2F)
//            w  = (u64)hi << 32 | lo          (every bit toggles: stuck cells)
//   "zero":  w = 0                            (scrub)
//   invert:  w = ~w
//
// One templated kernel, three modes: write, verify, verify_flip (verify,
// then store the complement of the EXPECTED word, so a transient error is
// reported once and a stuck cell again by the next verify).
//
// Access shape (CDNA4 guide §2): the 16-byte-aligned body moves 16 B per
// lane, 1 KiB per wave instruction. A workgroup walks tiles of
// kBlock * kUnroll vectors; a full tile issues its kUnroll independent
// loads before the first compare (as copy_f32x4_x4_kernel does), and the
// grid strides over tiles with a cap of kMaxGrid workgroups (8 per CU on a
// 256-CU chip). The buffer is only guaranteed 8-byte aligned: a leading and
// a trailing odd word are handled word by word in the same launch. Every
// index and byte offset is 64-bit.
//
// fmix32 and the word patterns themselves (pattern_word, pattern_pair) are in
// burnin_core.h, where burnin_selftest.cpp runs them on the CPU.
//
// Included by hipcore.hip (needs the torch headers and hipcore.hip's
// using-declarations of hip_host.h's resource owners).
#include "burnin_core.h"
#include "burnin_host.h"

namespace hbm_memtest {

using namespace burnin;

constexpr int kBlock = 256;
constexpr int kUnroll = 4;                    // 16-B vectors per lane per tile
constexpr int kWordsPerThreadIter = 2 * kUnroll;
constexpr int kMaxGrid = 2048;
constexpr u64 kTileVecs = (u64)kBlock * kUnroll;

enum Mode { kWrite = 0, kVerify = 1, kVerifyFlip = 2 };

// Device-side report, all u64: [0] mismatching words, [1] OR of
// expected^actual, [2] record slots claimed, then cap records {g, expected,
// actual}.
constexpr int kRepErrors = 0, kRepBits = 1, kRepClaimed = 2, kRepHeader = 3,
              kRecWords = 3;

// Mismatch slow path: one claimed record per bad word while slots are left.
__device__ __noinline__ void record_mismatch(u64* rep, u64 cap, u64 g,
                                             u64 expected, u64 actual) {
  u64* r;
  if (!claim_record<kRepClaimed, kRepHeader, kRecWords>(rep, cap, r)) return;
  r[0] = g;
  r[1] = expected;
  r[2] = actual;
}

__device__ inline void check_word(u64* rep, u64 cap, u64 g, u64 expected,
                                  u64 actual, u32& cnt, u64& bits) {
  u64 d = expected ^ actual;
  if (d != 0) {
    ++cnt;
    bits |= d;
    record_mismatch(rep, cap, g, expected, actual);
  }
}

template <int MODE, int PAT>
__device__ inline void do_word(u64* p, u64 g, u64 seed, u64 inv, u64* rep,
                               u64 cap, u32& cnt, u64& bits) {
  u64 e = pattern_word<PAT>(g, seed, inv);
  if (MODE == kWrite) {
    *p = e;
    return;
  }
  u64 a = *p;
  check_word(rep, cap, g, e, a, cnt, bits);
  if (MODE == kVerifyFlip) *p = ~e;
}

template <int MODE, int PAT>
__global__ __launch_bounds__(kBlock) void memtest_kernel(
    u64* __restrict__ p, u64 n, u64 base, u64 seed, u64 inv,
    u64* __restrict__ rep, u64 cap) {
  const u64 head = ((reinterpret_cast<uintptr_t>(p) & 8) != 0 && n > 0) ? 1 : 0;
  const u64 nvec = (n - head) >> 1;
  const bool tail = ((n - head) & 1) != 0;
  ulonglong2* __restrict__ v = reinterpret_cast<ulonglong2*>(p + head);
  const u64 gbody = base + head;
  const u64 ntiles = (nvec + kTileVecs - 1) / kTileVecs;

  u32 cnt = 0;   // mismatching words seen by this lane
  u64 bits = 0;  // OR of expected ^ actual seen by this lane

  for (u64 t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const u64 v0 = t * kTileVecs + threadIdx.x;
    const HiTerms hi =
        tile_terms(gbody + 2 * t * kTileVecs, 2 * kTileVecs, seed);
    if ((t + 1) * kTileVecs <= nvec) {
      ulonglong2 a[kUnroll];
      if (MODE != kWrite) {
#pragma unroll
        for (int j = 0; j < kUnroll; ++j) a[j] = v[v0 + (u64)j * kBlock];
      }
#pragma unroll
      for (int j = 0; j < kUnroll; ++j) {
        const u64 vi = v0 + (u64)j * kBlock;
        const u64 g0 = gbody + 2 * vi;
        ulonglong2 e;
        pattern_pair<PAT>(g0, seed, inv, hi, e.x, e.y);
        if (MODE == kWrite) {
          v[vi] = e;
        } else {
          if (((a[j].x ^ e.x) | (a[j].y ^ e.y)) != 0) {
            check_word(rep, cap, g0, e.x, a[j].x, cnt, bits);
            check_word(rep, cap, g0 + 1, e.y, a[j].y, cnt, bits);
          }
          if (MODE == kVerifyFlip) {
            e.x = ~e.x;
            e.y = ~e.y;
            v[vi] = e;
          }
        }
      }
    } else {
      // last, partial tile: every vector bounds-checked
      for (int j = 0; j < kUnroll; ++j) {
        const u64 vi = v0 + (u64)j * kBlock;
        if (vi >= nvec) break;
        const u64 g0 = gbody + 2 * vi;
        ulonglong2 e;
        pattern_pair<PAT>(g0, seed, inv, hi, e.x, e.y);
        if (MODE == kWrite) {
          v[vi] = e;
        } else {
          ulonglong2 a = v[vi];
          check_word(rep, cap, g0, e.x, a.x, cnt, bits);
          check_word(rep, cap, g0 + 1, e.y, a.y, cnt, bits);
          if (MODE == kVerifyFlip) {
            e.x = ~e.x;
            e.y = ~e.y;
            v[vi] = e;
          }
        }
      }
    }
  }

  // the odd words either side of the 16-byte-aligned body
  if (blockIdx.x == 0) {
    if (threadIdx.x == 0 && head)
      do_word<MODE, PAT>(p, base, seed, inv, rep, cap, cnt, bits);
    if (threadIdx.x == 1 && tail)
      do_word<MODE, PAT>(p + (n - 1), base + (n - 1), seed, inv, rep, cap, cnt,
                         bits);
  }

  if (MODE != kWrite) {
    // per-wave reduction, then at most one atomic pair per wave, and none
    // from a wave that saw no mismatch
    u64 c = cnt;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      c += __shfl_xor(c, off, 64);
      bits |= __shfl_xor(bits, off, 64);
    }
    if ((threadIdx.x & 63) == 0 && c != 0) {
      atomicAdd(&rep[kRepErrors], c);
      atomicOr(&rep[kRepBits], bits);
    }
  }
}

// The instantiations as [mode][pattern].
constexpr void (*kKernels[3][3])(u64*, u64, u64, u64, u64, u64*, u64) = {
    {memtest_kernel<kWrite, kAddr>, memtest_kernel<kWrite, kRand>,
     memtest_kernel<kWrite, kZero>},
    {memtest_kernel<kVerify, kAddr>, memtest_kernel<kVerify, kRand>,
     memtest_kernel<kVerify, kZero>},
    {memtest_kernel<kVerifyFlip, kAddr>, memtest_kernel<kVerifyFlip, kRand>,
     memtest_kernel<kVerifyFlip, kZero>},
};

// The one launch path, shared by the tensor bindings and the driver. rep may
// be null for kWrite only.
void launch(int mode, int pat, u64* p, u64 n, u64 base, u64 seed, bool invert,
            u64* rep, u64 cap, hipStream_t s) {
  if (n == 0) return;
  TORCH_CHECK((reinterpret_cast<uintptr_t>(p) & 7) == 0,
              "memtest: buffer must be 8-byte aligned");
  TORCH_CHECK(mode == kWrite || rep != nullptr, "memtest: verify needs a report");
  const u64 head = (reinterpret_cast<uintptr_t>(p) & 8) ? 1 : 0;
  const u64 nvec = (n - head) >> 1;
  const u64 ntiles = (nvec + kTileVecs - 1) / kTileVecs;
  dim3 grid((unsigned)std::min<u64>(std::max<u64>(ntiles, 1), kMaxGrid));
  const u64 inv = invert ? ~0ull : 0ull;
  TORCH_CHECK(mode >= 0 && mode < 3, "unknown memtest mode ", mode);
  TORCH_CHECK(pat >= 0 && pat < 3, "unknown memtest pattern code ", pat);
  hipLaunchKernelGGL(kKernels[mode][pat], grid, dim3(kBlock), 0, s, p, n, base,
                     seed, inv, rep, cap);
  HIP_CHECK(hipGetLastError());
}

int parse_pattern(const std::string& name) {
  if (name == "addr") return kAddr;
  if (name == "rand") return kRand;
  if (name == "zero") return kZero;
  TORCH_CHECK(false, "memtest pattern must be 'addr', 'rand' or 'zero', got '",
              name, "'");
  return -1;
}

// ---------------------------------------------------------------------------
// Tensor bindings: the numerics-testable surface
// ---------------------------------------------------------------------------

void check_tensor(const torch::Tensor& t) {
  TORCH_CHECK(t.is_cuda(), "memtest: tensor must be on the GPU");
  TORCH_CHECK(t.scalar_type() == torch::kInt64, "memtest: int64 only");
  TORCH_CHECK(t.dim() == 1 && t.is_contiguous(),
              "memtest: 1-D contiguous tensor required");
  int cur = -1;
  HIP_CHECK(hipGetDevice(&cur));
  TORCH_CHECK(t.get_device() == cur, "memtest: tensor is on device ",
              t.get_device(), " but the current device is ", cur);
}

void memtest_write(torch::Tensor t, const std::string& pattern, u64 seed,
                   u64 base_word, bool invert) {
  check_tensor(t);
  int pat = parse_pattern(pattern);
  auto stream = at::hip::getCurrentHIPStream();
  launch(kWrite, pat, reinterpret_cast<u64*>(t.data_ptr<int64_t>()),
         (u64)t.numel(), base_word, seed, invert, nullptr, 0, stream.stream());
}

py::dict report_dict(const u64* h, u64 cap) {
  py::dict d;
  d["errors"] = py::int_(h[kRepErrors]);
  d["bad_bits"] = py::int_(h[kRepBits]);
  py::list recs;
  u64 nrec = std::min<u64>(h[kRepClaimed], cap);
  for (u64 i = 0; i < nrec; ++i) {
    const u64* r = h + kRepHeader + kRecWords * i;
    recs.append(py::make_tuple(py::int_(r[0]), py::int_(r[1]), py::int_(r[2])));
  }
  d["records"] = recs;
  return d;
}

py::dict verify_tensor(int mode, torch::Tensor t, const std::string& pattern,
                       u64 seed, u64 base_word, bool invert,
                       long long max_records) {
  check_tensor(t);
  int pat = parse_pattern(pattern);
  u64 cap = check_max_records(max_records);
  auto rep = torch::zeros({(int64_t)(kRepHeader + kRecWords * cap)}, t.options());
  auto stream = at::hip::getCurrentHIPStream();
  launch(mode, pat, reinterpret_cast<u64*>(t.data_ptr<int64_t>()),
         (u64)t.numel(), base_word, seed, invert,
         reinterpret_cast<u64*>(rep.data_ptr<int64_t>()), cap, stream.stream());
  auto host = rep.cpu();  // synchronises with the current stream
  return report_dict(reinterpret_cast<const u64*>(host.data_ptr<int64_t>()),
                     cap);
}

py::dict memtest_verify(torch::Tensor t, const std::string& pattern, u64 seed,
                        u64 base_word, bool invert, long long max_records) {
  return verify_tensor(kVerify, t, pattern, seed, base_word, invert,
                       max_records);
}

py::dict memtest_verify_flip(torch::Tensor t, const std::string& pattern,
                             u64 seed, u64 base_word, bool invert,
                             long long max_records) {
  return verify_tensor(kVerifyFlip, t, pattern, seed, base_word, invert,
                       max_records);
}

py::dict memtest_geometry() {
  py::dict d;
  d["block"] = kBlock;
  d["words_per_thread_iter"] = kWordsPerThreadIter;
  d["max_grid"] = kMaxGrid;
  return d;
}

// ---------------------------------------------------------------------------
// Driver: the burn-in pass over chunks of its own (DeviceBuf, never torch's
// caching allocator)
// ---------------------------------------------------------------------------

struct StepRecord {
  const char* step;
  u64 g, expected, actual;
};

struct DriverResult {
  u64 bytes = 0, errors = 0, bad_bits = 0;
  int passes = 0;
  double write_ms = 0, verify_ms = 0, seconds = 0;
  std::vector<StepRecord> records;
};

// The driver's steps in run order; an inject entry names one by its index.
constexpr int kInjectSteps = 6;
constexpr const char* kStepNames[kInjectSteps] = {
    "write addr",  "verify addr",      "write rand",
    "verify rand", "verify_flip rand", "verify rand inverted"};
constexpr int kDefaultInjectStep = 1;

// Detector self-test: XOR mask into the word at position `word` of the words
// under test, behind the kernel's back, immediately before step `step`.
struct Inject {
  u64 word, mask;
  int step;
};

// (word, xor_mask[, step]) entries; needs the GIL.
std::vector<Inject> parse_inject(const py::sequence& entries) {
  std::vector<Inject> out;
  for (py::handle h : entries) {
    TORCH_CHECK(py::isinstance<py::sequence>(h),
                "inject: an entry must be (word, xor_mask[, step])");
    auto e = py::reinterpret_borrow<py::sequence>(h);
    TORCH_CHECK(e.size() == 2 || e.size() == 3,
                "inject: an entry must be (word, xor_mask[, step]), got ",
                e.size(), " elements");
    Inject in{e[0].cast<u64>(), e[1].cast<u64>(), kDefaultInjectStep};
    if (e.size() == 3) {
      long long step = e[2].cast<long long>();
      TORCH_CHECK(step >= 0 && step < kInjectSteps, "inject: step ", step,
                  " is outside 0..", kInjectSteps - 1);
      in.step = (int)step;
    }
    out.push_back(in);
  }
  return out;
}

DriverResult run_driver(int device, const std::vector<u64>& chunk_words,
                        u64 seed, u64 cap, bool scrub,
                        const std::vector<Inject>& inject, u64 base_word) {
  DriverResult out;
  u64 total_words = 0;
  for (u64 w : chunk_words) total_words += w;
  out.bytes = total_words * 8;
  for (auto& in : inject)
    TORCH_CHECK(in.word < total_words, "inject: word ", in.word,
                " is outside the ", total_words, " words under test");

  DeviceScope scope(device);
  std::vector<DeviceBuf<u64>> chunks;
  for (u64 w : chunk_words) chunks.emplace_back(device, w);
  const size_t rep_words = kRepHeader + kRecWords * cap;
  DeviceBuf<u64> rep(device, rep_words);
  std::vector<u64> host_rep(rep_words);

  Stream stream;
  Event t0, t1, w0, w1;
  w0.record(stream);

  // One step = one mode over ALL chunks: with >= 1 GiB under test every line
  // has left the 256 MiB Infinity Cache before the next step reads it, so
  // the read-back comes from HBM.
  int steps_run = 0;
  auto step = [&](const char* name, int mode, int pat, bool invert) {
    // every earlier step has ended with stream.synchronize()
    for (auto& in : inject) {
      if (in.step != steps_run) continue;
      u64 off = 0;
      size_t c = 0;
      while (in.word - off >= chunk_words[c]) off += chunk_words[c++];
      u64* addr = chunks[c].ptr + (in.word - off);
      u64 word = 0;
      HIP_CHECK(hipMemcpy(&word, addr, 8, hipMemcpyDeviceToHost));
      word ^= in.mask;
      HIP_CHECK(hipMemcpy(addr, &word, 8, hipMemcpyHostToDevice));
    }
    ++steps_run;
    if (mode != kWrite)
      HIP_CHECK(hipMemsetAsync(rep.ptr, 0, rep_words * 8, stream.s));
    t0.record(stream);
    u64 g = base_word;
    for (size_t i = 0; i < chunks.size(); ++i) {
      launch(mode, pat, chunks[i].ptr, chunk_words[i], g, seed, invert, rep.ptr,
             cap, stream.s);
      g += chunk_words[i];
    }
    t1.record(stream);
    if (mode != kWrite)
      HIP_CHECK(hipMemcpyAsync(host_rep.data(), rep.ptr, rep_words * 8,
                               hipMemcpyDeviceToHost, stream.s));
    stream.synchronize();
    const float ms = Event::elapsed_ms(t0, t1);
    ++out.passes;
    if (mode == kWrite) {
      if (pat != kZero) out.write_ms += ms;
      return;
    }
    out.verify_ms += ms;
    out.errors += host_rep[kRepErrors];
    out.bad_bits |= host_rep[kRepBits];
    u64 nrec = std::min<u64>(host_rep[kRepClaimed], cap);
    for (u64 i = 0; i < nrec && out.records.size() < cap; ++i) {
      const u64* r = host_rep.data() + kRepHeader + kRecWords * i;
      out.records.push_back({name, r[0], r[1], r[2]});
    }
  };

  step(kStepNames[0], kWrite, kAddr, false);
  step(kStepNames[1], kVerify, kAddr, false);
  step(kStepNames[2], kWrite, kRand, false);
  step(kStepNames[3], kVerify, kRand, false);
  step(kStepNames[4], kVerifyFlip, kRand, false);
  step(kStepNames[5], kVerify, kRand, true);
  if (scrub) step("scrub", kWrite, kZero, false);

  w1.record(stream);
  w1.synchronize();
  out.seconds = Event::elapsed_ms(w0, w1) / 1e3;
  return out;
}

// inject entries are (word, xor_mask[, step]): word is a position within the
// words under test, step the index into kStepNames of the step the flip comes
// immediately before (two elements mean "verify addr"). base_word is the g of
// the first chunk's first word; a record's g is base_word + position.
py::dict hbm_memtest(int device, std::vector<u64> chunk_bytes, u64 seed,
                     long long max_records, bool scrub,
                     const py::sequence& inject_entries, u64 base_word) {
  u64 cap = check_max_records(max_records);
  const std::vector<Inject> inject = parse_inject(inject_entries);
  check_device(device);
  TORCH_CHECK(!chunk_bytes.empty(), "chunk_bytes must not be empty");
  std::vector<u64> words;
  for (u64 b : chunk_bytes) {
    TORCH_CHECK(b > 0 && b % 8 == 0,
                "every chunk must be a positive multiple of 8 bytes, got ", b);
    words.push_back(b / 8);
  }
  DriverResult r;
  {
    py::gil_scoped_release release;
    r = run_driver(device, words, seed, cap, scrub, inject, base_word);
  }
  py::dict d;
  d["bytes_tested"] = py::int_(r.bytes);
  d["passes"] = r.passes;
  d["errors"] = py::int_(r.errors);
  d["bad_bits"] = py::int_(r.bad_bits);
  py::list recs;
  for (auto& rec : r.records) {
    py::dict e;
    e["step"] = std::string(rec.step);
    e["g"] = py::int_(rec.g);
    e["expected"] = py::int_(rec.expected);
    e["actual"] = py::int_(rec.actual);
    recs.append(e);
  }
  d["records"] = recs;
  // bytes counted once per pass: 2 timed write steps, 4 timed verify steps
  d["write_gbps"] = r.write_ms > 0 ? 2.0 * r.bytes / (r.write_ms * 1e6) : 0.0;
  d["verify_gbps"] = r.verify_ms > 0 ? 4.0 * r.bytes / (r.verify_ms * 1e6) : 0.0;
  d["seconds"] = r.seconds;
  return d;
}

}  // namespace hbm_memtest
