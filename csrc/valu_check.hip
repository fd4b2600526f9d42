// Per-SIMD vector ALU check for the GPU burn-in (MI355X / gfx950).
//
// The other checks of /gpus/validate look at the matrix cores, the LDS and
// HBM, and every one of them trusts the vector ALU: cu_check's comparison
// side, gemm_check's verifier and the memtest's pattern generator run on it
// unchecked. This file makes every SIMD of every CU run five tests whose
// answers are known bit for bit, and say which SIMD it is:
//
//   int    32-bit mul lo / hi, 64-bit mad, add and sub, 32- and 64-bit
//          shifts, alignbit, bfe, popcount, count-leading-zeros, byte
//          permute, sad_u8, min / max, bfi
//   f32    fma, mul, add, sub, f32 -> i32, i32 -> f32, f32 -> f16, mul + add
//   f64    fma, mul, add, sub
//   pk16   packed fp16 fma, mul, add; packed f32 fma
//   trans  v_exp_f32, v_log_f32, v_rcp_f32, v_rsq_f32, v_sqrt_f32
//
// The generator, the step functions and the digest are in burnin_core.h
// (VALU section), where burnin_selftest.cpp runs the four exact tests on the
// CPU. A lane's answer for (test, round) is one u32 digest of kValuSteps
// results.
//
// Launch shape, as cu_check's and for its reason: 256 threads (four waves)
// and the largest dynamic LDS a workgroup may have, reserved and never
// touched, so exactly one workgroup fits per CU and its four waves spread
// over the four SIMDs. Each wave reads HW_REG_XCC_ID and HW_REG_HW_ID with
// s_getreg_b32; nothing is inferred from blockIdx. Every wave computes every
// (test, round): identical work on each SIMD.
//
// Check. Each lane compares its digest with want[test][round][lane], a u32
// table in device memory. For the four exact tests the host computes the
// table with the burnin_core.h code before the launch. trans has no host
// twin (the approximations' bits are the chip's own): its part of the table
// comes from a reference launch of one workgroup whose four waves each write
// a full copy. The host compares the copies; where they disagree the report
// says so, each odd wave counts as one trans error on its SIMD, and the
// majority copy is used (wave 0's where no three agree).
//
// Result: each wave writes its own 16-word sub-record with plain stores
// (kRec* below). No atomics, no spin-waits, nothing shared between
// workgroups; the kernel ends by itself whatever it finds.
//
// Detector self-test: inject entries {workgroup, test, round, wave, lane,
// xor_mask} flip bits of that lane's digest after the chain and before the
// compare. Entries change values only, never an address; the host rejects
// entries out of range.
//
// Included by hipcore.hip (needs the torch headers, <chrono>, <thread> and
// hipcore.hip's using-declarations of hip_host.h's resource owners).
#include "burnin_core.h"
#include "burnin_host.h"

namespace valu_check {

using namespace burnin;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

// One wave's sub-record, u32 words. kRecFirstTest holds test + 1, 0 = none.
constexpr int kRecValid = 0, kRecXcc = 1, kRecHwId = 2, kRecCounts = 3,
              kRecFirstTest = 8, kRecFirstRound = 9, kRecFirstLane = 10,
              kRecFirstExpected = 11, kRecFirstActual = 12, kRecWaveWords = 16;
constexpr int kRecWords = kWaves * kRecWaveWords;
constexpr u32 kRecMagic = 0x7A10C001u;

constexpr int kInjectWords = 6;
constexpr int kMaxInject = 64;
constexpr int kMaxRounds = 4096;
constexpr int kMaxGridMult = 8;
constexpr int kMaxLaunches = 8;  // cu_check's cap
constexpr int kTableThreads = 8;

// What one lane has seen so far. key orders first mismatches in time:
// (round*8 + test) << 6 | lane, ~0 = none.
struct LaneState {
  u32 cnt[kNumValuTests] = {0, 0, 0, 0, 0};
  u32 key = ~0u, expected = 0, actual = 0;
};

template <int TEST>
__device__ __forceinline__ void check_round(
    LaneState& st, const u32* __restrict__ want, int rounds, u32 base, u32 round,
    u32 wave, u32 lane, const u32* __restrict__ inject, int n_inject) {
  u32 d = valu_digest<TEST>(base, lane);
  for (int i = 0; i < n_inject; ++i) {
    const u32* e = inject + kInjectWords * i;
    if (e[0] == blockIdx.x && e[1] == (u32)TEST && e[2] == round && e[3] == wave &&
        e[4] == lane)
      d ^= e[5];
  }
  const u32 w = want[((size_t)TEST * rounds + round) * 64 + lane];
  if (d != w) {
    ++st.cnt[TEST];
    if (st.key == ~0u) {
      st.key = (round * 8 + TEST) << 6 | lane;
      st.expected = w;
      st.actual = d;
    }
  }
}

__global__ __launch_bounds__(kThreads) void valu_check_kernel(
    u32* __restrict__ out, const u32* __restrict__ want, int rounds, u32 seed_lo,
    u32 seed_hi, const u32* __restrict__ inject, int n_inject) {
  const u32 lane = threadIdx.x & 63;
  const u32 wave = threadIdx.x >> 6;

  u32 xcc, hw_id;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));

  LaneState st;
#pragma unroll 1
  for (u32 round = 0; round < (u32)rounds; ++round) {
    const u32 base = key_base(seed_lo, seed_hi, round);
    check_round<kValuInt>(st, want, rounds, base, round, wave, lane, inject, n_inject);
    check_round<kValuF32>(st, want, rounds, base, round, wave, lane, inject, n_inject);
    check_round<kValuF64>(st, want, rounds, base, round, wave, lane, inject, n_inject);
    check_round<kValuPk16>(st, want, rounds, base, round, wave, lane, inject, n_inject);
    check_round<kValuTrans>(st, want, rounds, base, round, wave, lane, inject, n_inject);
  }

  // per-wave fold: counts summed, earliest first mismatch wins
  u32 cnt[kNumValuTests];
  u32 key = st.key;
#pragma unroll
  for (int c = 0; c < kNumValuTests; ++c) cnt[c] = st.cnt[c];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int c = 0; c < kNumValuTests; ++c) cnt[c] += __shfl_xor(cnt[c], off, 64);
    key = min(key, (u32)__shfl_xor(key, off, 64));
  }
  const int src = (key == ~0u) ? 0 : (int)(key & 63u);
  const u32 f_expected = __shfl(st.expected, src, 64);
  const u32 f_actual = __shfl(st.actual, src, 64);
  if (lane == 0) {
    const bool any = key != ~0u;
    const u32 seq = key >> 6;  // round*8 + test
    u32x4* rec = reinterpret_cast<u32x4*>(
        out + (size_t)blockIdx.x * kRecWords + wave * kRecWaveWords);
    rec[0] = u32x4{kRecMagic, xcc, hw_id, cnt[0]};
    rec[1] = u32x4{cnt[1], cnt[2], cnt[3], cnt[4]};
    rec[2] = u32x4{any ? (seq & 7u) + 1u : 0u, any ? seq >> 3 : 0u,
                   any ? (u32)src : 0u, any ? f_expected : 0u};
    rec[3] = u32x4{any ? f_actual : 0u, 0u, 0u, 0u};
  }
}

// The reference launch of trans: one workgroup, each wave writes its own copy
// of the digests, copy[wave][round][lane], and its ids, ids[wave] = {xcc,
// hw_id}.
__global__ __launch_bounds__(kThreads) void valu_trans_reference_kernel(
    u32* __restrict__ copy, u32* __restrict__ ids, int rounds, u32 seed_lo,
    u32 seed_hi) {
  const u32 lane = threadIdx.x & 63;
  const u32 wave = threadIdx.x >> 6;
  u32 xcc, hw_id;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));
#pragma unroll 1
  for (u32 round = 0; round < (u32)rounds; ++round)
    copy[((size_t)wave * rounds + round) * 64 + lane] =
        valu_digest<kValuTrans>(key_base(seed_lo, seed_hi, round), lane);
  if (lane == 0) {
    ids[2 * wave] = xcc;
    ids[2 * wave + 1] = hw_id;
  }
}

// Every step's raw result bits of one (test, round) as one wave computes
// them: the numerics-testable surface. out[step][lane], hi << 32 | lo.
template <int TEST>
__global__ __launch_bounds__(64) void valu_values_kernel(u64* __restrict__ out,
                                                         u32 seed_lo, u32 seed_hi,
                                                         u32 round) {
  const u32 lane = threadIdx.x & 63;
  valu_round<TEST>(key_base(seed_lo, seed_hi, round), lane,
                   [&](u32 step, const ValuResult& r) {
                     out[step * 64 + lane] = (u64)(r.wide ? r.hi : 0u) << 32 | r.lo;
                   });
}

int parse_test(const std::string& name) {
  for (int i = 0; i < kNumValuTests; ++i)
    if (name == kValuTestNames[i]) return i;
  TORCH_CHECK(false, "valu_check: unknown test '", name, "'");
  return -1;
}

void check_rounds(long long rounds) {
  TORCH_CHECK(rounds >= 1 && rounds <= kMaxRounds, "rounds must be in [1, ",
              kMaxRounds, "]");
}

torch::Tensor valu_check_values(const std::string& test, long long round, u64 seed) {
  const int t = parse_test(test);
  TORCH_CHECK(round >= 0 && round < kMaxRounds, "valu_check: round must be in [0, ",
              kMaxRounds, ")");
  auto out = torch::empty(
      {(long long)kValuSteps, 64},
      torch::TensorOptions().dtype(torch::kInt64).device(torch::kCUDA));
  auto stream = at::hip::getCurrentHIPStream();
  u64* p = reinterpret_cast<u64*>(out.data_ptr<int64_t>());
  const SeedHalves s = split_seed(seed);
  constexpr void (*kKernels[kNumValuTests])(u64*, u32, u32, u32) = {
      valu_values_kernel<kValuInt>, valu_values_kernel<kValuF32>,
      valu_values_kernel<kValuF64>, valu_values_kernel<kValuPk16>,
      valu_values_kernel<kValuTrans>};
  hipLaunchKernelGGL(kKernels[t], dim3(1), dim3(64), 0, stream.stream(), p, s.lo,
                     s.hi, (u32)round);
  HIP_CHECK(hipGetLastError());
  return out;
}

// The host table of the four exact tests, table[test][round][lane], on up to
// kTableThreads threads (rounds are independent).
template <int TEST>
void table_rounds(u32* table, int rounds, int first, int stride, SeedHalves s) {
  for (int round = first; round < rounds; round += stride) {
    const u32 base = key_base(s.lo, s.hi, (u32)round);
    u32* row = table + ((size_t)TEST * rounds + round) * 64;
    for (u32 lane = 0; lane < 64; ++lane) row[lane] = valu_digest<TEST>(base, lane);
  }
}

void host_table(u32* table, int rounds, u64 seed) {
  const SeedHalves s = split_seed(seed);
  const int n = std::max(1, std::min({kTableThreads, rounds,
                                      (int)std::thread::hardware_concurrency()}));
  std::vector<std::thread> pool;
  for (int i = 0; i < n; ++i)
    pool.emplace_back([=] {
      table_rounds<kValuInt>(table, rounds, i, n, s);
      table_rounds<kValuF32>(table, rounds, i, n, s);
      table_rounds<kValuF64>(table, rounds, i, n, s);
      table_rounds<kValuPk16>(table, rounds, i, n, s);
    });
  for (auto& t : pool) t.join();
}

torch::Tensor valu_check_table(long long rounds, u64 seed) {
  check_rounds(rounds);
  std::vector<u32> table((size_t)kNumValuExact * rounds * 64);
  {
    py::gil_scoped_release release;
    host_table(table.data(), (int)rounds, seed);
  }
  auto out = torch::empty({(long long)kNumValuExact, rounds, 64},
                          torch::TensorOptions().dtype(torch::kInt64));
  int64_t* p = out.data_ptr<int64_t>();
  for (size_t i = 0; i < table.size(); ++i) p[i] = table[i];
  return out;
}

py::dict valu_check_geometry() {
  py::dict d;
  d["threads"] = kThreads;
  d["waves"] = kWaves;
  d["steps"] = kValuSteps;
  py::list tests;
  py::dict index, ops;
  for (int i = 0; i < kNumValuTests; ++i) {
    tests.append(std::string(kValuTestNames[i]));
    index[kValuTestNames[i]] = i;
    ops[kValuTestNames[i]] = kValuOps[i];
  }
  d["tests"] = tests;
  d["test_index"] = index;
  d["ops"] = ops;
  d["exact_tests"] = (int)kNumValuExact;
  py::dict win;
  win["f32"] = py::make_tuple(kValuF32ExpLo, kValuF32ExpHi);
  win["f64"] = py::make_tuple(kValuF64ExpLo, kValuF64ExpHi);
  win["f16"] = py::make_tuple(kValuF16ExpLo, kValuF16ExpHi);
  d["exponent_windows"] = win;
  d["pk16_span_bits"] = valu_pk16_span_bits(kValuF16ExpLo, kValuF16ExpHi);
  d["record_words"] = kRecWords;
  d["wave_record_words"] = kRecWaveWords;
  py::dict lay;
  lay["valid"] = kRecValid;
  lay["xcc"] = kRecXcc;
  lay["hw_id"] = kRecHwId;
  lay["counts"] = kRecCounts;
  lay["first_test"] = kRecFirstTest;
  lay["first_round"] = kRecFirstRound;
  lay["first_lane"] = kRecFirstLane;
  lay["first_expected"] = kRecFirstExpected;
  lay["first_actual"] = kRecFirstActual;
  d["wave_record_layout"] = lay;
  d["max_rounds"] = kMaxRounds;
  d["max_grid_mult"] = kMaxGridMult;
  d["max_launches"] = kMaxLaunches;
  d["max_inject"] = kMaxInject;
  d["inject_words"] = kInjectWords;
  return d;
}

// ---------------------------------------------------------------------------
// Driver
// ---------------------------------------------------------------------------

struct Inject {
  u32 workgroup, test, round, wave, lane, mask;
};

// What the reference launch of trans said.
struct TransReference {
  bool agree = true;
  bool majority = true;  // false: no three copies agreed, wave 0's is used
  u32 ids[2 * kWaves] = {};
  std::vector<int> odd_waves;
};

struct DriverResult {
  int launches = 0, grid = 0, cus = 0;
  double seconds = 0, table_seconds = 0;
  TransReference ref;
  std::vector<u32> words;  // launches * grid * kRecWords
};

inline u32 cu_key(u32 xcc, u32 hw_id) { return (xcc & 0xFu) << 8 | ((hw_id >> 8) & 0xFFu); }

// Picks the copy the table gets: the one at least three waves agree on, else
// wave 0's. Returns its wave.
int judge_reference(const std::vector<u32>& copies, size_t words, TransReference& ref) {
  auto same = [&](int a, int b) {
    return std::equal(copies.begin() + a * words, copies.begin() + (a + 1) * words,
                      copies.begin() + b * words);
  };
  int pick = 0;
  ref.majority = false;
  for (int a = 0; a < 2 && !ref.majority; ++a) {  // a majority holds wave 0 or 1
    int votes = 0;
    for (int b = 0; b < kWaves; ++b) votes += same(a, b);
    if (votes >= 3) {
      ref.majority = true;
      pick = a;
    }
  }
  for (int b = 0; b < kWaves; ++b)
    if (!same(pick, b)) ref.odd_waves.push_back(b);
  ref.agree = ref.odd_waves.empty();
  return pick;
}

DriverResult run_driver(int device, int rounds, u64 seed, int grid_mult,
                        const std::vector<Inject>& inject) {
  DriverResult out;

  DeviceScope scope(device);
  hipDeviceProp_t prop;
  HIP_CHECK(hipGetDeviceProperties(&prop, device));
  out.cus = prop.multiProcessorCount;
  const size_t lds_bytes = (prop.sharedMemPerBlockOptin / 16) * 16;
  // grid_mult 0: a single workgroup (the smallest launch there is)
  out.grid = grid_mult == 0 ? 1 : grid_mult * out.cus;
  for (auto& in : inject) {
    TORCH_CHECK(in.workgroup < (u32)out.grid, "inject: workgroup ", in.workgroup,
                " is outside the grid of ", out.grid);
    TORCH_CHECK(in.round < (u32)rounds, "inject: round ", in.round,
                " is outside the ", rounds, " rounds");
  }

  HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(valu_check_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds_bytes));

  const size_t round_words = (size_t)rounds * 64;
  std::vector<u32> table(kNumValuTests * round_words);
  const auto h0 = std::chrono::steady_clock::now();
  host_table(table.data(), rounds, seed);
  out.table_seconds =
      std::chrono::duration<double>(std::chrono::steady_clock::now() - h0).count();

  const SeedHalves sd = split_seed(seed);
  Stream stream;
  DeviceBuf<u32> want(device, table.size());
  {
    // trans: the chip's own bits, from one workgroup's four waves
    DeviceBuf<u32> copy(device, kWaves * round_words);
    DeviceBuf<u32> ids(device, 2 * kWaves);
    std::vector<u32> copies(kWaves * round_words);
    hipLaunchKernelGGL(valu_trans_reference_kernel, dim3(1), dim3(kThreads), 0,
                       stream.s, copy.ptr, ids.ptr, rounds, sd.lo, sd.hi);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(copies.data(), copy.ptr, copies.size() * sizeof(u32),
                             hipMemcpyDeviceToHost, stream.s));
    HIP_CHECK(hipMemcpyAsync(out.ref.ids, ids.ptr, sizeof(out.ref.ids),
                             hipMemcpyDeviceToHost, stream.s));
    stream.synchronize();
    const int pick = judge_reference(copies, round_words, out.ref);
    std::copy(copies.begin() + pick * round_words,
              copies.begin() + (pick + 1) * round_words,
              table.begin() + kValuTrans * round_words);
  }
  HIP_CHECK(hipMemcpyAsync(want.ptr, table.data(), table.size() * sizeof(u32),
                           hipMemcpyHostToDevice, stream.s));

  const size_t rec_words = (size_t)out.grid * kRecWords;
  const size_t rec_bytes = rec_words * sizeof(u32);
  DeviceBuf<u32> rec(device, rec_words);
  std::vector<u32> inj_host;
  for (auto& in : inject) {
    const u32 e[kInjectWords] = {in.workgroup, in.test, in.round,
                                 in.wave,      in.lane, in.mask};
    inj_host.insert(inj_host.end(), e, e + kInjectWords);
  }
  DeviceBuf<u32> inj(device, std::max<size_t>(inj_host.size(), 4));
  if (!inj_host.empty())
    HIP_CHECK(hipMemcpyAsync(inj.ptr, inj_host.data(), inj_host.size() * sizeof(u32),
                             hipMemcpyHostToDevice, stream.s));
  Event t0, t1;
  t0.record(stream);

  std::vector<u32> host(rec_words);
  std::vector<bool> seen(1u << 12, false);
  int distinct = 0;
  // On an idle GPU the first launch covers every CU; a busy one may need more.
  while (out.launches < kMaxLaunches) {
    HIP_CHECK(hipMemsetAsync(rec.ptr, 0, rec_bytes, stream.s));
    hipLaunchKernelGGL(valu_check_kernel, dim3(out.grid), dim3(kThreads), lds_bytes,
                       stream.s, rec.ptr, want.ptr, rounds, sd.lo, sd.hi, inj.ptr,
                       (int)inject.size());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(host.data(), rec.ptr, rec_bytes, hipMemcpyDeviceToHost,
                             stream.s));
    stream.synchronize();
    ++out.launches;
    for (int g = 0; g < out.grid; ++g) {
      const u32* w = host.data() + (size_t)g * kRecWords;
      for (int v = 0; v < kWaves; ++v)
        TORCH_CHECK(w[v * kRecWaveWords + kRecValid] == kRecMagic,
                    "valu_check: workgroup ", g, " wave ", v, " left no record");
      const u32 key = cu_key(w[kRecXcc], w[kRecHwId]);
      if (!seen[key]) {
        seen[key] = true;
        ++distinct;
      }
    }
    out.words.insert(out.words.end(), host.begin(), host.end());
    if (out.grid < out.cus || distinct >= out.cus) break;
  }
  t1.record(stream);
  t1.synchronize();
  out.seconds = Event::elapsed_ms(t0, t1) / 1e3;
  return out;
}

py::dict counts_dict(const u32* counts) {
  py::dict d;
  for (int c = 0; c < kNumValuTests; ++c) d[kValuTestNames[c]] = counts[c];
  return d;
}

// A wave's first mismatch, or None.
py::object first_dict(const u32* ww, int wave) {
  const u32 t = ww[kRecFirstTest];
  if (t == 0 || t > kNumValuTests) return py::none();
  py::dict f;
  f["test"] = std::string(kValuTestNames[t - 1]);
  f["round"] = ww[kRecFirstRound];
  f["wave"] = wave;
  f["lane"] = ww[kRecFirstLane];
  f["expected"] = ww[kRecFirstExpected];
  f["actual"] = ww[kRecFirstActual];
  return f;
}

py::dict valu_check(int device, int rounds, u64 seed, int grid_mult,
                    std::vector<std::vector<long long>> inject) {
  check_device(device);
  check_rounds(rounds);
  TORCH_CHECK(grid_mult >= 0 && grid_mult <= kMaxGridMult,
              "grid_mult must be in [0, ", kMaxGridMult, "]");
  TORCH_CHECK((int)inject.size() <= kMaxInject, "inject: at most ", kMaxInject,
              " entries");
  std::vector<Inject> inj;
  for (auto& e : inject) {
    TORCH_CHECK(e.size() == kInjectWords,
                "inject: entries are (workgroup, test, round, wave, lane, xor_mask)");
    for (long long x : e) check_inject_word(x);
    TORCH_CHECK(e[1] < kNumValuTests, "inject: test ", e[1], " is not one of 0..4");
    TORCH_CHECK(e[3] < kWaves, "inject: wave ", e[3], " is not one of 0..3");
    TORCH_CHECK(e[4] < 64, "inject: lane ", e[4], " is outside the wave");
    inj.push_back({(u32)e[0], (u32)e[1], (u32)e[2], (u32)e[3], (u32)e[4], (u32)e[5]});
  }
  DriverResult r;
  {
    py::gil_scoped_release release;
    r = run_driver(device, rounds, seed, grid_mult, inj);
  }
  py::list recs;
  const size_t nrec = r.words.size() / kRecWords;
  for (size_t i = 0; i < nrec; ++i) {
    const u32* w = r.words.data() + i * kRecWords;
    py::dict d;
    d["launch"] = (int)(i / r.grid);
    d["workgroup"] = (int)(i % r.grid);
    d["xcc"] = w[kRecXcc] & 0xFu;
    d["xcc_raw"] = w[kRecXcc];
    py::list hw, waves;
    u32 sum[kNumValuTests] = {0, 0, 0, 0, 0};
    // the workgroup's first: earliest (round, test), then the lowest wave
    int first_wave = -1;
    u32 first_seq = ~0u;
    for (int v = 0; v < kWaves; ++v) {
      const u32* ww = w + v * kRecWaveWords;
      hw.append(ww[kRecHwId]);
      for (int c = 0; c < kNumValuTests; ++c) sum[c] += ww[kRecCounts + c];
      py::dict wd;
      wd["counts"] = counts_dict(ww + kRecCounts);
      wd["first"] = first_dict(ww, v);
      waves.append(wd);
      if (ww[kRecFirstTest] != 0 && ww[kRecFirstTest] <= kNumValuTests) {
        const u32 seq = ww[kRecFirstRound] * 8 + ww[kRecFirstTest] - 1;
        if (seq < first_seq) {
          first_seq = seq;
          first_wave = v;
        }
      }
    }
    d["hw_id"] = hw;
    d["counts"] = counts_dict(sum);
    d["waves"] = waves;
    d["first"] = first_wave < 0 ? py::object(py::none())
                                : first_dict(w + first_wave * kRecWaveWords, first_wave);
    recs.append(d);
  }

  py::dict ref;
  py::list ref_hw, odd;
  for (int v = 0; v < kWaves; ++v) ref_hw.append(r.ref.ids[2 * v + 1]);
  for (int v : r.ref.odd_waves) odd.append(v);
  ref["agree"] = r.ref.agree;
  ref["xcc"] = r.ref.ids[0] & 0xFu;
  ref["xcc_raw"] = r.ref.ids[0];
  ref["hw_id"] = ref_hw;
  ref["odd_waves"] = odd;
  ref["used"] = r.ref.agree ? "all" : r.ref.majority ? "majority" : "wave0";
  if (!r.ref.agree) {
    // the reference workgroup's own record: one trans error per odd wave
    py::dict d;
    d["launch"] = -1;
    d["workgroup"] = 0;
    d["xcc"] = r.ref.ids[0] & 0xFu;
    d["xcc_raw"] = r.ref.ids[0];
    d["hw_id"] = ref_hw;
    py::list waves;
    u32 sum[kNumValuTests] = {0, 0, 0, 0, 0};
    for (int v = 0; v < kWaves; ++v) {
      u32 c[kNumValuTests] = {0, 0, 0, 0, 0};
      c[kValuTrans] = std::count(r.ref.odd_waves.begin(), r.ref.odd_waves.end(), v);
      sum[kValuTrans] += c[kValuTrans];
      py::dict wd;
      wd["counts"] = counts_dict(c);
      wd["first"] = py::none();
      waves.append(wd);
    }
    d["counts"] = counts_dict(sum);
    d["waves"] = waves;
    d["first"] = py::none();
    recs.append(d);
  }

  py::dict d;
  d["records"] = recs;
  d["launches"] = r.launches;
  d["grid"] = r.grid;
  d["rounds"] = rounds;
  d["seconds"] = r.seconds;
  d["table_seconds"] = r.table_seconds;
  d["trans_reference"] = ref;
  return d;
}

}  // namespace valu_check
