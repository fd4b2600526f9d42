// Per-CU MFMA and LDS check for the GPU burn-in (MI355X / gfx950).
//
// The throughput tiers of /gpus/validate time the matrix cores and never
// look at a result, and they judge a GPU as a whole. This file makes every
// compute unit compute tiles whose answer is known exactly, compare them on
// the spot, pattern-test its whole LDS, and say which CU it is: a CU that now
// and then returns a wrong accumulator shows here with its XCC, SE, SH and CU
// id, and nowhere else.
//
// Launch shape: 256 threads (four waves) and the largest dynamic LDS a
// workgroup may have (160 KiB on MI355X), so exactly one workgroup fits per
// CU and the first multiProcessorCount workgroups of a launch on an idle GPU
// land on distinct CUs. Each wave reads HW_REG_XCC_ID and HW_REG_HW_ID with
// s_getreg_b32; nothing is inferred from blockIdx.
//
// Generator. With a u64 seed (seed_lo, seed_hi its halves), format index fmt
// (0 bf16, 1 MX-fp8 e4m3, 2 MX-fp4 e2m1), tile t, operand (0 = A, 1 = B),
// row 0..15 (for B: the column of the result) and k:
//
//   fmix32(h): h^=h>>16; h*=0x85EBCA6B; h^=h>>13; h*=0xC2B2AE35; h^=h>>16
//
//   u = fmix32(fmix32(seed_lo + t*0x9E3779B9) ^ seed_hi
//              ^ (fmt<<28 | operand<<20 | row<<12 | k))
//
//   bf16:  m = (u % 255) - 127, value m/16
//   e4m3:  j = u % 65; code 0x00 for j = 0, otherwise with q = j-1
//          code = (q>>5)<<7 | (6 + ((q&31)>>3))<<3 | (q&7)
//          (zero and every code with exponent field 6..9: multiples of 2^-4
//          up to 7.5)
//   e2m1:  code = u & 15 (multiples of 1/2 up to 6)
//
// The tile is C[16][16] = A[16][K] * B[16][K]^T with K = 1024 / 1152 / 1280.
// Every product is an integer multiple of the squared granule and every
// partial sum stays below 2^24 of them, so the fp32 result is exact whatever
// the order of summation. Operands are never loaded: each lane generates its
// own fragment (bf16: A[l&15][32s + 8(l>>4) + j]; MX: k = 128s + 32(l>>4) + j,
// fp4 low nibble = even k in the low 4 dwords; both scales 127 = x1.0).
//
// Check. Each lane recomputes its four outputs (row = 4(l>>4) + reg, col =
// l&15) with integer VALU arithmetic in units of the granule, converts the
// sum to fp32 (exact) and compares bit patterns with the accumulators: two
// independent datapaths of one CU, no expected values from the host. Every
// workgroup computes the same tiles (wave w, round r: tile 4r + w).
//
// LDS, per round: all words w are filled with fmix32(w*0x9E3779B9 + seed_lo
// + round) by 16-byte stores, verified by a thread of another wave and lane
// than the writer, overwritten with the complement of the EXPECTED word,
// and verified again by a third thread.
//
// Result: each wave writes its own 16-word sub-record with plain stores
// (kRec* below); a workgroup's record is its four sub-records. No atomics,
// no spin-waits, nothing shared between workgroups; the kernel ends by
// itself whatever it finds.
//
// Detector self-test: inject entries {workgroup, test, tile_or_round,
// lane_or_word, xor_mask, sub} flip bits of accumulator register sub (0..3)
// of the named lane (after the chain, before the compare) or of the named
// LDS word, in phase sub: 0 between fill and first verify, 1 between the
// first verify's complement store and the second verify. sub may be left
// out and is then 0. Entries change values only, never an address; the host
// rejects entries out of range and the kernel bounds the LDS word again.
//
// fmix32 and the generator's elem_code / elem_int are in burnin_core.h, where
// burnin_selftest.cpp runs them on the CPU; this check draws every format at
// its full range (bf16 127, e4m3 4, e2m1 16).
//
// Included by hipcore.hip (needs the torch headers and hipcore.hip's
// using-declarations of hip_host.h's resource owners).
#include "burnin_core.h"
#include "burnin_host.h"

namespace cu_check {

using namespace burnin;
using i32x8 = __attribute__((ext_vector_type(8))) int;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

// The three formats, then the LDS test.
constexpr int kLds = kNumFormats, kNumTests = kNumFormats + 1;
constexpr int kK[kNumFormats] = {1024, 1152, 1280};
const char* const kTestNames[kNumTests] = {"bf16", "fp8", "fp4", "lds"};

// One wave's sub-record, u32 words. kRecFirstTest holds test + 1, 0 = none.
constexpr int kRecValid = 0, kRecXcc = 1, kRecHwId = 2, kRecCounts = 3,
              kRecFirstTest = 7, kRecFirstIndex = 8, kRecFirstLane = 9,
              kRecFirstReg = 10, kRecFirstExpected = 11, kRecFirstActual = 12,
              kRecWaveWords = 16;
constexpr int kRecWords = kWaves * kRecWaveWords;
constexpr u32 kRecMagic = 0xC0C4EC01u;

constexpr int kInjectWords = 6;
constexpr int kLdsPhases = 2;
constexpr int kMaxInject = 64;
constexpr int kMaxRounds = 65536;
constexpr int kMaxGridMult = 8;
constexpr int kMaxLaunches = 8;
constexpr int kMaxTile = kMaxRounds * kWaves;

template <int FMT>
__device__ __forceinline__ u32 gen(u32 base, u32 operand, u32 row, u32 k) {
  return fmix32(base ^ ((u32)FMT << 28 | operand << 20 | row << 12 | k));
}

// The element of draw u as the MFMA wants it, and as an integer count of
// operand granules: the generator at the format's full range.
template <int FMT>
__device__ __forceinline__ u32 code(u32 u) {
  return elem_code<FMT, kFullRange[FMT]>(u);
}
template <int FMT>
__device__ __forceinline__ int numer(u32 u) {
  return elem_int<FMT, kFullRange[FMT]>(u);
}

// The MFMA chain of one tile, one wave.
template <int FMT>
__device__ __forceinline__ f32x4 mfma_tile(u32 base, int lane) {
  const u32 row = lane & 15;
  const u32 kq = lane >> 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (FMT == kBf16) {
#pragma unroll 1
    for (u32 s = 0; s < kK[kBf16] / 32; ++s) {
      const u32 k0 = s * 32 + kq * 8;
      u32x4 a, b;
#pragma unroll
      for (u32 j = 0; j < 4; ++j) {
        a[j] = code<FMT>(gen<FMT>(base, 0, row, k0 + 2 * j)) |
               code<FMT>(gen<FMT>(base, 0, row, k0 + 2 * j + 1)) << 16;
        b[j] = code<FMT>(gen<FMT>(base, 1, row, k0 + 2 * j)) |
               code<FMT>(gen<FMT>(base, 1, row, k0 + 2 * j + 1)) << 16;
      }
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          __builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0,
          0, 0);
    }
  } else if (FMT == kFp8) {
#pragma unroll 1
    for (u32 s = 0; s < kK[kFp8] / 128; ++s) {
      const u32 k0 = s * 128 + kq * 32;
      i32x8 a, b;
#pragma unroll
      for (u32 d = 0; d < 8; ++d) {
        u32 wa = 0, wb = 0;
#pragma unroll
        for (u32 j = 0; j < 4; ++j) {
          wa |= code<FMT>(gen<FMT>(base, 0, row, k0 + 4 * d + j)) << (8 * j);
          wb |= code<FMT>(gen<FMT>(base, 1, row, k0 + 4 * d + j)) << (8 * j);
        }
        a[d] = (int)wa;
        b[d] = (int)wb;
      }
      acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, acc, 0, 0, 0,
                                                             127, 0, 127);
    }
  } else {
#pragma unroll 1
    for (u32 s = 0; s < kK[kFp4] / 128; ++s) {
      const u32 k0 = s * 128 + kq * 32;
      i32x8 a = {0, 0, 0, 0, 0, 0, 0, 0}, b = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (u32 d = 0; d < 4; ++d) {
        u32 wa = 0, wb = 0;
#pragma unroll
        for (u32 j = 0; j < 8; ++j) {
          wa |= code<FMT>(gen<FMT>(base, 0, row, k0 + 8 * d + j)) << (4 * j);
          wb |= code<FMT>(gen<FMT>(base, 1, row, k0 + 8 * d + j)) << (4 * j);
        }
        a[d] = (int)wa;
        b[d] = (int)wb;
      }
      acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, acc, 4, 4, 0,
                                                             127, 0, 127);
    }
  }
  return acc;
}

// What this lane's four outputs must be, by integer arithmetic.
template <int FMT>
__device__ __forceinline__ f32x4 expect_tile(u32 base, int lane) {
  const u32 col = lane & 15;
  const u32 row0 = (lane >> 4) * 4;
  int sum[4] = {0, 0, 0, 0};
#pragma unroll 2
  for (u32 k = 0; k < (u32)kK[FMT]; ++k) {
    const int b = numer<FMT>(gen<FMT>(base, 1, col, k));
#pragma unroll
    for (u32 r = 0; r < 4; ++r)
      sum[r] += numer<FMT>(gen<FMT>(base, 0, row0 + r, k)) * b;
  }
  f32x4 e;
#pragma unroll
  for (int r = 0; r < 4; ++r) e[r] = (float)sum[r] * (1.0f / kInvGranule[FMT]);
  return e;
}

// What one lane has seen so far. key orders first mismatches in time:
// (round*8 + step) << 6 | lane, ~0 = none.
struct LaneState {
  u32 cnt[kNumTests] = {0, 0, 0, 0};
  u32 key = ~0u, test = 0, index = 0, reg = 0, expected = 0, actual = 0;
};

__device__ __forceinline__ void note(LaneState& st, u32 test, u32 seq,
                                     u32 lane, u32 index, u32 reg,
                                     u32 expected, u32 actual) {
  ++st.cnt[test];
  if (st.key == ~0u) {
    st.key = seq << 6 | lane;
    st.test = test;
    st.index = index;
    st.reg = reg;
    st.expected = expected;
    st.actual = actual;
  }
}

template <int FMT>
__device__ __forceinline__ void check_tile(
    LaneState& st, u32 seed_lo, u32 seed_hi, u32 round, u32 t, int lane,
    const u32* __restrict__ inject, int n_inject) {
  const u32 base = key_base(seed_lo, seed_hi, t);
  f32x4 acc = mfma_tile<FMT>(base, lane);
  for (int i = 0; i < n_inject; ++i) {
    const u32* e = inject + kInjectWords * i;
    if (e[0] == blockIdx.x && e[1] == (u32)FMT && e[2] == t && e[3] == (u32)lane) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        // through a scalar, as in the compare below
        const float a = acc[r];
        if (e[5] == (u32)r) acc[r] = __uint_as_float(__float_as_uint(a) ^ e[4]);
      }
    }
  }
  const f32x4 want = expect_tile<FMT>(base, lane);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    // through scalars: a bit_cast applied to a vector element reads element 0
    const float wf = want[r], af = acc[r];
    const u32 eb = __float_as_uint(wf);
    const u32 ab = __float_as_uint(af);
    if (eb != ab) note(st, FMT, round * 8 + FMT, lane, t, r, eb, ab);
  }
}

__device__ inline u32x4 lds_pattern(u32 vec, u32 salt) {
  u32x4 e;
#pragma unroll
  for (u32 j = 0; j < 4; ++j) e[j] = fmix32((4 * vec + j) * kGolden + salt);
  return e;
}

// Verify the vectors thread `owner` is responsible for against the pattern
// xor inv; with FLIP store the complement of what was expected.
template <bool FLIP>
__device__ __forceinline__ void lds_verify(
    u32x4* lds, u32 lds_vecs, u32 owner, u32 salt, u32 inv, LaneState& st,
    u32 seq, u32 round, int lane) {
  for (u32 v = owner; v < lds_vecs; v += kThreads) {
    const u32x4 got = lds[v];
    u32x4 e = lds_pattern(v, salt);
#pragma unroll
    for (u32 j = 0; j < 4; ++j) {
      e[j] ^= inv;
      if (got[j] != e[j]) note(st, kLds, seq, lane, round, 4 * v + j, e[j], got[j]);
    }
    if (FLIP) lds[v] = ~e;
  }
}

// Apply the LDS inject entries of this workgroup, round and phase. n_inject
// is uniform over the grid, so every thread takes the barrier or none does.
__device__ __forceinline__ void lds_inject(u32x4* lds, u32 lds_vecs, u32 tid,
                                           u32 round, u32 phase,
                                           const u32* __restrict__ inject,
                                           int n_inject) {
  if (n_inject > 0) {
    if (tid == 0) {
      for (int i = 0; i < n_inject; ++i) {
        const u32* e = inject + kInjectWords * i;
        if (e[0] == blockIdx.x && e[1] == (u32)kLds && e[2] == round &&
            e[3] < 4 * lds_vecs && e[5] == phase)
          reinterpret_cast<u32*>(lds)[e[3]] ^= e[4];
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kThreads) void cu_check_kernel(
    u32* __restrict__ out, int rounds, u32 seed_lo, u32 seed_hi, u32 lds_vecs,
    const u32* __restrict__ inject, int n_inject) {
  extern __shared__ u32x4 cu_check_lds[];
  u32x4* lds = cu_check_lds;
  const u32 tid = threadIdx.x;
  const int lane = tid & 63;
  const u32 wave = tid >> 6;

  u32 xcc, hw_id;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));

  LaneState st;
  for (u32 round = 0; round < (u32)rounds; ++round) {
    const u32 t = round * kWaves + wave;
    check_tile<kBf16>(st, seed_lo, seed_hi, round, t, lane, inject, n_inject);
    check_tile<kFp8>(st, seed_lo, seed_hi, round, t, lane, inject, n_inject);
    check_tile<kFp4>(st, seed_lo, seed_hi, round, t, lane, inject, n_inject);

    const u32 salt = seed_lo + round;
    for (u32 v = tid; v < lds_vecs; v += kThreads) lds[v] = lds_pattern(v, salt);
    __syncthreads();
    lds_inject(lds, lds_vecs, tid, round, 0, inject, n_inject);
    // another wave AND another lane than the writer, twice
    lds_verify<true>(lds, lds_vecs, (tid + 65) & (kThreads - 1), salt, 0u, st,
                     round * 8 + 3, round, lane);
    __syncthreads();
    lds_inject(lds, lds_vecs, tid, round, 1, inject, n_inject);
    lds_verify<false>(lds, lds_vecs, (tid + 130) & (kThreads - 1), salt, ~0u, st,
                      round * 8 + 4, round, lane);
    __syncthreads();
  }

  // per-wave fold: counts summed, earliest first mismatch wins
  u32 cnt[kNumTests];
  u32 key = st.key;
#pragma unroll
  for (int c = 0; c < kNumTests; ++c) cnt[c] = st.cnt[c];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int c = 0; c < kNumTests; ++c) cnt[c] += __shfl_xor(cnt[c], off, 64);
    key = min(key, (u32)__shfl_xor(key, off, 64));
  }
  const int src = (key == ~0u) ? 0 : (int)(key & 63u);
  const u32 f_test = __shfl(st.test, src, 64);
  const u32 f_index = __shfl(st.index, src, 64);
  const u32 f_reg = __shfl(st.reg, src, 64);
  const u32 f_expected = __shfl(st.expected, src, 64);
  const u32 f_actual = __shfl(st.actual, src, 64);
  if (lane == 0) {
    const bool any = key != ~0u;
    u32x4* rec = reinterpret_cast<u32x4*>(
        out + (size_t)blockIdx.x * kRecWords + wave * kRecWaveWords);
    rec[0] = u32x4{kRecMagic, xcc, hw_id, cnt[0]};
    rec[1] = u32x4{cnt[1], cnt[2], cnt[3], any ? f_test + 1u : 0u};
    rec[2] = u32x4{any ? f_index : 0u, any ? (u32)src : 0u, any ? f_reg : 0u,
                   any ? f_expected : 0u};
    rec[3] = u32x4{any ? f_actual : 0u, 0u, 0u, 0u};
  }
}

// One tile's MFMA result as one wave computes it: the numerics-testable
// surface. out[row][col], 16 x 16 fp32.
template <int FMT>
__global__ __launch_bounds__(64) void cu_check_tile_kernel(
    float* __restrict__ out, u32 seed_lo, u32 seed_hi, u32 t) {
  const int lane = threadIdx.x & 63;
  const f32x4 acc = mfma_tile<FMT>(key_base(seed_lo, seed_hi, t), lane);
  const int col = lane & 15;
  const int row0 = (lane >> 4) * 4;
#pragma unroll
  for (int r = 0; r < 4; ++r) out[(row0 + r) * 16 + col] = acc[r];
}

int parse_test(const std::string& name, int limit) {
  for (int i = 0; i < limit; ++i)
    if (name == kTestNames[i]) return i;
  TORCH_CHECK(false, "cu_check: unknown test '", name, "'");
  return -1;
}

torch::Tensor cu_check_tile(const std::string& fmt, long long tile, u64 seed) {
  const int f = parse_test(fmt, 3);
  TORCH_CHECK(tile >= 0 && tile < kMaxTile, "cu_check: tile must be in [0, ",
              kMaxTile, ")");
  auto out = torch::empty(
      {16, 16}, torch::TensorOptions().dtype(torch::kFloat32).device(torch::kCUDA));
  auto stream = at::hip::getCurrentHIPStream();
  float* p = out.data_ptr<float>();
  const SeedHalves s = split_seed(seed);
  constexpr void (*kTileKernels[3])(float*, u32, u32, u32) = {
      cu_check_tile_kernel<kBf16>, cu_check_tile_kernel<kFp8>,
      cu_check_tile_kernel<kFp4>};
  hipLaunchKernelGGL(kTileKernels[f], dim3(1), dim3(64), 0, stream.stream(), p,
                     s.lo, s.hi, (u32)tile);
  HIP_CHECK(hipGetLastError());
  return out;
}

py::dict cu_check_geometry() {
  py::dict d;
  d["threads"] = kThreads;
  d["waves"] = kWaves;
  py::dict k, fmt;
  for (int i = 0; i < 3; ++i) {
    k[kTestNames[i]] = kK[i];
    fmt[kTestNames[i]] = i;
  }
  d["k"] = k;
  d["fmt_index"] = fmt;
  py::list tests;
  for (int i = 0; i < kNumTests; ++i) tests.append(std::string(kTestNames[i]));
  d["tests"] = tests;
  d["record_words"] = kRecWords;
  d["wave_record_words"] = kRecWaveWords;
  py::dict lay;
  lay["valid"] = kRecValid;
  lay["xcc"] = kRecXcc;
  lay["hw_id"] = kRecHwId;
  lay["counts"] = kRecCounts;
  lay["first_test"] = kRecFirstTest;
  lay["first_index"] = kRecFirstIndex;
  lay["first_lane"] = kRecFirstLane;
  lay["first_reg_or_word"] = kRecFirstReg;
  lay["first_expected"] = kRecFirstExpected;
  lay["first_actual"] = kRecFirstActual;
  d["wave_record_layout"] = lay;
  d["max_rounds"] = kMaxRounds;
  d["max_grid_mult"] = kMaxGridMult;
  d["max_launches"] = kMaxLaunches;
  d["max_inject"] = kMaxInject;
  d["inject_words"] = kInjectWords;
  d["lds_phases"] = kLdsPhases;
  return d;
}

// ---------------------------------------------------------------------------
// Driver
// ---------------------------------------------------------------------------

struct Inject {
  u32 workgroup, test, index, lane_or_word, mask, sub;
};

struct DriverResult {
  int launches = 0, grid = 0, cus = 0;
  size_t lds_bytes = 0;
  double seconds = 0;
  std::vector<u32> words;  // launches * grid * kRecWords
};

inline u32 cu_key(u32 xcc, u32 hw_id) { return (xcc & 0xFu) << 8 | ((hw_id >> 8) & 0xFFu); }

DriverResult run_driver(int device, int rounds, u64 seed, int grid_mult,
                        const std::vector<Inject>& inject) {
  DriverResult out;

  DeviceScope scope(device);
  hipDeviceProp_t prop;
  HIP_CHECK(hipGetDeviceProperties(&prop, device));
  out.cus = prop.multiProcessorCount;
  out.lds_bytes = (prop.sharedMemPerBlockOptin / 16) * 16;
  TORCH_CHECK(out.lds_bytes >= 16, "cu_check: device reports no LDS");
  // grid_mult 0: a single workgroup (the smallest launch there is)
  out.grid = grid_mult == 0 ? 1 : grid_mult * out.cus;
  const u32 lds_vecs = (u32)(out.lds_bytes / 16);
  for (auto& in : inject) {
    TORCH_CHECK(in.workgroup < (u32)out.grid, "inject: workgroup ", in.workgroup,
                " is outside the grid of ", out.grid);
    if (in.test == kLds) {
      TORCH_CHECK(in.index < (u32)rounds, "inject: round ", in.index,
                  " is outside the ", rounds, " rounds");
      TORCH_CHECK(in.lane_or_word < 4 * lds_vecs, "inject: word ",
                  in.lane_or_word, " is outside the ", 4 * lds_vecs,
                  " words of LDS");
    } else {
      TORCH_CHECK(in.index < (u32)rounds * kWaves, "inject: tile ", in.index,
                  " is outside the ", rounds * kWaves, " tiles");
      TORCH_CHECK(in.lane_or_word < 64, "inject: lane ", in.lane_or_word,
                  " is outside the wave");
    }
  }

  HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(cu_check_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)out.lds_bytes));

  const size_t rec_words = (size_t)out.grid * kRecWords;
  const size_t rec_bytes = rec_words * sizeof(u32);
  DeviceBuf<u32> rec(device, rec_words);
  std::vector<u32> inj_host;
  for (auto& in : inject) {
    const u32 e[kInjectWords] = {in.workgroup, in.test, in.index,
                                 in.lane_or_word, in.mask, in.sub};
    inj_host.insert(inj_host.end(), e, e + kInjectWords);
  }
  DeviceBuf<u32> inj(device, std::max<size_t>(inj_host.size(), 4));

  Stream stream;
  Event t0, t1;
  if (!inj_host.empty())
    HIP_CHECK(hipMemcpyAsync(inj.ptr, inj_host.data(),
                             inj_host.size() * sizeof(u32),
                             hipMemcpyHostToDevice, stream.s));
  t0.record(stream);

  std::vector<u32> host(rec_words);
  std::vector<bool> seen(1u << 12, false);
  int distinct = 0;
  const SeedHalves sd = split_seed(seed);
  // On an idle GPU the first launch covers every CU; a busy one may need more.
  while (out.launches < kMaxLaunches) {
    HIP_CHECK(hipMemsetAsync(rec.ptr, 0, rec_bytes, stream.s));
    hipLaunchKernelGGL(cu_check_kernel, dim3(out.grid), dim3(kThreads),
                       out.lds_bytes, stream.s, rec.ptr, rounds, sd.lo, sd.hi,
                       lds_vecs, inj.ptr, (int)inject.size());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(host.data(), rec.ptr, rec_bytes,
                             hipMemcpyDeviceToHost, stream.s));
    stream.synchronize();
    ++out.launches;
    for (int g = 0; g < out.grid; ++g) {
      const u32* w = host.data() + (size_t)g * kRecWords;
      for (int v = 0; v < kWaves; ++v)
        TORCH_CHECK(w[v * kRecWaveWords + kRecValid] == kRecMagic,
                    "cu_check: workgroup ", g, " wave ", v, " left no record");
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

py::dict cu_check(int device, int rounds, u64 seed, int grid_mult,
                  std::vector<std::vector<long long>> inject) {
  check_device(device);
  TORCH_CHECK(rounds >= 1 && rounds <= kMaxRounds, "rounds must be in [1, ",
              kMaxRounds, "]");
  TORCH_CHECK(grid_mult >= 0 && grid_mult <= kMaxGridMult,
              "grid_mult must be in [0, ", kMaxGridMult, "]");
  TORCH_CHECK((int)inject.size() <= kMaxInject, "at most ", kMaxInject,
              " inject entries");
  std::vector<Inject> inj;
  for (auto& e : inject) {
    TORCH_CHECK(e.size() == kInjectWords - 1 || e.size() == kInjectWords,
                "inject: entries are (workgroup, test, tile_or_round, "
                "lane_or_word, xor_mask[, sub])");
    for (long long x : e)
      TORCH_CHECK(x >= 0 && x <= 0xFFFFFFFFll, "inject: ", x,
                  " is not an unsigned 32-bit value");
    TORCH_CHECK(e[1] < kNumTests, "inject: test ", e[1], " is not one of 0..3");
    const long long sub = e.size() == kInjectWords ? e[5] : 0;
    if (e[1] == kLds) {
      TORCH_CHECK(sub < kLdsPhases, "inject: phase ", sub, " is not 0 or 1");
    } else {
      TORCH_CHECK(sub < 4, "inject: register ", sub, " is not one of 0..3");
    }
    inj.push_back({(u32)e[0], (u32)e[1], (u32)e[2], (u32)e[3], (u32)e[4],
                   (u32)sub});
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
    py::list hw;
    py::dict counts;
    u32 sum[kNumTests] = {0, 0, 0, 0};
    const u32* first = nullptr;
    for (int v = 0; v < kWaves; ++v) {
      const u32* ww = w + v * kRecWaveWords;
      hw.append(ww[kRecHwId]);
      for (int c = 0; c < kNumTests; ++c) sum[c] += ww[kRecCounts + c];
      if (first == nullptr && ww[kRecFirstTest] != 0) first = ww;
    }
    d["hw_id"] = hw;
    for (int c = 0; c < kNumTests; ++c) counts[kTestNames[c]] = sum[c];
    d["counts"] = counts;
    if (first != nullptr && first[kRecFirstTest] <= kNumTests) {
      py::dict f;
      const bool lds = first[kRecFirstTest] - 1 == kLds;
      f["test"] = std::string(kTestNames[first[kRecFirstTest] - 1]);
      f[lds ? "round" : "tile"] = first[kRecFirstIndex];
      f["wave"] = (int)((first - w) / kRecWaveWords);
      f["lane"] = first[kRecFirstLane];
      f[lds ? "word" : "reg"] = first[kRecFirstReg];
      f["expected"] = first[kRecFirstExpected];
      f["actual"] = first[kRecFirstActual];
      d["first"] = f;
    } else {
      d["first"] = py::none();
    }
    recs.append(d);
  }
  py::dict d;
  d["records"] = recs;
  d["launches"] = r.launches;
  d["grid"] = r.grid;
  d["rounds"] = rounds;
  d["lds_bytes"] = py::int_(r.lds_bytes);
  d["seconds"] = r.seconds;
  return d;
}

}  // namespace cu_check
