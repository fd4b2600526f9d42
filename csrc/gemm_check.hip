// Checked GEMM loop for the GPU burn-in (MI355X / gfx950).
//
// The throughput tiers of /gpus/validate drive the whole datapath (HBM ->
// LDS-DMA -> swizzled LDS reads -> MFMA -> epilogue stores on every CU at
// once) and never look at a result. This file runs the same 256^2 kernels back
// to back at full size on operands whose sums are exact in fp32, and after
// every launch verifies C on the device with integer row and column checksums
// per 256x256 tile (algorithm-based fault tolerance). A wrong accumulator
// shows as one row and one column of one tile, named with the workgroup that
// computed it.
//
// Generator. With a u64 seed (seed_lo, seed_hi its halves), format index fmt
// (0 bf16, 1 MX-fp8 e4m3, 2 MX-fp4 e2m1), operand (0 = A, 1 = Bt), row and k:
//
//   fmix32(h): h^=h>>16; h*=0x85EBCA6B; h^=h>>13; h*=0xC2B2AE35; h^=h>>16
//
//   u = fmix32(fmix32(seed_lo + row*0x9E3779B9) ^ seed_hi
//              ^ (fmt<<28 | operand<<24 | k))                   (k < 2^24)
//
//   bf16, range r (1..127):  m = (u % (2r+1)) - r, value m/16
//   e4m3, range w (1..4):    j = u % (16w+1); code 0x00 for j = 0, otherwise
//          with q = j-1, s = q / 8w, t = q % 8w:
//          code = s<<7 | (6 + (t>>3))<<3 | (t&7)
//          (zero and every code with exponent field 6..6+w-1: multiples of
//          2^-4 up to 15 * 2^(w-1) of them)
//   e2m1, range 16:          code = u & 15 (multiples of 1/2 up to 6)
//
// An element depends on (seed, fmt, operand, row, k) and on the range, never
// on the extents. The range shrinks with K (hipcore.gemm_check_range) so that
// max_a * max_b * K / (granule_a * granule_b) <= 2^24: every partial sum is
// then an integer number of product granules (2^-8 for bf16 and e4m3, 2^-2
// for e2m1) below 2^24, exact in fp32 whatever the order of summation. The
// host re-evaluates the condition and rejects a range that violates it.
// Layouts are the GEMM bindings': bf16 [rows][K], e4m3 bytes [rows][K], e2m1
// bytes [rows][K/2] with the low nibble the even k.
//
// Expected checksums, from the generator and never from memory, in product
// granules. With a, b the operands' integer numerators, for every tile (I, J):
//
//   R[I][J][r] = sum_k a[256I+r][k] * SB[J][k],  SB[J][k] = sum_{j in J} b[j][k]
//   Q[I][J][c] = sum_k SA[I][k] * b[256J+c][k],  SA[I][k] = sum_{i in I} a[i][k]
//
// int64 [M/256][N/256][256] each. tile_sum_kernel makes SA and SB (M*K + N*K
// hash evaluations, twice: once per operand row base), row_dot_kernel the dot
// products (one wave per operand row, eight tiles per pass over k, so the
// row's hashes are evaluated ceil(tiles/8) times).
//
// Verify (the per-iteration hot path). One workgroup of 256 threads takes a
// strip of 64 rows of one tile: wave w the rows 16w..16w+15, one 16-byte load
// per lane per row (64 lanes x float4 = one 256-float tile row), all 16 loads
// issued before the first use. The loads are non-temporal: C is read once,
// and at 8192^2 letting it through the 256 MiB Infinity Cache evicted the
// operands the next GEMM reads, which cost that GEMM 33-41 us
// (profiles/gemm_check.md). Per element: scale by the inverse granule
// (exact), count it as malformed unless |x| <= 2^24 and x is an integer (NaN,
// Inf, a never-written poison word, anything that is no possible sum; it then
// contributes 0), otherwise convert to int. A row sum is a wave reduction
// (int32 within 16 lanes: 64 x 2^24 = 2^30; int64 across the four groups) and
// is compared with R on the spot. Column sums run down the rows in each
// lane's registers (16 x 2^24 fits int32), the four waves are added through
// 4 KiB of LDS (64 x 2^24 = 2^30) and the strip's 256 partial sums go to a
// slab [tile][strip][256]; col_check_kernel adds a tile's four strips in
// int64 and compares with Q. Integers only, equality only, no tolerance. The
// slab is written in full by every verify, so nothing is cleared between
// iterations and the result is reproducible bit for bit.
//
// Report, device-resident u64 words: [0] row mismatches, [1] column
// mismatches, [2] malformed elements, [3] record slots claimed, [4] operand
// elements that differ from the generator, then up to cap records of
// kRecWords words, claimed with burnin_core.h's claim_record. Counts are never
// capped.
//
// No spin-waits, nothing shared between workgroups but the counters; every
// kernel ends by itself whatever it finds.
//
// fmix32, the generator's elem_code / elem_int and the exactness condition
// are in burnin_core.h, where burnin_selftest.cpp runs them on the CPU.
//
// Included by hipcore.hip after its 256^2 variant tables (needs the torch
// headers, hipcore.hip's using-declarations of hip_host.h's resource owners,
// mfma_warmup, find_variant and launch_256).
#include "burnin_core.h"
#include "burnin_host.h"

namespace gemm_check {

using namespace burnin;

// A kind is one of burnin_core.h's formats.
constexpr int kMinK[kNumFormats] = {192, 256, 512};      // the GEMM bindings'
constexpr int kKMult[kNumFormats] = {64, 128, 256};
constexpr int kDefaultCode[kNumFormats] = {0, 16, 16};   // what validate_gpus times

constexpr int kTile = 256;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kWaveRows = 16;                 // loads in flight per lane
constexpr int kStripRows = kWaves * kWaveRows;
constexpr int kStrips = kTile / kStripRows;
constexpr int kDotTiles = 8;                  // tiles per pass of row_dot_kernel

constexpr int kRepRows = 0, kRepCols = 1, kRepMalformed = 2, kRepClaimed = 3,
              kRepOperand = 4, kRepHeader = 8;
// A record: {type | iter << 8, tile_row << 32 | tile_col, index, got, want}.
// index: the row or column in the tile; malformed: row << 8 | col, got the
// fp32 bits.
constexpr int kRecWords = 5;
enum RecType { kRecRow = 0, kRecCol = 1, kRecMalformed = 2 };
const char* const kRecTypeNames[3] = {"row", "col", "malformed"};
constexpr int kMaxInject = 64;
constexpr int kMaxIters = 100000;
constexpr int kMaxExtent = 1 << 16;
constexpr u32 kPoisonBits = 0x7FC0DEADu;  // a quiet NaN

enum Loop {
  kOverlap = 0, kSerial = 1, kUnchecked = 2, kVerifyOnly = 3, kVerifyCold = 4,
  kSerialAtomic = 5, kVerifyAtomic = 6, kNumLoops = 7
};
const char* const kLoopNames[kNumLoops] = {"overlap", "serial", "unchecked", "verify",
                                           "verify-cold", "serial-atomic",
                                           "verify-atomic"};
// kVerifyCold cycles over this many bytes of results, three times the 256 MiB
// Infinity Cache, so that every read comes from HBM.
constexpr size_t kColdBytes = 768ull << 20;
// Measured (profiles/gemm_check.md): the 256^2 kernels fill every CU, so the
// second stream buys no overlap and its event hand-offs cost more than they
// hide; the serial loop is what ships.
constexpr int kDefaultLoop = kSerial;

// ---------------------------------------------------------------------------
// Generator
// ---------------------------------------------------------------------------

template <int KIND>
__device__ __forceinline__ u32 draw(u32 base, u32 operand, u32 k) {
  return fmix32(base ^ ((u32)KIND << 28 | operand << 24 | k));
}

// Operand fill, or with CHECK the comparison of a stored operand with the
// generator. One 16-byte vector per thread and step: 8 bf16, 16 e4m3 or 32
// e2m1 elements of one row.
template <int KIND, bool CHECK>
__global__ __launch_bounds__(kThreads) void operand_kernel(
    u32x4* __restrict__ p, u64 nvec, u32 vecs_per_row, u32 operand, u32 seed_lo,
    u32 seed_hi, u32 range, u64* __restrict__ rep) {
  constexpr u32 kBits = kElemBits[KIND];
  constexpr u32 kPerWord = 32 / kBits;
  constexpr u32 kMask = (u32)((1ull << kBits) - 1);
  u32 bad = 0;
  const u64 stride = (u64)gridDim.x * kThreads;
  for (u64 v = (u64)blockIdx.x * kThreads + threadIdx.x; v < nvec; v += stride) {
    const u32 row = (u32)(v / vecs_per_row);
    const u32 k0 = (u32)(v % vecs_per_row) * 4u * kPerWord;
    const u32 base = key_base(seed_lo, seed_hi, row);
    u32x4 e;
#pragma unroll
    for (u32 w = 0; w < 4; ++w) {
      u32 word = 0;
#pragma unroll
      for (u32 j = 0; j < kPerWord; ++j)
        word |= elem_code<KIND>(draw<KIND>(base, operand, k0 + w * kPerWord + j), range)
                << (kBits * j);
      e[w] = word;
    }
    if (!CHECK) {
      p[v] = e;
    } else {
      const u32x4 got = p[v];
#pragma unroll
      for (u32 w = 0; w < 4; ++w) {
        const u32 d = got[w] ^ e[w];
        if (d != 0) {
#pragma unroll
          for (u32 j = 0; j < kPerWord; ++j) bad += ((d >> (kBits * j)) & kMask) != 0;
        }
      }
    }
  }
  if (CHECK) {
    wave_sum(bad);
    if ((threadIdx.x & 63) == 0 && bad != 0) atomicAdd(&rep[kRepOperand], (u64)bad);
  }
}

// ---------------------------------------------------------------------------
// Expected checksums
// ---------------------------------------------------------------------------

// S[t][k] = sum over the 256 rows of tile t of the operand's numerators.
template <int KIND>
__global__ __launch_bounds__(kThreads) void tile_sum_kernel(
    int* __restrict__ S, u32 tiles, u32 K, u32 operand, u32 seed_lo, u32 seed_hi,
    u32 range) {
  const u64 idx = (u64)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= (u64)tiles * K) return;
  const u32 t = (u32)(idx / K), k = (u32)(idx % K);
  int s = 0;
  for (u32 r = 0; r < (u32)kTile; ++r)
    s += elem_int<KIND>(
        draw<KIND>(key_base(seed_lo, seed_hi, t * kTile + r), operand, k), range);
  S[idx] = s;
}

// out[(row/256)*stride_own + t*stride_other + row%256] = sum_k x[row][k] *
// S[t][k] for every tile t of the other operand; one wave per row.
template <int KIND>
__global__ __launch_bounds__(kThreads) void row_dot_kernel(
    i64* __restrict__ out, const int* __restrict__ S, u32 rows, u32 tiles, u32 K,
    u32 operand, u32 seed_lo, u32 seed_hi, u32 range, u32 stride_own,
    u32 stride_other) {
  const u32 lane = threadIdx.x & 63;
  const u32 row = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (row >= rows) return;  // wave-uniform
  const u32 base = key_base(seed_lo, seed_hi, row);
  for (u32 t0 = 0; t0 < tiles; t0 += kDotTiles) {
    i64 acc[kDotTiles];
#pragma unroll
    for (int j = 0; j < kDotTiles; ++j) acc[j] = 0;
    for (u32 k = lane; k < K; k += 64) {
      const i64 x = elem_int<KIND>(draw<KIND>(base, operand, k), range);
#pragma unroll
      for (int j = 0; j < kDotTiles; ++j)
        if (t0 + j < tiles) acc[j] += x * S[(size_t)(t0 + j) * K + k];
    }
#pragma unroll
    for (int j = 0; j < kDotTiles; ++j) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) acc[j] += __shfl_xor(acc[j], off, 64);
      if (lane == 0 && t0 + j < tiles)
        out[(size_t)(row / kTile) * stride_own + (size_t)(t0 + j) * stride_other +
            row % kTile] = acc[j];
    }
  }
}

// ---------------------------------------------------------------------------
// Verify
// ---------------------------------------------------------------------------

// Mismatch slow path: one claimed record per finding while slots are left.
__device__ __noinline__ void record(u64* rep, u64 cap, u64 type, u64 iter,
                                    u64 tile_row, u64 tile_col, u64 index,
                                    u64 got, u64 want) {
  u64* r;
  if (!claim_record<kRepClaimed, kRepHeader, kRecWords>(rep, cap, r)) return;
  r[0] = type | iter << 8;
  r[1] = tile_row << 32 | tile_col;
  r[2] = index;
  r[3] = got;
  r[4] = want;
}

// grid = tiles * kStrips workgroups; C is [M][ldc] fp32 with M and ldc
// multiples of 256, so every load below is inside C. ATOMIC: the strip's
// column sums are added to acc [tile][256] (cleared by the host before the
// launch) with 64-bit atomics instead of being stored to the slab; integer
// sums, so the result is the same bit for bit. Measured slower, kept for the
// comparison (profiles/gemm_check.md).
template <bool ATOMIC>
__global__ __launch_bounds__(kThreads) void verify_kernel(
    const float* __restrict__ C, u32 ldc, u32 tiles_n, const i64* __restrict__ R,
    int* __restrict__ slab, u64* __restrict__ acc, u64* __restrict__ rep, u64 cap,
    u32 iter, float inv_granule) {
  __shared__ int part[kWaves][kTile];
  const u32 tile = blockIdx.x / kStrips, strip = blockIdx.x % kStrips;
  const u32 ti = tile / tiles_n, tj = tile % tiles_n;
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u32 r0 = strip * kStripRows + wave * kWaveRows;  // in the tile

  const f32x4* src =
      reinterpret_cast<const f32x4*>(C + (size_t)(ti * kTile + r0) * ldc +
                                     (size_t)tj * kTile) + lane;
  const size_t row_vecs = ldc / 4;
  f32x4 v[kWaveRows];
#pragma unroll
  for (int j = 0; j < kWaveRows; ++j) v[j] = __builtin_nontemporal_load(src + j * row_vecs);

  int col[4] = {0, 0, 0, 0};
  i64 mine = 0;  // lane j < 16: the sum of row r0 + j
  u32 bad = 0;
#pragma unroll
  for (int j = 0; j < kWaveRows; ++j) {
    int s = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float f = v[j][e];
      const float y = f * inv_granule;
      int x = 0;
      if (fabsf(y) <= 16777216.f && y == truncf(y)) {  // false for NaN
        x = (int)y;
      } else {
        ++bad;
        record(rep, cap, kRecMalformed, iter, ti, tj,
               (u64)(r0 + j) << 8 | (4 * lane + e), __float_as_uint(f), 0);
      }
      col[e] += x;
      s += x;
    }
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) s += __shfl_xor(s, off, 64);
    const i64 row = (i64)s + __shfl_xor(s, 16, 64) + __shfl_xor(s, 32, 64) +
                    __shfl_xor(s, 48, 64);
    if ((int)lane == j) mine = row;
  }
  if (lane < (u32)kWaveRows) {
    const i64 want = R[(size_t)tile * kTile + r0 + lane];
    if (mine != want) {
      atomicAdd(&rep[kRepRows], 1ull);
      record(rep, cap, kRecRow, iter, ti, tj, r0 + lane, (u64)mine, (u64)want);
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) part[wave][4 * lane + e] = col[e];
  __syncthreads();
  int sum = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) sum += part[w][threadIdx.x];
  if (ATOMIC)
    atomicAdd(&acc[(size_t)tile * kTile + threadIdx.x], (u64)(i64)sum);
  else
    slab[((size_t)tile * kStrips + strip) * kTile + threadIdx.x] = sum;

  wave_sum(bad);
  if (lane == 0 && bad != 0) atomicAdd(&rep[kRepMalformed], (u64)bad);
}

// One thread per tile column: the four strips added (ATOMIC: the accumulated
// sum read), compared with Q.
template <bool ATOMIC>
__global__ __launch_bounds__(kThreads) void col_check_kernel(
    const int* __restrict__ slab, const u64* __restrict__ acc,
    const i64* __restrict__ Q, u32 tiles, u32 tiles_n, u64* __restrict__ rep,
    u64 cap, u32 iter) {
  const u32 tile = blockIdx.x, c = threadIdx.x;
  if (tile >= tiles) return;
  i64 got = 0;
  if (ATOMIC) {
    got = (i64)acc[(size_t)tile * kTile + c];
  } else {
#pragma unroll
    for (int s = 0; s < kStrips; ++s)
      got += slab[((size_t)tile * kStrips + s) * kTile + c];
  }
  const i64 want = Q[(size_t)tile * kTile + c];
  if (got != want) {
    atomicAdd(&rep[kRepCols], 1ull);
    record(rep, cap, kRecCol, iter, tile / tiles_n, tile % tiles_n, c, (u64)got,
           (u64)want);
  }
}

// Detector self-test: flips bits of one element of C. The host has checked
// that the element is inside C.
__global__ void inject_kernel(float* C, size_t element, u32 mask) {
  u32* p = reinterpret_cast<u32*>(C) + element;
  *p ^= mask;
}

// ---------------------------------------------------------------------------
// Host: argument checks and the launches the bindings and the driver share
// ---------------------------------------------------------------------------

int parse_kind(const std::string& name) {
  for (int i = 0; i < kNumFormats; ++i)
    if (name == kFormatNames[i]) return i;
  TORCH_CHECK(false, "gemm_check: unknown kind '", name, "' (bf16, fp8, fp4)");
  return -1;
}

// The exactness condition, re-evaluated: largest numerator squared times K
// must not exceed 2^24.
void check_range(int kind, i64 K, i64 range) {
  TORCH_CHECK(K >= 1 && K <= kTwo24, "gemm_check: K must be in [1, 2^24]");
  const bool legal = range >= kMinRange[kind] && range <= kFullRange[kind];
  if (kind == kBf16) {
    TORCH_CHECK(legal, "gemm_check: bf16 range must be in [1, 127]");
  } else if (kind == kFp8) {
    TORCH_CHECK(legal, "gemm_check: fp8 range must be in [1, 4]");
  } else {
    TORCH_CHECK(legal, "gemm_check: fp4 range must be 16");
  }
  TORCH_CHECK(sums_exact(kind, range, K), "gemm_check: range ", range, " of ",
              kFormatNames[kind], " is not exact at K = ", K, ": ",
              max_numerator(kind, range), "^2 * K > 2^24");
}

void check_extent(i64 v, const char* name) {
  TORCH_CHECK(v >= kTile && v % kTile == 0 && v <= kMaxExtent, "gemm_check: ", name,
              " must be a multiple of 256 in [256, ", kMaxExtent, "]");
}

// K as the kind's GEMM binding takes it.
void check_k(int kind, i64 K) {
  TORCH_CHECK(K >= kMinK[kind] && K % kKMult[kind] == 0, "gemm_check: K of ",
              kFormatNames[kind], " must be a multiple of ", kKMult[kind], ", >= ",
              kMinK[kind]);
}

size_t operand_bytes(int kind, size_t rows, size_t K) {
  return rows * K * kElemBits[kind] / 8;
}

using OperandKernel = void (*)(u32x4*, u64, u32, u32, u32, u32, u32, u64*);
constexpr OperandKernel kOperandKernels[kNumFormats][2] = {
    {operand_kernel<kBf16, false>, operand_kernel<kBf16, true>},
    {operand_kernel<kFp8, false>, operand_kernel<kFp8, true>},
    {operand_kernel<kFp4, false>, operand_kernel<kFp4, true>},
};
using TileSumKernel = void (*)(int*, u32, u32, u32, u32, u32, u32);
constexpr TileSumKernel kTileSumKernels[kNumFormats] = {
    tile_sum_kernel<kBf16>, tile_sum_kernel<kFp8>, tile_sum_kernel<kFp4>};
using RowDotKernel = void (*)(i64*, const int*, u32, u32, u32, u32, u32, u32, u32,
                              u32, u32);
constexpr RowDotKernel kRowDotKernels[kNumFormats] = {
    row_dot_kernel<kBf16>, row_dot_kernel<kFp8>, row_dot_kernel<kFp4>};

// Fill (check = false) or compare with the generator (check = true, counted
// in rep[kRepOperand]) one operand of `rows` x K elements at p.
void launch_operand(int kind, bool check, void* p, u32 rows, u32 K, u32 operand,
                    u64 seed, u32 range, u64* rep, hipStream_t s) {
  const u32 vecs_per_row = K * kElemBits[kind] / 128;
  const u64 nvec = (u64)rows * vecs_per_row;
  const unsigned grid = (unsigned)std::min<u64>((nvec + kThreads - 1) / kThreads, 4096);
  const SeedHalves sd = split_seed(seed);
  hipLaunchKernelGGL(kOperandKernels[kind][check ? 1 : 0], dim3(grid),
                     dim3(kThreads), 0, s, static_cast<u32x4*>(p), nvec,
                     vecs_per_row, operand, sd.lo, sd.hi, range, rep);
  HIP_CHECK(hipGetLastError());
}

// R and Q of an M x N x K problem; SA [M/256][K] and SB [N/256][K] are scratch.
void launch_expected(int kind, u32 M, u32 N, u32 K, u64 seed, u32 range, int* SA,
                     int* SB, i64* R, i64* Q, hipStream_t s) {
  const u32 tm = M / kTile, tn = N / kTile;
  const SeedHalves sd = split_seed(seed);
  auto blocks = [](u64 n) { return dim3((unsigned)((n + kThreads - 1) / kThreads)); };
  hipLaunchKernelGGL(kTileSumKernels[kind], blocks((u64)tm * K), dim3(kThreads), 0,
                     s, SA, tm, K, 0u, sd.lo, sd.hi, range);
  hipLaunchKernelGGL(kTileSumKernels[kind], blocks((u64)tn * K), dim3(kThreads), 0,
                     s, SB, tn, K, 1u, sd.lo, sd.hi, range);
  hipLaunchKernelGGL(kRowDotKernels[kind], dim3(M / kWaves), dim3(kThreads), 0, s, R,
                     SB, M, tn, K, 0u, sd.lo, sd.hi, range, tn * kTile, (u32)kTile);
  hipLaunchKernelGGL(kRowDotKernels[kind], dim3(N / kWaves), dim3(kThreads), 0, s, Q,
                     SA, N, tm, K, 1u, sd.lo, sd.hi, range, (u32)kTile, tn * kTile);
  HIP_CHECK(hipGetLastError());
}

// One verification of C [M][N] against R and Q; slab holds tiles * kStrips *
// 256 ints. With acc (tiles * 256 u64) the column sums are combined with
// atomics instead.
void launch_verify(int kind, const float* C, u32 M, u32 N, const i64* R,
                   const i64* Q, int* slab, u64* rep, u64 cap, u32 iter,
                   hipStream_t s, u64* acc = nullptr) {
  const u32 tn = N / kTile, tiles = (M / kTile) * tn;
  const dim3 grid(tiles * kStrips), block(kThreads);
  if (acc != nullptr) {
    HIP_CHECK(hipMemsetAsync(acc, 0, (size_t)tiles * kTile * sizeof(u64), s));
    hipLaunchKernelGGL(verify_kernel<true>, grid, block, 0, s, C, N, tn, R, slab, acc,
                       rep, cap, iter, kInvGranule[kind]);
    hipLaunchKernelGGL(col_check_kernel<true>, dim3(tiles), block, 0, s, slab, acc, Q,
                       tiles, tn, rep, cap, iter);
  } else {
    hipLaunchKernelGGL(verify_kernel<false>, grid, block, 0, s, C, N, tn, R, slab, acc,
                       rep, cap, iter, kInvGranule[kind]);
    hipLaunchKernelGGL(col_check_kernel<false>, dim3(tiles), block, 0, s, slab, acc,
                       Q, tiles, tn, rep, cap, iter);
  }
  HIP_CHECK(hipGetLastError());
}

size_t rep_words(u64 cap) { return kRepHeader + kRecWords * cap; }

py::dict report_dict(const u64* h, u64 cap) {
  py::dict d, errors;
  errors["rows"] = py::int_(h[kRepRows]);
  errors["cols"] = py::int_(h[kRepCols]);
  errors["malformed"] = py::int_(h[kRepMalformed]);
  d["errors"] = errors;
  py::list recs;
  const u64 nrec = std::min<u64>(h[kRepClaimed], cap);
  for (u64 i = 0; i < nrec; ++i) {
    const u64* r = h + kRepHeader + kRecWords * i;
    const u64 type = r[0] & 0xFF;
    if (type > kRecMalformed) continue;
    py::dict e;
    e["type"] = std::string(kRecTypeNames[type]);
    e["iter"] = py::int_(r[0] >> 8);
    e["tile_row"] = py::int_(r[1] >> 32);
    e["tile_col"] = py::int_(r[1] & 0xFFFFFFFFull);
    if (type == kRecMalformed) {
      e["row"] = py::int_(r[2] >> 8);
      e["col"] = py::int_(r[2] & 0xFF);
      e["bits"] = py::int_(r[3]);
    } else {
      e["index"] = py::int_(r[2]);
      e["got"] = py::int_((i64)r[3]);
      e["want"] = py::int_((i64)r[4]);
    }
    recs.append(e);
  }
  d["records"] = recs;
  return d;
}

// ---------------------------------------------------------------------------
// Tensor bindings: each stage alone, on torch's current device and stream
// ---------------------------------------------------------------------------

torch::Tensor gemm_check_fill(const std::string& kind_name, int operand, i64 rows,
                              i64 K, u64 seed, i64 range) {
  const int kind = parse_kind(kind_name);
  TORCH_CHECK(operand == 0 || operand == 1, "gemm_check: operand is 0 (A) or 1 (Bt)");
  TORCH_CHECK(rows >= 1 && rows <= kMaxExtent, "gemm_check: rows must be in [1, ",
              kMaxExtent, "]");
  check_range(kind, K, range);
  TORCH_CHECK(K * kElemBits[kind] % 128 == 0,
              "gemm_check: a row must be a multiple of 16 bytes");
  auto opts = torch::TensorOptions().device(torch::kCUDA);
  torch::Tensor t =
      kind == kBf16 ? torch::empty({rows, K}, opts.dtype(torch::kBFloat16))
                    : torch::empty({rows, kind == kFp4 ? K / 2 : K},
                                   opts.dtype(torch::kUInt8));
  launch_operand(kind, false, t.data_ptr(), (u32)rows, (u32)K, (u32)operand, seed,
                 (u32)range, nullptr, at::hip::getCurrentHIPStream().stream());
  return t;
}

std::pair<torch::Tensor, torch::Tensor> expected_tensors(int kind, i64 M, i64 N,
                                                         i64 K, u64 seed,
                                                         i64 range) {
  check_extent(M, "M");
  check_extent(N, "N");
  check_range(kind, K, range);
  auto opts = torch::TensorOptions().device(torch::kCUDA);
  const i64 tm = M / kTile, tn = N / kTile;
  auto SA = torch::empty({tm, K}, opts.dtype(torch::kInt32));
  auto SB = torch::empty({tn, K}, opts.dtype(torch::kInt32));
  auto R = torch::empty({tm, tn, kTile}, opts.dtype(torch::kInt64));
  auto Q = torch::empty({tm, tn, kTile}, opts.dtype(torch::kInt64));
  launch_expected(kind, (u32)M, (u32)N, (u32)K, seed, (u32)range,
                  SA.data_ptr<int>(), SB.data_ptr<int>(),
                  reinterpret_cast<i64*>(R.data_ptr<int64_t>()),
                  reinterpret_cast<i64*>(Q.data_ptr<int64_t>()),
                  at::hip::getCurrentHIPStream().stream());
  return {R, Q};
}

std::pair<torch::Tensor, torch::Tensor> gemm_check_expected(
    const std::string& kind_name, i64 M, i64 N, i64 K, u64 seed, i64 range) {
  return expected_tensors(parse_kind(kind_name), M, N, K, seed, range);
}

// The operand check of the driver's read-back on a stored operand: the number
// of elements of t that differ from the generator's. For the tests; every
// argument is checked before the launch.
u64 gemm_check_operand(const std::string& kind_name, int operand, torch::Tensor t,
                       i64 K, u64 seed, i64 range) {
  const int kind = parse_kind(kind_name);
  TORCH_CHECK(operand == 0 || operand == 1, "gemm_check: operand is 0 (A) or 1 (Bt)");
  check_range(kind, K, range);
  TORCH_CHECK(K * kElemBits[kind] % 128 == 0,
              "gemm_check: a row must be a multiple of 16 bytes");
  TORCH_CHECK(t.is_cuda() && t.dim() == 2 && t.is_contiguous() &&
                  t.scalar_type() == (kind == kBf16 ? torch::kBFloat16 : torch::kUInt8),
              "gemm_check: the operand must be a contiguous 2-D GPU tensor, bfloat16 "
              "for bf16 and uint8 for fp8 and fp4");
  const i64 rows = t.size(0);
  TORCH_CHECK(rows >= 1 && rows <= kMaxExtent, "gemm_check: rows must be in [1, ",
              kMaxExtent, "]");
  TORCH_CHECK(t.size(1) == (kind == kFp4 ? K / 2 : K), "gemm_check: the operand must be "
              "[rows][K] (fp4: [rows][K/2]) but a row has ", t.size(1), " entries");
  int cur = -1;
  HIP_CHECK(hipGetDevice(&cur));
  TORCH_CHECK(t.get_device() == cur, "gemm_check: the operand is on device ",
              t.get_device(), " but the current device is ", cur);
  TORCH_CHECK((reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0,
              "gemm_check: the operand must be 16-byte aligned");
  auto rep = torch::zeros({(int64_t)kRepHeader},
                          torch::TensorOptions().device(torch::kCUDA).dtype(torch::kInt64));
  launch_operand(kind, true, t.data_ptr(), (u32)rows, (u32)K, (u32)operand, seed,
                 (u32)range, reinterpret_cast<u64*>(rep.data_ptr<int64_t>()),
                 at::hip::getCurrentHIPStream().stream());
  auto host = rep.cpu();  // synchronises with the current stream
  return reinterpret_cast<const u64*>(host.data_ptr<int64_t>())[kRepOperand];
}

// atomic: the column sums are combined in a tiles * 256 u64 accumulator, as
// the serial-atomic and verify-atomic loops of the driver do.
py::dict gemm_check_verify(const std::string& kind_name, torch::Tensor C, i64 K,
                           u64 seed, i64 range, i64 max_records, bool atomic) {
  const int kind = parse_kind(kind_name);
  TORCH_CHECK(C.is_cuda() && C.scalar_type() == torch::kFloat32 && C.dim() == 2 &&
                  C.is_contiguous(),
              "gemm_check: C must be a contiguous 2-D float32 GPU tensor");
  int cur = -1;
  HIP_CHECK(hipGetDevice(&cur));
  TORCH_CHECK(C.get_device() == cur, "gemm_check: C is on device ", C.get_device(),
              " but the current device is ", cur);
  TORCH_CHECK((reinterpret_cast<uintptr_t>(C.data_ptr()) & 15) == 0,
              "gemm_check: C must be 16-byte aligned");
  const u64 cap = check_max_records(max_records);
  const i64 M = C.size(0), N = C.size(1);
  auto rq = expected_tensors(kind, M, N, K, seed, range);
  auto opts = torch::TensorOptions().device(torch::kCUDA);
  auto slab = torch::empty({(M / kTile) * (N / kTile) * kStrips * kTile},
                           opts.dtype(torch::kInt32));
  auto rep = torch::zeros({(int64_t)rep_words(cap)}, opts.dtype(torch::kInt64));
  torch::Tensor acc;
  if (atomic)
    acc = torch::empty({(M / kTile) * (N / kTile) * kTile}, opts.dtype(torch::kInt64));
  launch_verify(kind, C.data_ptr<float>(), (u32)M, (u32)N,
                reinterpret_cast<const i64*>(rq.first.data_ptr<int64_t>()),
                reinterpret_cast<const i64*>(rq.second.data_ptr<int64_t>()),
                slab.data_ptr<int>(), reinterpret_cast<u64*>(rep.data_ptr<int64_t>()),
                cap, 0, at::hip::getCurrentHIPStream().stream(),
                atomic ? reinterpret_cast<u64*>(acc.data_ptr<int64_t>()) : nullptr);
  auto host = rep.cpu();  // synchronises with the current stream
  return report_dict(reinterpret_cast<const u64*>(host.data_ptr<int64_t>()), cap);
}

py::dict gemm_check_geometry() {
  py::dict d, index, min_k, code, inv;
  py::list kinds, loops;
  for (int i = 0; i < kNumFormats; ++i) {
    kinds.append(std::string(kFormatNames[i]));
    index[kFormatNames[i]] = i;
    min_k[kFormatNames[i]] = kMinK[i];
    code[kFormatNames[i]] = kDefaultCode[i];
    inv[kFormatNames[i]] = (int)kInvGranule[i];
  }
  for (int i = 0; i < kNumLoops; ++i) loops.append(std::string(kLoopNames[i]));
  d["kinds"] = kinds;
  d["kind_index"] = index;
  d["min_k"] = min_k;
  d["default_code"] = code;
  d["inverse_granule"] = inv;
  d["loops"] = loops;
  d["default_loop"] = std::string(kLoopNames[kDefaultLoop]);
  d["tile"] = kTile;
  d["threads"] = kThreads;
  d["strip_rows"] = kStripRows;
  d["strips"] = kStrips;
  d["record_words"] = kRecWords;
  d["max_records"] = py::int_(kMaxRecordsLimit);
  d["max_inject"] = kMaxInject;
  d["max_iters"] = kMaxIters;
  d["poison_bits"] = kPoisonBits;
  return d;
}

// ---------------------------------------------------------------------------
// Driver
// ---------------------------------------------------------------------------

struct Inject {
  u32 iter, row, col, mask;
};

struct DriverResult {
  double seconds = 0;
  std::vector<u64> rep;
};

// Enqueues one size^3 GEMM into C on a stream.
using GemmFn = std::function<void(hipStream_t, float*)>;

// Warm-up, fill, expected sums, then `iters` x (GEMM, verify) in the order
// `loop` names, then the operand read-back. kSerial (the default): one
// stream, one C. kOverlap: C is double-buffered and verify runs on a second
// stream; verify i waits for GEMM i, GEMM i+2 for verify i. kUnchecked (GEMMs
// only), kVerifyOnly (one GEMM, then `iters` verifies of it, which the cache
// may serve) and kVerifyCold (verifies cycling over kColdBytes of results, so
// that they come from HBM) exist to time the parts, kSerialAtomic and
// kVerifyAtomic to time the atomic combining of the column sums
// (scripts/gemm_check_ab.py).
DriverResult run_driver(int device, int kind, int size, int iters, u64 seed,
                        u32 range, u64 cap, const std::vector<Inject>& inject,
                        int loop, const std::function<GemmFn(const void*, const void*)>& bind) {
  DriverResult out;
  DeviceScope scope(device);
  mfma_warmup(device, 20000);

  const size_t op_bytes = operand_bytes(kind, size, size);
  const size_t c_elems = (size_t)size * size;
  const u32 tiles = (u32)(size / kTile), n = (u32)size;
  DeviceBuf<unsigned char> A(device, op_bytes), Bt(device, op_bytes);
  std::vector<DeviceBuf<float>> C;
  const size_t c_bytes = c_elems * sizeof(float);
  const int nbuf = loop == kOverlap      ? 2
                   : loop == kVerifyCold ? (int)std::max<size_t>(3, (kColdBytes + c_bytes - 1) / c_bytes)
                                         : 1;
  for (int b = 0; b < nbuf; ++b) C.emplace_back(device, c_elems);
  DeviceBuf<int> SA(device, (size_t)tiles * n), SB(device, (size_t)tiles * n);
  DeviceBuf<i64> R(device, (size_t)tiles * tiles * kTile),
      Q(device, (size_t)tiles * tiles * kTile);
  DeviceBuf<int> slab(device, (size_t)tiles * tiles * kStrips * kTile);
  const bool atomic = loop == kSerialAtomic || loop == kVerifyAtomic;
  DeviceBuf<u64> acc(device, (size_t)tiles * tiles * kTile);
  const size_t words = rep_words(cap);
  DeviceBuf<u64> rep(device, words);
  out.rep.assign(words, 0);
  const GemmFn gemm = bind(A.ptr, Bt.ptr);

  Stream gs, vs;
  Event t0, t1, done[2], verified[2];
  HIP_CHECK(hipMemsetAsync(rep.ptr, 0, words * sizeof(u64), gs.s));
  launch_operand(kind, false, A.ptr, n, n, 0, seed, range, nullptr, gs.s);
  launch_operand(kind, false, Bt.ptr, n, n, 1, seed, range, nullptr, gs.s);
  launch_expected(kind, n, n, n, seed, range, SA.ptr, SB.ptr, R.ptr, Q.ptr, gs.s);
  gemm(gs.s, C[0].ptr);  // one warm launch, then the poison over it
  // an unwritten tile must count as malformed, not match stale data
  for (auto& c : C)
    HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c.ptr),
                                (int)kPoisonBits, c_elems, gs.s));
  gs.synchronize();

  auto inject_after = [&](int i, float* c) {
    for (auto& in : inject)
      if ((int)in.iter == i)
        hipLaunchKernelGGL(inject_kernel, dim3(1), dim3(1), 0, gs.s, c,
                           (size_t)in.row * n + in.col, in.mask);
  };
  auto verify = [&](const Stream& s, int i, const float* c) {
    launch_verify(kind, c, n, n, R.ptr, Q.ptr, slab.ptr, rep.ptr, cap, (u32)i, s.s,
                  atomic ? acc.ptr : nullptr);
  };

  t0.record(gs);
  if (loop == kOverlap) {
    for (int i = 0; i < iters; ++i) {
      const int b = i & 1;
      if (i >= 2) HIP_CHECK(hipStreamWaitEvent(gs.s, verified[b].e, 0));
      gemm(gs.s, C[b].ptr);
      inject_after(i, C[b].ptr);
      done[b].record(gs);
      HIP_CHECK(hipStreamWaitEvent(vs.s, done[b].e, 0));
      verify(vs, i, C[b].ptr);
      verified[b].record(vs);
    }
    for (int b = 0; b < std::min(iters, 2); ++b)
      HIP_CHECK(hipStreamWaitEvent(gs.s, verified[b].e, 0));
  } else if (loop == kVerifyOnly || loop == kVerifyCold || loop == kVerifyAtomic) {
    for (auto& c : C) gemm(gs.s, c.ptr);
    t0.record(gs);
    for (int i = 0; i < iters; ++i) verify(gs, i, C[i % nbuf].ptr);
  } else {
    for (int i = 0; i < iters; ++i) {
      gemm(gs.s, C[0].ptr);
      inject_after(i, C[0].ptr);
      if (loop != kUnchecked) verify(gs, i, C[0].ptr);
    }
  }
  HIP_CHECK(hipGetLastError());
  t1.record(gs);

  // corrupted memory or a wrong computation: the stored operands against the
  // generator
  launch_operand(kind, true, A.ptr, n, n, 0, seed, range, rep.ptr, gs.s);
  launch_operand(kind, true, Bt.ptr, n, n, 1, seed, range, rep.ptr, gs.s);
  HIP_CHECK(hipMemcpyAsync(out.rep.data(), rep.ptr, words * sizeof(u64),
                           hipMemcpyDeviceToHost, gs.s));
  gs.synchronize();
  vs.synchronize();
  out.seconds = Event::elapsed_ms(t0, t1) / 1e3;
  return out;
}

int parse_loop(const std::string& name) {
  for (int i = 0; i < kNumLoops; ++i)
    if (name == kLoopNames[i]) return i;
  TORCH_CHECK(false, "gemm_check: unknown loop '", name,
              "' (overlap, serial, unchecked, verify, verify-cold, serial-atomic, "
              "verify-atomic)");
  return -1;
}

// code < 0: the kind's default, the kernel validate_gpus times.
py::dict gemm_check(int device, const std::string& kind_name, int size, int iters,
                    u64 seed, i64 range, int code, i64 max_records,
                    std::vector<std::vector<i64>> inject,
                    const std::string& loop_name) {
  const int kind = parse_kind(kind_name);
  const int loop = parse_loop(loop_name);
  check_device(device);
  check_extent(size, "size");
  check_k(kind, size);
  check_range(kind, size, range);
  TORCH_CHECK(iters >= 1 && iters <= kMaxIters, "iters must be in [1, ", kMaxIters, "]");
  const u64 cap = check_max_records(max_records);
  if (code < 0) code = kDefaultCode[kind];
  std::function<GemmFn(const void*, const void*)> bind;
  if (kind == kBf16) {
    auto kernel = find_variant(kBf16Variants8ph, code, "8-phase variant");
    bind = [=](const void* a, const void* b) -> GemmFn {
      return [=](hipStream_t s, float* c) {
        launch_256(kernel, s, static_cast<const __hip_bfloat16*>(a),
                   static_cast<const __hip_bfloat16*>(b), c, size, size, size);
      };
    };
  } else {
    auto kernel = kind == kFp8 ? find_variant(kFp8MxShapes, code, "fp8 MX shape code")
                               : find_variant(kFp4MxShapes, code, "fp4 MX shape code");
    bind = [=](const void* a, const void* b) -> GemmFn {
      return [=](hipStream_t s, float* c) {
        launch_256(kernel, s, static_cast<const unsigned char*>(a),
                   static_cast<const unsigned char*>(b), c, size, size, size);
      };
    };
  }
  TORCH_CHECK((int)inject.size() <= kMaxInject, "at most ", kMaxInject,
              " inject entries");
  TORCH_CHECK(inject.empty() || loop == kOverlap || loop == kSerial ||
                  loop == kSerialAtomic,
              "inject: only the checked loops take entries");
  std::vector<Inject> inj;
  for (auto& e : inject) {
    TORCH_CHECK(e.size() == 4, "inject: entries are (iter, row, col, xor_mask)");
    TORCH_CHECK(e[0] >= 0 && e[0] < iters, "inject: iteration ", e[0],
                " is outside the ", iters, " iterations");
    TORCH_CHECK(e[1] >= 0 && e[1] < size && e[2] >= 0 && e[2] < size,
                "inject: element (", e[1], ", ", e[2], ") is outside C");
    TORCH_CHECK(e[3] >= 0 && e[3] <= 0xFFFFFFFFll, "inject: ", e[3],
                " is not an unsigned 32-bit mask");
    inj.push_back({(u32)e[0], (u32)e[1], (u32)e[2], (u32)e[3]});
  }
  DriverResult r;
  {
    py::gil_scoped_release release;
    r = run_driver(device, kind, size, iters, seed, (u32)range, cap, inj, loop, bind);
  }
  py::dict d = report_dict(r.rep.data(), cap);
  d["kind"] = kind_name;
  d["code"] = code;
  d["loop"] = loop_name;
  d["size"] = size;
  d["iters"] = iters;
  d["seconds"] = r.seconds;
  d["tflops"] = loop == kVerifyOnly || loop == kVerifyCold || loop == kVerifyAtomic ||
                        r.seconds <= 0
                    ? 0.0
                    : 2.0 * size * (double)size * size * iters / (r.seconds * 1e12);
  d["checked_bytes"] =
      py::int_(loop == kUnchecked ? 0ull : (u64)iters * 4ull * size * size);
  d["operand_errors"] = py::int_(r.rep[kRepOperand]);
  return d;
}

}  // namespace gemm_check
