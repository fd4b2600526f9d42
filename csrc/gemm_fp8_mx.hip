// MX-fp8 (OCP e4m3) and MX-fp4 (e2m1) MFMA GEMM on the 256^2-tile 8-phase
// skeleton (gemm_8phase_common.h).
//
// gfx950's only high-rate fp8 path is the block-scaled MX instruction
// (guide §3: there is NO non-scaled mfma_f32_*x64_fp8; the MX-scaled
// 16x16x128 runs at ~4.6 PF µbench vs 2.1 PF for non-scaled fp8). This
// kernel runs it as a plain fp8 GEMM: every 32-element block scale is
// e8m0 127 (x1.0), so numerics are "e4m3 inputs, fp32 accumulate" up to the
// instruction's own product alignment: within each group of 8 consecutive k
// it truncates product bits below 2^-13 of the group's largest exponent sum
// (measured; docs/testing.md). Operands spanning few exponents never reach
// that cut and accumulate exactly as fp32 would.
//
// Operand layout (verified on hardware by csrc-probe, max err 0.0 vs exact
// integer reference — see profiles/gemm_kernel_stats.md round-2 fp8 note):
//   A: lane l holds row (l&15), k bytes (l>>4)*32 .. +32 (8 VGPRs, v8i32)
//   B: lane l holds col (l&15) of B = row of Bt, same k range
//   C/D: col = lane&15, row = (lane>>4)*4 + reg (shape-determined,
//        dtype-independent on gfx950)
//   scales: opsel 0, low byte 127 on both operands; cbsz=0 blgp=0 (e4m3).
//
// Structure: the shared in-phase schedule in its rolled form (bf16 variant
// 0 — the best of the 4 bf16 schedule structures measured) with a K-step of
// 128 bytes: a half-tile is [128][128] fp8 = 16 KiB — the SAME byte shape
// as the bf16 [128][64] half, so staging, swizzle, slot cadence, counted
// vmcnt and barriers are the skeleton's; only the fragment reads (2x
// ds_read_b128 = 32 B per fragment) and the MFMA cluster (8 independent
// 16x16x128 per phase, no kk loop) differ.
//
// FMT template axis: 0 = fp8 e4m3 (K-step 128), 4 = fp4 e2m1 (K-step 256 —
// nibble-packed, so a [128][256-fp4] half-tile is the SAME 16 KiB byte
// shape; each quadrant phase then runs two 16x16x128 MFMAs per fragment
// pair, one per 128-element k-half, at the 4x fp4 rate). The fp4 operand
// layout (low nibble = even k; 16 bytes in the low 4 dwords of the v8i32
// operand; cbsz=blgp=4) was verified on hardware with the same
// single-MFMA exact-integer probe as fp8 (max abs err 0.0).
//
// Shipped defaults (each measured in both A/B interleave orders; the
// tuning ladder with PMC evidence is profiles/gemm_kernel_stats.md):
//   fp8: SWZV=1 (row-bit-3 swizzle; bank conflicts 44M -> 0, +11%),
//        unmerged phases — 2.22 PF @8192^3 random operands;
//   fp4: SWZV=0, MP23=1 (merged phases 2+3, +1-2%) — 4.02-4.09 PF,
//        bit-exact vs the dequantized fp32 reference.
// MP23 (gemm_8ph::ktile) is measured here and nowhere else: the MX clusters
// retire ~4x faster than bf16's, making the per-phase barrier overhead
// relatively larger.
// Rejected-by-measurement variants stay selectable for A/B: shape 17
// (alternate swizzle), 18 (quad-transpose dwordx4 epilogue), 19/20
// (merge toggles), 32 (the 32x32x64 instruction: only 2 independent
// accumulators per phase against its 64-cycle dependent latency).
//
// Constraints: M,N multiples of 256; K multiple of 128 (fp8) / 256 (fp4),
// K >= 2 K-steps.
#include <hip/hip_runtime.h>

#include "gemm_8phase_common.h"

namespace gemm_fp8_mx {

using namespace gemm_8ph;
using f32x16 = __attribute__((ext_vector_type(16))) float;
using i32x4 = __attribute__((ext_vector_type(4))) int;
using i32x8 = __attribute__((ext_vector_type(8))) int;

// One MFMA operand fragment at byte offset kb of a half-tile row.
// fp8: 32 B as two independently-swizzled 16-B chunks; fp4: 16 B = 32
// nibbles in the low 4 dwords.
template <int FMT, int SWZV>
__device__ __forceinline__ i32x8 read_frag(const unsigned char* half, int row,
                                           int kb) {
  const unsigned char* r = half + row * ROW_BYTES;
  i32x4 lo = *reinterpret_cast<const i32x4*>(r + swz_byte<SWZV>(row, kb));
  if (FMT == 4) return i32x8{lo[0], lo[1], lo[2], lo[3], 0, 0, 0, 0};
  i32x4 hi = *reinterpret_cast<const i32x4*>(r + swz_byte<SWZV>(row, kb + 16));
  return i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// Policy of the 16x16x128 instruction: per-wave 4 m-frags x 2 n-frags per
// quadrant, KS k-steps of 64 B per K-tile row (fp8: one 32-B fragment per
// lane; fp4: one 16-B fragment per 128-element k-half).
template <int FMT, int SWZV>
struct Mx16Wave {
  static constexpr int KS = (FMT == 4) ? 2 : 1;

  int arow, brow, fkb;
  i32x8 a[4][KS];       // [fm][ks], qm-current A set
  i32x8 b[2][2][KS];    // [set][fn][ks]
  f32x4 acc[2][4][2][2] = {};

  __device__ explicit Mx16Wave(const TileCoord& c)
      : arow(c.wm * 64 + (c.lane & 15)),
        brow(c.wn * 32 + (c.lane & 15)),
        fkb((c.lane >> 4) * (FMT == 4 ? 16 : 32)) {}

  __device__ __forceinline__ void read_a(const unsigned char* half) {
#pragma unroll
    for (int fm = 0; fm < 4; ++fm)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        a[fm][ks] = read_frag<FMT, SWZV>(half, arow + fm * 16, ks * 64 + fkb);
  }
  template <int SET>
  __device__ __forceinline__ void read_b(const unsigned char* half) {
#pragma unroll
    for (int fn = 0; fn < 2; ++fn)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        b[SET][fn][ks] = read_frag<FMT, SWZV>(half, brow + fn * 16, ks * 64 + fkb);
  }
  template <int QM, int QN>
  __device__ __forceinline__ void mfma() {
#pragma unroll
    for (int fm = 0; fm < 4; ++fm)
#pragma unroll
      for (int fn = 0; fn < 2; ++fn)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
          acc[QM][fm][QN][fn] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
              a[fm][ks], b[QN][fn][ks], acc[QM][fm][QN][fn], FMT, FMT, 0, 127,
              0, 127);
  }
};

// Policy of the 32x32x64 instruction: fragments are 32-row/32-col, each
// phase runs {fp8: 2 m-frags x 2 k-steps, fp4: 2 x 4} MFMAs (~25% higher
// uarch ceiling than 16x16x128 — guide §3 µbench 9099 vs 7228 TF fp4).
// Operand/C-D layouts hardware-verified by csrc-probe (max abs err 0.0):
// A lane l = row l&31, k (l>>5)*32 elements; C col = lane&31,
// row = (reg&3) + 8*(reg>>2) + 4*(lane>>5).
template <int FMT, int SWZV>
struct Mx32Wave {
  static constexpr int KSTEPS = (FMT == 4) ? 4 : 2;    // 32B(fp4)/64B(fp8) per step
  static constexpr int STEPB = ROW_BYTES / KSTEPS;     // bytes per k-step row-slice
  static constexpr int LANEB = STEPB / 2;              // per-lane slice (l>>5 half)

  int arow, brow, fkb;
  i32x8 a[2][KSTEPS];   // [fm][ks]
  i32x8 b[2][KSTEPS];   // [set][ks]; one 32-col frag per wave
  f32x16 acc[2][2][2] = {};  // [qm][fm][qn]

  __device__ explicit Mx32Wave(const TileCoord& c)
      : arow(c.wm * 64 + (c.lane & 31)),
        brow(c.wn * 32 + (c.lane & 31)),
        fkb((c.lane >> 5) * LANEB) {}

  __device__ __forceinline__ void read_a(const unsigned char* half) {
#pragma unroll
    for (int fm = 0; fm < 2; ++fm)
#pragma unroll
      for (int ks = 0; ks < KSTEPS; ++ks)
        a[fm][ks] = read_frag<FMT, SWZV>(half, arow + fm * 32, ks * STEPB + fkb);
  }
  template <int SET>
  __device__ __forceinline__ void read_b(const unsigned char* half) {
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks)
      b[SET][ks] = read_frag<FMT, SWZV>(half, brow, ks * STEPB + fkb);
  }
  template <int QM, int QN>
  __device__ __forceinline__ void mfma() {
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks)
#pragma unroll
      for (int fm = 0; fm < 2; ++fm)
        acc[QM][fm][QN] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
            a[fm][ks], b[QN][ks], acc[QM][fm][QN], FMT, FMT, 0, 127, 0, 127);
  }

  __device__ inline void store(float* __restrict__ C, int N,
                               const TileCoord& c) const {
    const int ccol = c.lane & 31;
    const int rbase = 4 * (c.lane >> 5);
#pragma unroll
    for (int qm = 0; qm < 2; ++qm)
#pragma unroll
      for (int fm = 0; fm < 2; ++fm)
#pragma unroll
        for (int qn = 0; qn < 2; ++qn) {
          int row0 = c.bm + qm * 128 + c.wm * 64 + fm * 32;
          int col = c.bn + qn * 128 + c.wn * 32 + ccol;
#pragma unroll
          for (int reg = 0; reg < 16; ++reg) {
            int r = (reg & 3) + 8 * (reg >> 2) + rbase;
            C[(long)(row0 + r) * N + col] = acc[qm][fm][qn][reg];
          }
        }
  }
};

// Shared kernel body: block panels, rolled in-phase K loop over `w`.
template <int FMT, int SWZV, bool MP23, typename WAVE>
__device__ __forceinline__ void mx_kloop(WAVE& w, const TileCoord& c,
                                         const unsigned char* A,
                                         const unsigned char* Bt, int K,
                                         unsigned char* lds) {
  const int Kb = (FMT == 4) ? K / 2 : K;  // row stride in bytes
  const HalfStager<SWZV> stage(A + (long)c.bm * Kb, Bt + (long)c.bn * Kb, Kb, lds);
  kloop_rolled<MP23>(w, stage, lds, Kb / ROW_BYTES);
}

// EPI: 1 = quad-transpose dwordx4 epilogue; MP23: merged phases 2+3.
template <int FMT, int SWZV = 0, int EPI = 0, int MP23 = 0>
__global__ __launch_bounds__(THREADS, 2) void gemm_fp8_mx_kernel(
    const unsigned char* __restrict__ A,   // [M][K] packed
    const unsigned char* __restrict__ Bt,  // [N][K] packed
    float* __restrict__ C,                 // [M][N]
    int M, int N, int K) {                 // K in ELEMENTS
  __shared__ unsigned char lds[LDS_BYTES];
  const TileCoord c = tile_coord<0>(N);
  Mx16Wave<FMT, SWZV> w(c);
  mx_kloop<FMT, SWZV, MP23 != 0>(w, c, A, Bt, K, lds);
  store_c16<EPI>(C, N, c, w.acc);
}

template <int FMT, int SWZV = 0>  // FMT: 0 = fp8 e4m3, 4 = fp4 e2m1
__global__ __launch_bounds__(THREADS, 2) void gemm_mx32_kernel(
    const unsigned char* __restrict__ A,   // [M][K] packed
    const unsigned char* __restrict__ Bt,  // [N][K] packed
    float* __restrict__ C,                 // [M][N]
    int M, int N, int K) {                 // K in ELEMENTS
  __shared__ unsigned char lds[LDS_BYTES];
  const TileCoord c = tile_coord<0>(N);
  Mx32Wave<FMT, SWZV> w(c);
  mx_kloop<FMT, SWZV, false>(w, c, A, Bt, K, lds);
  w.store(C, N, c);
}

// pseudorandom VALID e4m3 fill: full sign/mantissa variation, exponents
// bounded so products stay finite (bench-honesty: zero or sign-stuck fills
// inflate TF via DVFS — guide §5.4 rule 25)
__global__ void fill_e4m3_hash_kernel(unsigned char* p, size_t n, unsigned seed) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    unsigned h = (unsigned)(i * 2654435761u) ^ seed;
    h ^= h >> 13;
    h *= 0x85ebca6bu;
    h ^= h >> 16;
    // sign = bit 0; exponent in [4..11] (values ~2^-3 .. 2^4); mantissa 3 bits
    unsigned char b = (unsigned char)(((h & 1u) << 7) | ((((h >> 1) & 7u) + 4u) << 3) |
                                      ((h >> 4) & 7u));
    p[i] = b;
  }
}

// pseudorandom e2m1 (fp4) nibble fill: all 16 codes are valid values
__global__ void fill_e2m1_hash_kernel(unsigned char* p, size_t n, unsigned seed) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    unsigned h = (unsigned)(i * 2654435761u) ^ seed;
    h ^= h >> 13;
    h *= 0x85ebca6bu;
    h ^= h >> 16;
    p[i] = (unsigned char)(h & 0xFF);
  }
}

}  // namespace gemm_fp8_mx
