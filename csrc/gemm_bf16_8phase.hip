// bf16 MFMA GEMM on the 256^2-tile 8-phase skeleton (gemm_8phase_common.h;
// CDNA4 guide §5 "The 256² 8-phase template"). The high tier of the GPU
// health-validation burn-in: the 128^2 double-buffered kernel (gemm_bf16.hip)
// measures ~835 TF; this structure's published figures are ~1330 TF @4096^3
// on random operands.
//
// BK=64: a half-tile is [128][64] bf16; a fragment is one ds_read_b128; each
// quadrant phase runs 16 mfma_f32_16x16x32_bf16 (4 fm x 2 fn x 2 kk).
//
// Variants, by the public `variant` code of gemm_bf16_8ph (odd code = even
// code + the bijective XCD remap; within-probe A/B via gemm_bf16_8ph_ab).
// Four schedule structures have been built and measured:
//   0, 1   in-phase schedule, rolled K loop (the shipped default is 0):
//          reads 12/4/8/0 per phase, single A set, one counted vmcnt per
//          K-tile at phase 3's tail;
//   2, 3   phase-ahead schedule (below);
//   4, 5   in-phase schedule with the K loop unrolled 2 tiles per iteration
//          ("8 phases/iter, 2 K-tiles/iter" as the guide's template states):
//          every LDS slot index becomes a compile-time constant, removing
//          the per-phase (4t+i)&7 address arithmetic;
//   6, 7   as 4, 5 without the manual lgkmcnt fences: the ds_reads are
//          compiler-generated, so the compiler already inserts the minimal
//          s_waitcnt before each dependent MFMA — the manual
//          lgkmcnt(0)+sched_barrier(0) pair is a full drain plus a hard
//          scheduling wall on top of it;
//   12     as 0 with the row-bit-3 LDS swizzle (SWZV=1).
// Codes 8-11 were never variants: they named a merged-phase (8, 9) and a
// static-setprio (10, 11) schedule whose source the template dispatch never
// reached, so they ran the kernels of 6/7 (profiles/gemm_kernel_stats.md).
// That source is gone. 8 and 9 are rejected as unknown; 10 and 11 are still
// accepted as aliases of 6 and 7 until their test cases can be retired too.
//
// Phase-ahead schedule (reads 4/4/8/8: the A(qm=0) fragments of tile t+1 are
// read during tile t's phase 3, so phase 0 starts its MFMA with zero A-read
// latency; needs a second A register set, +32 VGPR, and a counted vmcnt at
// the tail of phases 0/2/3). Invariants (half h of tile t:
// 4t+{0=A0,1=B0,2=A1,3=B1}, staged at phase j of tile t as h=4t+7+j, i.e. 7
// halves ahead):
//   p0: read B0(t)   [cover: p3(t-1) tail vmcnt target 4t+1]; MFMA q(0,0)
//       with A-set0 (read at p3(t-1)) + B-set0;  tail vmcnt -> 4t+3
//   p1: read B1(t)   [cover: p0 tail]; MFMA q(0,1) A-set0 + B-set1
//   p2: read A1(t) -> A-set1 [cover: p0 tail, 4t+2 <= 4t+3]; MFMA q(1,1);
//       tail vmcnt -> 4t+4 (next tile's A0)
//   p3: read A0(t+1) -> A-set0 (last used p1); MFMA q(1,0) A-set1 + B-set0
//       behind lgkmcnt(8) (the 8 fresh reads may stay outstanding — nothing
//       in this phase consumes them); tail vmcnt -> 4t+5 (next B0)
// Every tail vmcnt precedes the phase's closing s_barrier: a per-wave
// s_waitcnt only covers that wave's own glds, so the barrier is what makes
// the guarantee collective before another wave's ds_read consumes the slot.
// Register WAR: A-set0 is rewritten at p3 while q(1,0) reads A-set1; B-set0
// rewritten at p0 after its last read in p3(t-1); slots are never ds_read
// after the phase that may glds-overwrite them (same argument as the
// in-phase schedule).
//
// Constraints: M,N multiples of 256; K multiple of 64 with K >= 192
// (prologue stages 7 half-tiles = tile0 + 3/4 of tile1).
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include "gemm_8phase_common.h"

namespace gemm_bf16_8ph {

using namespace gemm_8ph;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;

enum Sched { ROLLED, PHASE_AHEAD, UNROLLED_FENCED, UNROLLED };

// Per-wave registers and MFMA clusters of the bf16 format. The load_* and
// cluster members take explicit fragment sets so the phase-ahead loop can
// bring its second A set; read_a/read_b/mfma are the policy the shared
// in-phase schedule (gemm_8ph::ktile) drives.
template <int SWZV>
struct Bf16Wave {
  using AFrag = bf16x8[4][2];  // [fm][kk]: 4 m-frags x 2 k-halves
  using BFrag = bf16x8[2][2];  // [fn][kk]

  int arow, brow;  // this lane's fragment row within an A / B half-tile
  int fkb;         // this lane's 16-B k-slice within a 64-B k-half
  AFrag a;         // qm-current A set
  BFrag b[2];      // both B sets kept
  f32x4 acc[2][4][2][2] = {};  // [qm][fm][qn][fn], all indices compile-time

  __device__ explicit Bf16Wave(const TileCoord& c)
      : arow(c.wm * 64 + (c.lane & 15)),
        brow(c.wn * 32 + (c.lane & 15)),
        fkb((c.lane >> 4) * 16) {}

  __device__ __forceinline__ bf16x8 frag(const unsigned char* half, int row,
                                         int kk) const {
    return *reinterpret_cast<const bf16x8*>(
        half + row * ROW_BYTES + swz_byte<SWZV>(row, kk * 64 + fkb));
  }
  __device__ __forceinline__ void load_a(AFrag& dst, const unsigned char* half) const {
#pragma unroll
    for (int fm = 0; fm < 4; ++fm)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) dst[fm][kk] = frag(half, arow + fm * 16, kk);
  }
  __device__ __forceinline__ void load_b(BFrag& dst, const unsigned char* half) const {
#pragma unroll
    for (int fn = 0; fn < 2; ++fn)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) dst[fn][kk] = frag(half, brow + fn * 16, kk);
  }
  template <int QM, int QN>
  __device__ __forceinline__ void cluster(const AFrag& af, const BFrag& bf) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int fm = 0; fm < 4; ++fm)
#pragma unroll
        for (int fn = 0; fn < 2; ++fn)
          acc[QM][fm][QN][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af[fm][kk], bf[fn][kk], acc[QM][fm][QN][fn], 0, 0, 0);
  }

  __device__ __forceinline__ void read_a(const unsigned char* half) { load_a(a, half); }
  template <int SET>
  __device__ __forceinline__ void read_b(const unsigned char* half) { load_b(b[SET], half); }
  template <int QM, int QN>
  __device__ __forceinline__ void mfma() { cluster<QM, QN>(a, b[QN]); }
};

// Ensure (collectively with the following barrier) that half `target` has
// landed: allow only the halves staged after it to remain outstanding.
__device__ inline void wait_half_landed(int staged_through, int target) {
  int allowed = staged_through - target;  // halves issued after `target`
  wait_vmcnt(allowed < 0 ? 0 : (allowed > 5 ? 5 : allowed));
}

// The phase-ahead K loop (header comment). A different schedule from
// gemm_8ph::ktile, built from the same stager, waits and clusters; `a0` is
// the wave's ordinary A set, `a1` the second one.
template <int SWZV>
__device__ __forceinline__ void kloop_phase_ahead(Bf16Wave<SWZV>& w,
                                                  const HalfStager<SWZV>& stage,
                                                  const unsigned char* lds, int T) {
  auto stage_ahead = [&](int h) {
    if (h < 4 * T) stage(h);
  };
  auto open_cluster = [&]() {
    __builtin_amdgcn_s_barrier();
    wait_lgkm0_fence();
    __builtin_amdgcn_s_setprio(1);
  };

  for (int h = 0; h < 7 && h < 4 * T; ++h) stage(h);
  // prologue covers: tile0's A0 (for the prologue A reads) AND B0
  // (consumed by phase 0's in-phase reads after the barrier)
  wait_half_landed(min(7, 4 * T) - 1, 1);
  __builtin_amdgcn_s_barrier();

  typename Bf16Wave<SWZV>::AFrag& a0 = w.a;  // read at p3 of the previous tile
  typename Bf16Wave<SWZV>::AFrag a1;         // read at p2
  w.load_a(a0, lds);  // prologue A-set0 prime (plays the role of p3(t=-1))

  for (int t = 0; t < T; ++t) {
    const unsigned char* Bs0 = lds + ((4 * t + 1) & 7) * HALF_BYTES;
    const unsigned char* As1 = lds + ((4 * t + 2) & 7) * HALF_BYTES;
    const unsigned char* Bs1 = lds + ((4 * t + 3) & 7) * HALF_BYTES;
    const unsigned char* As0n = lds + ((4 * t + 4) & 7) * HALF_BYTES;

    // ---- phase 0: read B0(t); MFMA q(0,0) = a0 x b0; stage 4t+7
    w.load_b(w.b[0], Bs0);
    stage_ahead(4 * t + 7);
    open_cluster();
    w.template cluster<0, 0>(a0, w.b[0]);
    __builtin_amdgcn_s_setprio(0);
    // cover p1's B1(t) (=half 4t+3) collectively via the barrier
    wait_half_landed(min(4 * T, 4 * t + 8) - 1, 4 * t + 3);
    __builtin_amdgcn_s_barrier();

    // ---- phase 1: read B1(t); MFMA q(0,1) = a0 x b1; stage 4t+8
    w.load_b(w.b[1], Bs1);
    stage_ahead(4 * t + 8);
    open_cluster();
    w.template cluster<0, 1>(a0, w.b[1]);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_s_barrier();

    // ---- phase 2: read A1(t); MFMA q(1,1) = a1 x b1; stage 4t+9
    w.load_a(a1, As1);
    stage_ahead(4 * t + 9);
    open_cluster();
    w.template cluster<1, 1>(a1, w.b[1]);
    __builtin_amdgcn_s_setprio(0);
    // cover p3's A0(t+1) (=half 4t+4)
    if (t + 1 < T) wait_half_landed(min(4 * T, 4 * t + 10) - 1, 4 * t + 4);
    __builtin_amdgcn_s_barrier();

    // ---- phase 3: read A0(t+1) phase-AHEAD; MFMA q(1,0) = a1 x b0;
    //      stage 4t+10
    if (t + 1 < T) w.load_a(a0, As0n);
    stage_ahead(4 * t + 10);
    __builtin_amdgcn_s_barrier();
    // the 8 fresh A reads may stay outstanding: q(1,0) uses none of them
    asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
    w.template cluster<1, 0>(a1, w.b[0]);
    __builtin_amdgcn_s_setprio(0);
    // cover next p0's B0(t+1) (=half 4t+5)
    if (t + 1 < T) wait_half_landed(min(4 * T, 4 * t + 11) - 1, 4 * t + 5);
    __builtin_amdgcn_s_barrier();
  }
}

template <int XCD, Sched SCHED, int SWZV = 0>
__global__ __launch_bounds__(THREADS, 2) void gemm_bf16_8phase_kernel(
    const __hip_bfloat16* __restrict__ A,   // [M][K]
    const __hip_bfloat16* __restrict__ Bt,  // [N][K]
    float* __restrict__ C,                  // [M][N]
    int M, int N, int K) {
  __shared__ unsigned char lds[LDS_BYTES];

  const TileCoord c = tile_coord<XCD>(N);
  const int ld = K * 2;  // row stride in bytes
  const HalfStager<SWZV> stage(
      reinterpret_cast<const unsigned char*>(A) + (long)c.bm * ld,
      reinterpret_cast<const unsigned char*>(Bt) + (long)c.bn * ld, ld, lds);
  const int T = ld / ROW_BYTES;
  Bf16Wave<SWZV> w(c);

  if (SCHED == ROLLED) {
    kloop_rolled<false>(w, stage, lds, T);
  } else if (SCHED == PHASE_AHEAD) {
    kloop_phase_ahead<SWZV>(w, stage, lds, T);
  } else {
    // 2 K-tiles (8 phases) per iteration, slot bases 0 and 4
    constexpr bool LG = (SCHED == UNROLLED_FENCED);
    stage_prologue(stage, T);
    int t = 0;
    for (; t + 1 < T; t += 2) {
      ktile<0, LG, false>(w, stage, lds, t, T);
      ktile<4, LG, false>(w, stage, lds, t + 1, T);
    }
    if (t < T)  // odd T tail (t even here, slot base 0)
      ktile<0, LG, false>(w, stage, lds, t, T);
  }

  store_c16<0>(C, N, c, w.acc);
}

}  // namespace gemm_bf16_8ph
