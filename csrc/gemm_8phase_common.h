// Shared skeleton of the 256^2-tile 8-phase GEMM family (CDNA4 guide §5
// "The 256² 8-phase template"): bf16 (gemm_bf16_8phase.hip) and MX fp8/fp4
// (gemm_fp8_mx.hip). Geometry, staging, swizzle, waits, the in-phase K-tile
// schedule and the 16x16 epilogue exist here once; a format contributes only
// a policy type (fragment registers, read_a/read_b from a half-tile, one
// quadrant's MFMA cluster, the accumulator and its store).
//
// Geometry: 256x256 output tile, 8 waves as 2(M)x4(N) = 512 threads, per-wave
// output 128x64. One K-tile is 4 half-tiles (A0, B0, A1, B1) of 128 rows x
// 128 BYTES = 16 KiB each: [128][64] bf16, [128][128] fp8 and [128][256] fp4
// all have this byte shape, so everything below addresses in bytes. LDS holds
// 8 half-tile slots (2 K-tiles) = 128 KiB; half h lives in slot h&7.
#pragma once
#include <hip/hip_runtime.h>

namespace gemm_8ph {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int TILE = 256;                        // BM = BN
constexpr int THREADS = 512;                     // 8 waves, 2(M) x 4(N)
constexpr int ROW_BYTES = 128;                   // one half-tile row = one K-step
constexpr int HALF_BYTES = 128 * ROW_BYTES;      // 16 KiB
constexpr int SLOTS = 8;                         // 2 buffers x 4 half-tiles
constexpr int LDS_BYTES = SLOTS * HALF_BYTES;    // 128 KiB
constexpr int NXCD = 8;

__device__ inline void glds16(const unsigned char* gsrc, unsigned char* lds) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) unsigned int*)gsrc,
      (__attribute__((address_space(3))) unsigned int*)lds, 16, 0, 0);
}

// LDS XOR swizzle (chunk-xor form, 16-B granules): a ds_read_b128 16-lane
// group whose rows are distinct mod 8 spreads over 8 16-B slots. SWZV selects
// the row hash g(row):
//   0: g = row&7. Measured on the bf16 kernel (PMC SQ_LDS_BANK_CONFLICT per
//      4096^3 dispatch): st_16x32 single-bit 12.6M conflicts; this form 0.
//      The full (row&15)<<4 conflict-free form measured SLOWER (881-951 vs
//      1020-1073 TF): its row-scattered glds source costs more in fetch than
//      the residual conflicts gain. fp8's two-chunk fragment reads measured
//      44M conflicts/6-dispatch with it — rows r and r+8 always collide
//      under a 3-bit hash of row&7;
//   1: g = (row&7) ^ ((row>>3)&1) — folds row bit 3 into the hash, making
//      the 16 rows of a b128 lane group land on 16 disjoint 4-bank spans
//      (derivation in profiles/gemm_kernel_stats.md; +11% on fp8).
// Any per-row xor is self-inverse, so the glds SOURCE address (HalfStager)
// and the ds_read address share the formula — guide §5.4 rule 21,
// both-sides-or-neither: the LDS destination stays lane-linear because glds
// writes base + lane*16.
template <int SWZV>
__device__ inline int swz_byte(int row, int byte_off) {
  int g = (row & 7) ^ (SWZV ? ((row >> 3) & 1) : 0);
  return byte_off ^ (g << 4);
}

// Stages half-tiles of this block's operand panels: 1024 16-B slots per
// half, 512 threads x 2 passes. LDS destination is lane-linear (slot order ==
// lds address order); the swizzle permutes which global 16-B chunk lands in
// each slot. A thread's source and destination offsets within a half-tile
// never change, so they are formed once.
template <int SWZV>
struct HalfStager {
  const unsigned char* a_blk;  // this block's 256 rows of A, row stride ld
  const unsigned char* b_blk;  // this block's 256 rows of Bt
  int ld;                      // row stride in bytes
  unsigned char* lds;
  // per pass; int as in the kernels this replaces: 127 * ld must fit, i.e.
  // a row stride below 16 MiB (K < 8M bf16/fp8 elements)
  int src_off[2], dst_off[2];

  __device__ inline HalfStager(const unsigned char* a_blk,
                               const unsigned char* b_blk, int ld,
                               unsigned char* lds)
      : a_blk(a_blk), b_blk(b_blk), ld(ld), lds(lds) {
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      int slot = pass * THREADS + threadIdx.x;
      int row = slot >> 3;
      int byte_off = (slot & 7) * 16;
      src_off[pass] = row * ld + swz_byte<SWZV>(row, byte_off);
      dst_off[pass] = row * ROW_BYTES + byte_off;
    }
  }

  // half h = 4*tile + {0=A0, 1=B0, 2=A1, 3=B1} into `slot`
  __device__ inline void operator()(int h, int slot) const {
    int c = h & 3;
    int tt = h >> 2;
    const unsigned char* g;
    if (c == 0)
      g = a_blk + tt * ROW_BYTES;
    else if (c == 1)
      g = b_blk + tt * ROW_BYTES;
    else if (c == 2)
      g = a_blk + (long)128 * ld + tt * ROW_BYTES;
    else
      g = b_blk + (long)128 * ld + tt * ROW_BYTES;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass)
      glds16(g + src_off[pass], lds + slot * HALF_BYTES + dst_off[pass]);
  }
  // ... into its home slot h&7
  __device__ inline void operator()(int h) const { (*this)(h, h & 7); }
};

__device__ inline void wait_lgkm0_fence() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// wait until at most `halves_outstanding` half-tiles (2 glds each) of this
// wave's global_load_lds traffic remain in flight
__device__ inline void wait_vmcnt(int halves_outstanding) {
  switch (halves_outstanding) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
  }
  __builtin_amdgcn_sched_barrier(0);
}

// Tail wait of K-tile t: tile t+1's four halves (through 4t+7) must be
// complete before its phase-0 ds_reads, so only the halves staged after
// them (`staged` = halves issued so far) may stay in flight. Every tail
// vmcnt precedes its phase's closing s_barrier: a per-wave s_waitcnt only
// covers that wave's own glds, so the barrier is what makes the guarantee
// collective before another wave's ds_read consumes the slot.
__device__ inline void wait_next_tile_landed(int staged, int t) {
  int allowed = staged - 4 * (t + 2);
  wait_vmcnt(allowed < 0 ? 0 : (allowed > 3 ? 3 : allowed));
}

// Prologue of the in-phase schedule: tile 0 fully + 3 halves of tile 1 (the
// guide's 4 then +3), so K must cover at least 7 halves.
template <typename STAGE>
__device__ inline void stage_prologue(const STAGE& stage, int T) {
  // runs once: keep the loops rolled rather than spend code size on them
#pragma nounroll
  for (int h = 0; h < 4 && h < 4 * T; ++h) stage(h);
  wait_vmcnt(2);  // A0,B0 of tile 0 complete
#pragma nounroll
  for (int h = 4; h < 7 && h < 4 * T; ++h) stage(h);
  wait_vmcnt(3);  // all of tile 0 complete (<=3 halves of tile 1 in flight)
  __builtin_amdgcn_s_barrier();
}

// Workgroup -> output tile and wave/lane position within it.
struct TileCoord {
  int bm, bn;    // tile origin in C
  int lane;
  int wm, wn;    // wave's 64-row band of each A half, 32-col band of each B half
};

// XCD=1: bijective XCD-contiguous remap (guide T1): hardware round-robins
// consecutive blockIdx across the 8 XCDs; give XCD x the contiguous tile
// range instead so neighboring tiles (shared A panel) hit its private L2
// (+10±3% on bf16 GEMM @8k).
template <int XCD>
__device__ inline TileCoord tile_coord(int N) {
  int bid = (int)blockIdx.x;
  if (XCD) {
    int nwg = (int)gridDim.x;
    int q = nwg / NXCD, r = nwg % NXCD;
    int xcd = bid % NXCD, seq = bid / NXCD;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + seq;
  }
  const int tiles_n = N / TILE;
  const int wave = threadIdx.x >> 6;
  return TileCoord{(bid / tiles_n) * TILE, (bid % tiles_n) * TILE,
                   (int)(threadIdx.x & 63), wave >> 2, wave & 3};
}

// One K-tile (4 phases) of the in-phase schedule, the only copy. Per K-tile
// the reads go 12/4/8/0 per phase with a single A register set:
//   p0: read A0 + B0, stage 4t+7,  MFMA q(0,0)
//   p1: read B1,      stage 4t+8,  MFMA q(0,1)
//   p2: read A1,      stage 4t+9,  MFMA q(1,1)
//   p3: (no reads)    stage 4t+10, MFMA q(1,0) — B set 0 still live
// and one counted vmcnt at the tile's tail. A slot is never ds_read after
// the phase that may glds-overwrite it.
//
// SBASE: -1 = rolled loop, slots (4t+i)&7 computed at run time; 0 or 4 =
//   compile-time slot base (4t)&7 of the two-tile-unrolled form, which makes
//   every slot and staging destination a constant.
// LGKM: manual lgkm waits — lgkmcnt(8) before phase 0's barrier (12 ds_reads
//   issued: lets the first land while the rest fly) and a full
//   lgkmcnt(0)+sched_barrier(0) fence before every cluster. Off = the
//   compiler's own minimal s_waitcnt before each dependent MFMA.
// MP23: phases 2+3 merged into one barrier section (3 barrier pairs per
//   K-tile). The h=4t+10 stage cannot stay in the merged phase — it
//   overwrites the A1 slot while OTHER waves' A1 ds_reads may be in flight
//   (only a barrier after every wave's lgkm drain makes the slot safe) — so
//   it is deferred to the next tile's phase 0 (as half 4(t+1)+6, ahead of
//   4(t+1)+7), costing one half-tile of prefetch depth at the tile boundary.
template <int SBASE, bool LGKM, bool MP23, typename POLICY, typename STAGE>
__device__ __forceinline__ void ktile(POLICY& p, const STAGE& stage,
                                      const unsigned char* lds, int t, int T) {
  const int sb = SBASE >= 0 ? SBASE : 4 * t;
  const unsigned char* As0 = lds + ((sb + 0) & 7) * HALF_BYTES;
  const unsigned char* Bs0 = lds + ((sb + 1) & 7) * HALF_BYTES;
  const unsigned char* As1 = lds + ((sb + 2) & 7) * HALF_BYTES;
  const unsigned char* Bs1 = lds + ((sb + 3) & 7) * HALF_BYTES;

  auto stage_ahead = [&](int k) {  // half 4t+k, if the K range has it
    if (4 * t + k < 4 * T) {
      if (SBASE >= 0)
        stage(4 * t + k, (SBASE + k) & 7);
      else
        stage(4 * t + k);
    }
  };
  auto open_cluster = [&]() {
    __builtin_amdgcn_s_barrier();
    if (LGKM) wait_lgkm0_fence();
    __builtin_amdgcn_s_setprio(1);
  };
  auto close_cluster = [&]() {
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_s_barrier();
  };

  // ---- phase 0: quadrant (0,0)
  p.read_a(As0);
  p.template read_b<0>(Bs0);
  if (MP23 && t > 0) stage_ahead(6);  // deferred from the previous merged phase
  stage_ahead(7);
  if (LGKM) asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");
  open_cluster();
  p.template mfma<0, 0>();
  close_cluster();

  // ---- phase 1: quadrant (0,1)
  p.template read_b<1>(Bs1);
  stage_ahead(8);
  open_cluster();
  p.template mfma<0, 1>();
  close_cluster();

  // ---- phase 2: quadrant (1,1); A(qm=1) replaces A(qm=0)
  p.read_a(As1);
  stage_ahead(9);
  open_cluster();
  p.template mfma<1, 1>();
  if (!MP23) {
    close_cluster();
    // ---- phase 3: quadrant (1,0)
    stage_ahead(10);
    open_cluster();
  }
  p.template mfma<1, 0>();
  __builtin_amdgcn_s_setprio(0);
  wait_next_tile_landed(min(4 * T, 4 * t + (MP23 ? 10 : 11)), t);
  __builtin_amdgcn_s_barrier();
}

// The rolled K loop: prologue + one ktile per K-tile.
template <bool MP23, typename POLICY, typename STAGE>
__device__ __forceinline__ void kloop_rolled(POLICY& p, const STAGE& stage,
                                             const unsigned char* lds, int T) {
  stage_prologue(stage, T);
  for (int t = 0; t < T; ++t) ktile<-1, true, MP23>(p, stage, lds, t, T);
}

// In-quad 4x4 transpose of an MFMA f32x4 fragment (rows r0..r0+3, col =
// own lane) so lane 4g+j ends holding row r0+j across the quad's 4 cols —
// one global_store_dwordx4 instead of four scattered dword stores. Two
// bit-exchange rounds (element-bit b <-> lane-bit b) via shfl_xor, which
// hipcc lowers to DPP quad_perm (no LDS). Guide T-epilogue: a store tail
// is often ISSUE-bound, so 4x fewer store instructions at equal bytes.
__device__ inline f32x4 quad_transpose(f32x4 v, int lane) {
  const int j = lane & 3;
  f32x4 u, w;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float ex = __shfl_xor(v[r ^ 1], 1);
    u[r] = ((r & 1) == (j & 1)) ? v[r] : ex;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float ex = __shfl_xor(u[r ^ 2], 2);
    w[r] = ((r & 2) == (j & 2)) ? u[r] : ex;
  }
  return w;
}

// Epilogue for 16x16 MFMA accumulators acc[qm][fm][qn][fn]: C/D map col =
// lane&15, row = (lane>>4)*4 + r (guide §3). EPI=1 stores each fragment as
// one dwordx4 after quad_transpose.
template <int EPI>
__device__ inline void store_c16(float* __restrict__ C, int N,
                                 const TileCoord& c,
                                 const f32x4 (&acc)[2][4][2][2]) {
  const int ccol = c.lane & 15;
  const int crow = (c.lane >> 4) * 4;
#pragma unroll
  for (int qm = 0; qm < 2; ++qm)
#pragma unroll
    for (int fm = 0; fm < 4; ++fm)
#pragma unroll
      for (int qn = 0; qn < 2; ++qn)
#pragma unroll
        for (int fn = 0; fn < 2; ++fn) {
          int row0 = c.bm + qm * 128 + c.wm * 64 + fm * 16 + crow;
          if (EPI == 1) {
            f32x4 w = quad_transpose(acc[qm][fm][qn][fn], c.lane);
            int colq = c.bn + qn * 128 + c.wn * 32 + fn * 16 + (c.lane & 12);
            *reinterpret_cast<f32x4*>(
                &C[(long)(row0 + (c.lane & 3)) * N + colq]) = w;
          } else {
            int col = c.bn + qn * 128 + c.wn * 32 + fn * 16 + ccol;
#pragma unroll
            for (int r = 0; r < 4; ++r)
              C[(long)(row0 + r) * N + col] = acc[qm][fm][qn][fn][r];
          }
        }
}

}  // namespace gemm_8ph
