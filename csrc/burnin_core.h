// Shared core of the GPU burn-in's data-checking passes (hbm_memtest.hip,
// cu_check.hip, gemm_check.hip): the one definition of the hash, the exact
// operand generator, the exactness condition and the memtest word patterns,
// plus the two device idioms the kernels share.
//
// Everything above the device section is pure integer (and one exact float)
// arithmetic in plain C++17 with no torch and no HIP runtime call: it compiles
// as host code under g++ and as host and device code under hipcc, so
// burnin_selftest.cpp can hold it to the numpy references of tests/ on a
// machine without a GPU.
#pragma once

#ifdef __HIPCC__
#define BURNIN_FN __host__ __device__ __forceinline__
#else
#define BURNIN_FN inline
#endif

namespace burnin {

using u32 = unsigned int;
using u64 = unsigned long long;
using i64 = long long;

constexpr u32 kGolden = 0x9E3779B9u;
constexpr i64 kTwo24 = 1ll << 24;

BURNIN_FN u32 fmix32(u32 h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

// A u64 seed as the kernels take it: two u32 arguments.
struct SeedHalves {
  u32 lo, hi;
};
BURNIN_FN SeedHalves split_seed(u64 seed) { return {(u32)seed, (u32)(seed >> 32)}; }

// ---------------------------------------------------------------------------
// Formats: the index is the fmt field of both generators' tags
// ---------------------------------------------------------------------------

enum Format { kBf16 = 0, kFp8 = 1, kFp4 = 2, kNumFormats = 3 };
constexpr const char* kFormatNames[kNumFormats] = {"bf16", "fp8", "fp4"};
constexpr int kElemBits[kNumFormats] = {16, 8, 4};
// Ranges: bf16 r in 1..127 (numerators -r..r), e4m3 w in 1..4 (exponent fields
// 6..6+w-1), e2m1 16 (all 16 codes).
constexpr u32 kMinRange[kNumFormats] = {1, 1, 16};
constexpr u32 kFullRange[kNumFormats] = {127, 4, 16};
// Inverse granules: an operand is an integer over 16, 16 or 2, a product an
// integer over 256, 256 or 4.
constexpr float kInvOperandGranule[kNumFormats] = {16.f, 16.f, 2.f};
constexpr float kInvGranule[kNumFormats] = {256.f, 256.f, 4.f};

// ---------------------------------------------------------------------------
// Generator: u = fmix32(key_base(seed, key) ^ tag) picks the element; the tag
// layouts are the checks' own
// ---------------------------------------------------------------------------

BURNIN_FN u32 key_base(u32 seed_lo, u32 seed_hi, u32 key) {
  return fmix32(seed_lo + key * kGolden) ^ seed_hi;
}

// The element as the matrix cores want it: bf16 bits, e4m3 byte or e2m1
// nibble.
//   bf16, range r:  m = (u % (2r+1)) - r, value m/16
//   e4m3, range w:  j = u % (16w+1); code 0x00 for j = 0, otherwise with
//                   q = j-1, s = q / 8w, t = q % 8w:
//                   code = s<<7 | (6 + (t>>3))<<3 | (t&7)
//   e2m1:           code = u & 15
// The range is an argument, or with RANGE a compile-time constant: the
// divisions are then by constants from the start, and elem_code<FMT, R>(u)
// compiles to what a generator written for that one range would.
template <int FMT, u32 RANGE = 0>
BURNIN_FN u32 elem_code(u32 u, u32 range = RANGE) {
  if (RANGE != 0) range = RANGE;
  if (FMT == kBf16) {
    int m = (int)(u % (2u * range + 1u)) - (int)range;
    return __builtin_bit_cast(u32, (float)m * 0.0625f) >> 16;  // 7 bits: exact
  }
  if (FMT == kFp8) {
    u32 j = u % (16u * range + 1u);
    u32 q = j - 1u, s = q / (8u * range), t = q % (8u * range);
    return j == 0 ? 0u : (s << 7 | (6u + (t >> 3)) << 3 | (t & 7u));
  }
  return u & 15u;
}

// The same element as an integer count of granules (1/16, 2^-4, 1/2), from
// the generator's definition and not from the code above.
template <int FMT, u32 RANGE = 0>
BURNIN_FN int elem_int(u32 u, u32 range = RANGE) {
  if (RANGE != 0) range = RANGE;
  if (FMT == kBf16) return (int)(u % (2u * range + 1u)) - (int)range;
  if (FMT == kFp8) {
    u32 j = u % (16u * range + 1u);
    if (j == 0) return 0;
    u32 q = j - 1u, s = q / (8u * range), t = q % (8u * range);
    int mag = (int)((8u + (t & 7u)) << (t >> 3));  // (1+m/8) * 2^(e-7) * 16
    return s ? -mag : mag;
  }
  u32 e = (u >> 1) & 3u, m = u & 1u;
  int mag = e == 0 ? (int)m : (int)((2u + m) << (e - 1u));  // (1+m/2) * 2^(e-1) * 2
  return (u & 8u) ? -mag : mag;
}

// Largest numerator magnitude of a format at a legal range.
BURNIN_FN i64 max_numerator(int fmt, i64 range) {
  if (fmt == kBf16) return range;
  if (fmt == kFp8) return 15ll << (range - 1);
  return 12;
}

// The exactness condition: with `top` the largest numerator, every partial
// sum of K products is an integer number of product granules of magnitude at
// most top^2 * K, exact in fp32 whatever the order of summation while that
// does not exceed 2^24.
BURNIN_FN bool sums_exact(int fmt, i64 range, i64 K) {
  const i64 top = max_numerator(fmt, range);
  return top * top * K <= kTwo24;
}

// ---------------------------------------------------------------------------
// Memtest word patterns (hbm_memtest.hip has the definitions in words)
// ---------------------------------------------------------------------------

enum Pattern { kAddr = 0, kRand = 1, kZero = 2 };

// The two b-dependent terms of "rand". b is the upper half of g ^ seed and
// changes once per 2^32 words, so a tile that does not straddle a multiple
// of 2^32 computes them once, wave-uniformly: two of the six multiplies per
// word leave the per-lane work.
struct HiTerms {
  u32 p, q;
  bool uniform;  // p, q hold for every word of the tile
  BURNIN_FN void set(u32 b) {
    p = b * 0x9E3779B9u;
    q = b * 0x85EBCA77u + 0x27D4EB2Fu;
  }
};

BURNIN_FN u64 rand_word(u32 a, u32 p, u32 q) {
  u32 lo = fmix32(a + p);
  u32 hi = fmix32(~a + q);
  return ((u64)hi << 32) | lo;
}

// Expected value of the single word g.
template <int PAT>
BURNIN_FN u64 pattern_word(u64 g, u64 seed, u64 inv) {
  if (PAT == kZero) return inv;
  u64 x = g ^ seed;
  if (PAT == kAddr) return x ^ inv;
  HiTerms t;
  t.set((u32)(x >> 32));
  return rand_word((u32)x, t.p, t.q) ^ inv;
}

// Terms for the words [g_first, g_first + nwords); every argument is
// wave-uniform, so the branch on .uniform is a scalar one.
BURNIN_FN HiTerms tile_terms(u64 g_first, u64 nwords, u64 seed) {
  HiTerms t;
  t.uniform = (g_first >> 32) == ((g_first + (nwords - 1)) >> 32);
  t.set((u32)((g_first ^ seed) >> 32));
  return t;
}

// Expected values of the two words g0, g0 + 1 of one 16-byte vector.
template <int PAT>
BURNIN_FN void pattern_pair(u64 g0, u64 seed, u64 inv, const HiTerms& t, u64& w0,
                            u64& w1) {
  if (PAT == kRand && t.uniform) {
    const u32 sl = (u32)seed, l0 = (u32)g0;
    w0 = rand_word(l0 ^ sl, t.p, t.q) ^ inv;
    w1 = rand_word((l0 + 1u) ^ sl, t.p, t.q) ^ inv;
  } else {
    w0 = pattern_word<PAT>(g0, seed, inv);
    w1 = pattern_word<PAT>(g0 + 1, seed, inv);
  }
}

// ---------------------------------------------------------------------------
// Device only
// ---------------------------------------------------------------------------
#ifdef __HIPCC__

using f32x4 = __attribute__((ext_vector_type(4))) float;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;

// Replaces v by its sum over the 64 lanes of the wave, in every lane; T is
// u32, u64 or i64.
template <typename T>
__device__ __forceinline__ void wave_sum(T& v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
}

// Claims one record slot of a device-resident u64 report: HEADER words, of
// which word CLAIMED counts the claims, then cap records of REC_WORDS words.
// One claim atomic per finding, and only while the counter is still below the
// cap, so a badly broken card stops issuing them once the records are full.
// True with rec pointing at the claimed record, false (rec untouched) when
// there is none left.
template <int CLAIMED, int HEADER, int REC_WORDS>
__device__ __forceinline__ bool claim_record(u64* rep, u64 cap, u64*& rec) {
  if (cap == 0) return false;
  u64 claimed = __hip_atomic_load(&rep[CLAIMED], __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);
  if (claimed >= cap) return false;
  u64 slot = atomicAdd(&rep[CLAIMED], 1ull);
  if (slot >= cap) return false;
  rec = rep + HEADER + REC_WORDS * slot;
  return true;
}

#endif  // __HIPCC__

}  // namespace burnin
