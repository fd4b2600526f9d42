// Shared core of the GPU burn-in's data-checking passes (hbm_memtest.hip,
// cu_check.hip, gemm_check.hip, valu_check.hip): the one definition of the
// hash, the exact operand generator, the exactness condition, the memtest
// word patterns and the vector ALU tests, plus the two device idioms the
// kernels share.
//
// Everything above the device section is integer and exactly rounded float
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
// Vector ALU check (valu_check.hip has the launch and the record in words)
//
// Five tests, each a round of kValuSteps steps per lane. Step s of test t
// runs operation s % kValuOps[t] on operands drawn from counter hashes,
//
//   u(operand) = fmix32(key_base(seed_lo, seed_hi, round)
//                       ^ (test<<28 | step<<12 | operand<<8 | lane))
//
// never from an earlier result, and always lane-dependent: a wave-uniform
// operand would let the compiler do the work on the scalar ALU. The result
// bits of every step are folded into the lane's digest, d = fmix32(d ^ bits)
// from d = 0, low word then high word for a 64-bit result.
//
// The four exact tests below are plain C++ (integer arithmetic, and IEEE
// round-to-nearest-even fma / mul / add / sub / conversions with contraction
// off), so the host computes the very digests the GPU must report. The few
// operations plain C++ does not reliably turn into the intended instruction
// use the device builtin, with a twin written from the instruction's
// definition for the host. A g++ build for a target with FMA instructions
// needs -ffp-contract=off (g++ has no pragma for it); burnin_selftest.cpp
// checks that a separate multiply and add stayed separate.
// ---------------------------------------------------------------------------

#ifdef __clang__
#define BURNIN_UNROLL _Pragma("unroll")
#define BURNIN_FP_STRICT _Pragma("clang fp contract(off)")
#else
#define BURNIN_UNROLL
#define BURNIN_FP_STRICT
#endif

enum ValuTest {
  kValuInt = 0,
  kValuF32 = 1,
  kValuF64 = 2,
  kValuPk16 = 3,
  kValuTrans = 4,
  kNumValuTests = 5,
  kNumValuExact = 4,  // the tests with a host twin: all but trans
};
constexpr const char* kValuTestNames[kNumValuTests] = {"int", "f32", "f64", "pk16",
                                                       "trans"};
constexpr u32 kValuSteps = 256;
// Operations a test cycles through by step.
constexpr u32 kValuOps[kNumValuTests] = {16, 8, 4, 4, 5};

// Exponent-field windows of the float operands: sign and mantissa are random,
// the exponent field is forced into [lo, hi]. Every operand then has a
// magnitude in [2^-7, 2^8) (fp16: [2^-4, 2^5)), so no NaN, infinity or
// overflow can arise, and no f32 or f64 denormal either: a product is a
// multiple of 2^-60 (f64: 2^-118) and a sum of operands one of 2^-30 (2^-59),
// so the smallest non-zero result of a cancellation is far above the smallest
// normal number. fp16 is the exception on purpose: a product is a multiple of
// 2^-28 and the smallest normal is 2^-14, so a cancelling packed fma does
// reach the subnormal range and shows whether the hardware keeps it.
constexpr u32 kValuF32ExpLo = 120, kValuF32ExpHi = 134;
constexpr u32 kValuF64ExpLo = 1016, kValuF64ExpHi = 1030;
constexpr u32 kValuF16ExpLo = 11, kValuF16ExpHi = 19;

// The pk16 host twin computes a*b + c of fp16 operands in double and rounds
// once. That is exact while every bit of the product and the addend fits one
// double: from the lowest bit of a product, 2^(2*(lo - 15 - 10)), to above
// the largest sum, 2^(2*(hi - 15 + 1) + 1).
constexpr int valu_pk16_span_bits(int lo, int hi) {
  return (2 * (hi - 15 + 1) + 1) - 2 * (lo - 15 - 10);
}
constexpr bool valu_pk16_double_exact(int lo, int hi) {
  return valu_pk16_span_bits(lo, hi) <= 53;
}
static_assert(valu_pk16_double_exact(kValuF16ExpLo, kValuF16ExpHi),
              "the fp16 window is too wide for the double twin");

BURNIN_FN u32 valu_draw(u32 base, u32 test, u32 step, u32 operand, u32 lane) {
  return fmix32(base ^ (test << 28 | step << 12 | operand << 8 | lane));
}

BURNIN_FN float valu_f32(u32 u) {
  const u32 field =
      kValuF32ExpLo + ((u >> 23) & 0xFFu) % (kValuF32ExpHi - kValuF32ExpLo + 1u);
  return __builtin_bit_cast(float, (u & 0x807FFFFFu) | field << 23);
}

BURNIN_FN double valu_f64(u32 hi, u32 lo) {
  const u32 field =
      kValuF64ExpLo + ((hi >> 20) & 0x7FFu) % (kValuF64ExpHi - kValuF64ExpLo + 1u);
  return __builtin_bit_cast(double, (u64)((hi & 0x800FFFFFu) | field << 20) << 32 | lo);
}

// fp16 bits from the low 16 bits of h.
BURNIN_FN u32 valu_f16(u32 h) {
  const u32 field =
      kValuF16ExpLo + ((h >> 10) & 31u) % (kValuF16ExpHi - kValuF16ExpLo + 1u);
  return (h & 0x83FFu) | field << 10;
}
BURNIN_FN u32 valu_pk16(u32 u) { return valu_f16(u & 0xFFFFu) | valu_f16(u >> 16) << 16; }

// Any finite fp16 as a double (exact).
BURNIN_FN double f16_bits_to_double(u32 h) {
  const u32 e = (h >> 10) & 31u, m = h & 0x3FFu;
  // 2^(e-25) and 2^-24 as doubles, built from their bits
  const double scale =
      __builtin_bit_cast(double, (u64)(1023u + (e ? e : 1u) - 25u) << 52);
  const double mag = (double)((e ? 1024u : 0u) + m) * scale;
  return (h & 0x8000u) ? -mag : mag;
}

// A finite double rounded once to fp16, round-to-nearest-even, with
// subnormal results and overflow to infinity, in integer arithmetic.
BURNIN_FN u32 f16_bits_from_double(double v) {
  const u64 b = __builtin_bit_cast(u64, v);
  const u32 sign = (u32)(b >> 48) & 0x8000u;
  const int ef = (int)((b >> 52) & 0x7FFu);
  if (ef == 0) return sign;  // zero (a double denormal is far below 2^-25)
  const int e = ef - 1023;
  const u64 mant = (b & ((1ull << 52) - 1)) | 1ull << 52;
  // keep 10 fraction bits of a normal result, fewer below 2^-14
  const int shift = e >= -14 ? 42 : 42 + (-14 - e);
  if (shift > 54) return sign;  // below half the smallest subnormal
  u64 q = mant >> shift;
  const u64 rem = mant & ((1ull << shift) - 1), half = 1ull << (shift - 1);
  if (rem > half || (rem == half && (q & 1))) ++q;
  // a normal q carries its implicit bit: it adds 1 to the exponent field, and
  // a rounding carry moves on into it by itself
  const u64 bits = e >= -14 ? ((u64)(e + 14) << 10) + q : q;
  return sign | (bits >= 0x7C00u ? 0x7C00u : (u32)bits);
}

BURNIN_FN u32 valu_perm_twin(u32 a, u32 b, u32 sel) {
  // v_perm_b32 with selectors 0..7: byte i of the result is byte sel_i of the
  // 8 bytes {a, b}, b the low four
  const u64 both = (u64)a << 32 | b;
  u32 r = 0;
  for (u32 i = 0; i < 4; ++i)
    r |= (u32)((both >> (8u * ((sel >> (8u * i)) & 7u))) & 0xFFu) << (8u * i);
  return r;
}

BURNIN_FN u32 valu_sad_u8_twin(u32 a, u32 b, u32 c) {
  for (u32 i = 0; i < 4; ++i) {
    const u32 x = (a >> (8u * i)) & 0xFFu, y = (b >> (8u * i)) & 0xFFu;
    c += x > y ? x - y : y - x;
  }
  return c;
}

BURNIN_FN u32 valu_bfe_twin(u32 a, u32 off, u32 width) {
  return (a >> off) & ((1u << width) - 1u);  // off, width in 0..31
}

BURNIN_FN u32 valu_perm(u32 a, u32 b, u32 sel) {
#ifdef __HIP_DEVICE_COMPILE__
  return __builtin_amdgcn_perm(a, b, sel);
#else
  return valu_perm_twin(a, b, sel);
#endif
}
BURNIN_FN u32 valu_sad_u8(u32 a, u32 b, u32 c) {
#ifdef __HIP_DEVICE_COMPILE__
  return __builtin_amdgcn_sad_u8(a, b, c);
#else
  return valu_sad_u8_twin(a, b, c);
#endif
}
BURNIN_FN u32 valu_bfe(u32 a, u32 off, u32 width) {
#ifdef __HIP_DEVICE_COMPILE__
  return __builtin_amdgcn_ubfe(a, off, width);
#else
  return valu_bfe_twin(a, off, width);
#endif
}

// One step's result: lo, and hi where the operation's result has 64 bits.
struct ValuResult {
  u32 lo, hi;
  bool wide;
};

BURNIN_FN u32 valu_fold(u32 d, const ValuResult& r) {
  d = fmix32(d ^ r.lo);
  return r.wide ? fmix32(d ^ r.hi) : d;
}

// int: unsigned types throughout, signed views by conversion only.
BURNIN_FN ValuResult valu_int_step(u32 base, u32 step, u32 op, u32 lane) {
  const u32 a = valu_draw(base, kValuInt, step, 0, lane);
  const u32 b = valu_draw(base, kValuInt, step, 1, lane);
  const u32 c = valu_draw(base, kValuInt, step, 2, lane);
  const u32 d = valu_draw(base, kValuInt, step, 3, lane);
  const u64 x = (u64)b << 32 | a, y = (u64)d << 32 | c;
  u64 w;
  switch (op) {
    case 0: return {a * b, 0, false};                          // v_mul_lo_u32
    case 1: return {(u32)(((u64)a * b) >> 32), 0, false};      // v_mul_hi_u32
    case 2:                                                    // v_mul_hi_i32
      return {(u32)(((i64)(int)a * (i64)(int)b) >> 32), 0, false};
    case 3: w = (u64)a * b + y; break;                         // v_mad_u64_u32
    case 4: w = x + y; break;                                  // carry chain
    case 5: w = x - y; break;                                  // borrow chain
    case 6:                                                    // 32-bit shifts
      return {a << (b & 31u), (u32)((int)c >> (b & 31u)), true};
    case 7: {                                                  // 64-bit shifts
      const u32 e = valu_draw(base, kValuInt, step, 4, lane);
      w = (x >> (e & 63u)) ^ (y << ((e >> 8) & 63u));
      break;
    }
    case 8:                                                    // v_alignbit_b32
      return {(u32)(((u64)a << 32 | b) >> (c & 31u)), 0, false};
    case 9: return {valu_bfe(a, b & 31u, c & 31u), 0, false};  // v_bfe_u32
    case 10: return {(u32)__builtin_popcount(a) + b, 0, false};  // v_bcnt_u32_b32
    case 11: return {a ? (u32)__builtin_clz(a) : 32u, 0, false};  // v_ffbh_u32
    case 12: return {valu_perm(a, b, c & 0x07070707u), 0, false};  // v_perm_b32
    case 13: return {valu_sad_u8(a, b, c), 0, false};          // v_sad_u8
    case 14:                                                   // min / max
      return {(a < b ? a : b) + (c > d ? c : d),
              (u32)((int)a < (int)b ? a : b) + (u32)((int)c > (int)d ? c : d), true};
    default: return {(a & b) | (~a & c), 0, false};            // v_bfi_b32
  }
  return {(u32)w, (u32)(w >> 32), true};
}

BURNIN_FN ValuResult valu_f32_step(u32 base, u32 step, u32 op, u32 lane) {
  BURNIN_FP_STRICT
  const float a = valu_f32(valu_draw(base, kValuF32, step, 0, lane));
  const float b = valu_f32(valu_draw(base, kValuF32, step, 1, lane));
  const float c = valu_f32(valu_draw(base, kValuF32, step, 2, lane));
  float r;
  switch (op) {
    case 0: r = __builtin_fmaf(a, b, c); break;
    case 1: r = a * b; break;
    case 2: r = a + b; break;
    case 3: r = a - b; break;
    case 4: return {(u32)(int)(a * b), 0, false};  // |a*b| < 2^16; toward zero
    case 5:                                        // i32 to f32, RNE
      return {__builtin_bit_cast(
                  u32, (float)(int)valu_draw(base, kValuF32, step, 3, lane)),
              0, false};
    case 6:  // f32 to f16, RNE
#ifdef __HIP_DEVICE_COMPILE__
      return {(u32)__builtin_bit_cast(unsigned short, (_Float16)a), 0, false};
#else
      return {f16_bits_from_double((double)a), 0, false};
#endif
    default: {  // a multiply and an add that stay two roundings
      const float p = a * b;
      r = p + c;
      break;
    }
  }
  return {__builtin_bit_cast(u32, r), 0, false};
}

BURNIN_FN ValuResult valu_f64_step(u32 base, u32 step, u32 op, u32 lane) {
  BURNIN_FP_STRICT
  const double a = valu_f64(valu_draw(base, kValuF64, step, 0, lane),
                            valu_draw(base, kValuF64, step, 1, lane));
  const double b = valu_f64(valu_draw(base, kValuF64, step, 2, lane),
                            valu_draw(base, kValuF64, step, 3, lane));
  const double c = valu_f64(valu_draw(base, kValuF64, step, 4, lane),
                            valu_draw(base, kValuF64, step, 5, lane));
  double r;
  switch (op) {
    case 0: r = __builtin_fma(a, b, c); break;
    case 1: r = a * b; break;
    case 2: r = a + b; break;
    default: r = a - b; break;
  }
  const u64 w = __builtin_bit_cast(u64, r);
  return {(u32)w, (u32)(w >> 32), true};
}

// One half of a packed fp16 result, the host's way: exact in double
// (valu_pk16_double_exact), then one rounding.
BURNIN_FN u32 valu_f16_fma_twin(u32 a, u32 b, u32 c) {
  return f16_bits_from_double(f16_bits_to_double(a) * f16_bits_to_double(b) +
                              f16_bits_to_double(c));
}

// pk16: v_pk_fma_f16, v_pk_mul_f16, v_pk_add_f16 on two halves per lane, and
// v_pk_fma_f32 on two floats. Packed fp16 keeps denormals here (hipcc's
// default mode on gfx950; profiles/valu_check.md has the observation), so the
// addend's sign is left random and cancellations do reach the subnormal range.
BURNIN_FN ValuResult valu_pk16_step(u32 base, u32 step, u32 op, u32 lane) {
  BURNIN_FP_STRICT
  const u32 ua = valu_draw(base, kValuPk16, step, 0, lane);
  const u32 ub = valu_draw(base, kValuPk16, step, 1, lane);
  const u32 uc = valu_draw(base, kValuPk16, step, 2, lane);
  if (op == 3) {
    const u32 ud = valu_draw(base, kValuPk16, step, 3, lane);
    const u32 ue = valu_draw(base, kValuPk16, step, 4, lane);
    const u32 uf = valu_draw(base, kValuPk16, step, 5, lane);
#ifdef __HIP_DEVICE_COMPILE__
    using f32x2 = __attribute__((ext_vector_type(2))) float;
    const f32x2 a = {valu_f32(ua), valu_f32(ud)}, b = {valu_f32(ub), valu_f32(ue)},
                c = {valu_f32(uc), valu_f32(uf)};
    const f32x2 r = __builtin_elementwise_fma(a, b, c);
    const float r0 = r[0], r1 = r[1];
#else
    const float r0 = __builtin_fmaf(valu_f32(ua), valu_f32(ub), valu_f32(uc));
    const float r1 = __builtin_fmaf(valu_f32(ud), valu_f32(ue), valu_f32(uf));
#endif
    return {__builtin_bit_cast(u32, r0), __builtin_bit_cast(u32, r1), true};
  }
  const u32 a = valu_pk16(ua), b = valu_pk16(ub), c = valu_pk16(uc);
#ifdef __HIP_DEVICE_COMPILE__
  using f16x2 = __attribute__((ext_vector_type(2))) _Float16;
  const f16x2 ha = __builtin_bit_cast(f16x2, a), hb = __builtin_bit_cast(f16x2, b),
              hc = __builtin_bit_cast(f16x2, c);
  const f16x2 r = op == 0 ? __builtin_elementwise_fma(ha, hb, hc)
                  : op == 1 ? ha * hb
                            : ha + hc;
  return {__builtin_bit_cast(u32, r), 0, false};
#else
  // mul as a*b + 0 and add as a*1 + c: the same single rounding
  constexpr u32 kOne = 0x3C00u;
  u32 r = 0;
  for (u32 h = 0; h < 2; ++h) {
    const u32 x = (a >> (16u * h)) & 0xFFFFu, y = (b >> (16u * h)) & 0xFFFFu,
              z = (c >> (16u * h)) & 0xFFFFu;
    r |= (op == 0 ? valu_f16_fma_twin(x, y, z)
          : op == 1 ? valu_f16_fma_twin(x, y, 0u)
                    : valu_f16_fma_twin(x, kOne, z))
         << (16u * h);
  }
  return {r, 0, false};
#endif
}

// trans: the argument of operation op for draw u. exp2 over [-16, 16), log2
// over [2, 2^24) (away from the cancellation at 1), rcp, rsq and sqrt over
// [2^-20, 2^20).
BURNIN_FN float valu_trans_arg(u32 op, u32 u) {
  if (op == 0) return (float)((int)(u >> 8) - (1 << 23)) * (1.0f / 524288.0f);
  const u32 field = op == 1 ? 128u + ((u >> 23) & 0xFFu) % 23u
                            : 107u + ((u >> 23) & 0xFFu) % 40u;
  return __builtin_bit_cast(float, (u & 0x007FFFFFu) | field << 23);
}

#ifdef __HIPCC__
// The hardware's own approximations: no host twin, the bits are the chip's.
__device__ __forceinline__ ValuResult valu_trans_step(u32 base, u32 step, u32 op,
                                                      u32 lane) {
  const float x = valu_trans_arg(op, valu_draw(base, kValuTrans, step, 0, lane));
  float r;
  switch (op) {
    case 0: r = __builtin_amdgcn_exp2f(x); break;   // v_exp_f32
    case 1: r = __builtin_amdgcn_logf(x); break;    // v_log_f32
    case 2: r = __builtin_amdgcn_rcpf(x); break;    // v_rcp_f32
    case 3: r = __builtin_amdgcn_rsqf(x); break;    // v_rsq_f32
    default: r = __builtin_amdgcn_sqrtf(x); break;  // v_sqrt_f32
  }
  return {__builtin_bit_cast(u32, r), 0, false};
}
#endif

// Step `step` of a test; op must be step % kValuOps[TEST] (an argument, so
// that a caller which unrolls by kValuOps makes it a constant).
template <int TEST>
BURNIN_FN ValuResult valu_step(u32 base, u32 step, u32 op, u32 lane) {
  if constexpr (TEST == kValuInt) return valu_int_step(base, step, op, lane);
  else if constexpr (TEST == kValuF32) return valu_f32_step(base, step, op, lane);
  else if constexpr (TEST == kValuF64) return valu_f64_step(base, step, op, lane);
  else if constexpr (TEST == kValuPk16) return valu_pk16_step(base, step, op, lane);
#ifdef __HIPCC__
  else return valu_trans_step(base, step, op, lane);  // device code only
#else
  else {
    static_assert(TEST != kValuTrans, "trans has no host twin");
  }
#endif
}

// All steps of one (test, round) for one lane, in order, each handed to
// sink(step, result): the one loop behind the digests, the host table and
// the raw values.
template <int TEST, typename Sink>
BURNIN_FN void valu_round(u32 base, u32 lane, Sink&& sink) {
  constexpr u32 kOps = kValuOps[TEST];
  for (u32 s0 = 0; s0 < kValuSteps; s0 += kOps) {
    BURNIN_UNROLL
    for (u32 op = 0; op < kOps; ++op)
      if (s0 + op < kValuSteps) sink(s0 + op, valu_step<TEST>(base, s0 + op, op, lane));
  }
}

// A lane's answer for (test, round): one u32.
template <int TEST>
BURNIN_FN u32 valu_digest(u32 base, u32 lane) {
  u32 d = 0;
  valu_round<TEST>(base, lane, [&](u32, const ValuResult& r) { d = valu_fold(d, r); });
  return d;
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
