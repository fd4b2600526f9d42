// Stand-alone driver of csrc/burnin_core.h on the CPU: no GPU, no Python.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-omit-frame-pointer
//       csrc/burnin_selftest.cpp -o /tmp/burnin_selftest && /tmp/burnin_selftest
//
// With no argument it runs the checks that need no outside oracle and prints
// "burnin selftest OK" (exit status 0 = clean):
//
//   * every code elem_code can draw, decoded with the bit decoders below
//     (written from the format definitions), equals elem_int times the
//     granule, for every format, legal range and residue of the draw, and the
//     set of codes has the stated size;
//   * the exactness condition accepts the largest K with top^2 * K <= 2^24 at
//     each format's full range and rejects K + 1;
//   * pattern_pair with tile_terms equals two pattern_word calls for tiles
//     that cross no multiple of 2^32, that cross one and that start on one;
//   * the VALU section: the exponent windows, fp16 rounding at ties, at the
//     subnormal boundary and at the largest finite value, the condition
//     under which the packed-fp16 twin is exact in double, the twins of the
//     device builtins, and that a multiply and an add stayed two roundings.
//
// With a sub-command it prints raw values, one number per token, for
// tests/test_burnin_core_cpu.py to compare with the numpy references:
//
//   cu <fmt> <tile> <seed> <operand>                  codes, then numerators, [16][K]
//   gemm <kind> <operand> <rows> <K> <seed> <range>   codes, then numerators, [rows][K]
//   mem <pattern> <seed> <base_word> <n> <invert>     n words
//   exact <kind> <range> <K>                          1 if the sums are exact, else 0
//   valu <test> <round> <seed>                        steps*64 result bits, then 64 digests
//
// fmt and kind are bf16, fp8 or fp4; pattern is addr, rand or zero; test is
// int, f32, f64 or pk16 (trans has no host twin). The tag
// layouts and cu_check's K are the checks' own definitions (cu_check.hip,
// gemm_check.hip) and are written out again here.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "burnin_core.h"

using namespace burnin;

static int g_failed = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      if (++g_failed <= 20)                                                \
        std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                                      \
  } while (0)

// ---------------------------------------------------------------------------
// Bit decoders, from the format definitions
// ---------------------------------------------------------------------------

// bf16: 1 sign, 8 exponent (bias 127), 7 mantissa bits.
static double decode_bf16(u32 bits) {
  const int s = (bits >> 15) & 1, e = (bits >> 7) & 0xFF, m = bits & 0x7F;
  const double mag = e == 0 ? std::ldexp(m / 128.0, -126) : std::ldexp(1.0 + m / 128.0, e - 127);
  return s ? -mag : mag;
}

// e4m3: 1 sign, 4 exponent (bias 7), 3 mantissa bits.
static double decode_e4m3(u32 code) {
  const int s = (code >> 7) & 1, e = (code >> 3) & 0xF, m = code & 7;
  const double mag = e == 0 ? std::ldexp(m / 8.0, -6) : std::ldexp(1.0 + m / 8.0, e - 7);
  return s ? -mag : mag;
}

// e2m1: 1 sign, 2 exponent (bias 1), 1 mantissa bit.
static double decode_e2m1(u32 code) {
  const int s = (code >> 3) & 1, e = (code >> 1) & 3, m = code & 1;
  const double mag = e == 0 ? m / 2.0 : std::ldexp(1.0 + m / 2.0, e - 1);
  return s ? -mag : mag;
}

static double decode(int fmt, u32 code) {
  return fmt == kBf16 ? decode_bf16(code) : fmt == kFp8 ? decode_e4m3(code) : decode_e2m1(code);
}

// ---------------------------------------------------------------------------
// Bare run
// ---------------------------------------------------------------------------

// How many residues the draw of a format has at a range.
static u32 residues(int fmt, u32 range) {
  return fmt == kBf16 ? 2 * range + 1 : fmt == kFp8 ? 16 * range + 1 : 16;
}

template <int FMT>
static void check_codes() {
  for (u32 range = kMinRange[FMT]; range <= kFullRange[FMT]; ++range) {
    const u32 n = residues(FMT, range);
    std::set<u32> seen;
    i64 top = 0;
    for (u32 j = 0; j < n; ++j) {
      // the residue itself and a large draw with the same residue
      const u32 draws[2] = {j, j + n * (0xFFFFFFFFu / n - 1)};
      for (u32 u : draws) {
        const u32 code = elem_code<FMT>(u, range);
        const int num = elem_int<FMT>(u, range);
        CHECK(decode(FMT, code) == num / (double)kInvOperandGranule[FMT]);
        CHECK(code < (1u << kElemBits[FMT]));
        if (range == kFullRange[FMT]) {  // the compile-time form cu_check uses
          CHECK((elem_code<FMT, kFullRange[FMT]>(u)) == code);
          CHECK((elem_int<FMT, kFullRange[FMT]>(u)) == num);
        }
        seen.insert(code);
        top = std::max<i64>(top, std::abs(num));
      }
    }
    CHECK(seen.size() == n);
    CHECK(top == max_numerator(FMT, range));
  }
}

static void check_exactness() {
  for (int fmt = 0; fmt < kNumFormats; ++fmt) {
    const i64 top = max_numerator(fmt, kFullRange[fmt]);
    const i64 K = kTwo24 / (top * top);  // the largest K with top^2 * K <= 2^24
    CHECK(top * top * K <= kTwo24 && top * top * (K + 1) > kTwo24);
    CHECK(sums_exact(fmt, kFullRange[fmt], K));
    CHECK(!sums_exact(fmt, kFullRange[fmt], K + 1));
  }
  CHECK(max_numerator(kBf16, 127) == 127 && max_numerator(kFp8, 4) == 120 &&
        max_numerator(kFp4, 16) == 12);
}

template <int PAT>
static void check_pairs(u64 g_first, u64 nwords, bool uniform) {
  const u64 seeds[2] = {0x0123456789ABCDEFull, 0xFFFFFFFF00000001ull};
  for (u64 seed : seeds) {
    for (u64 inv : {0ull, ~0ull}) {
      const HiTerms t = tile_terms(g_first, nwords, seed);
      CHECK(t.uniform == uniform);
      for (u64 i = 0; i + 1 < nwords; i += 2) {
        const u64 g0 = g_first + i;
        u64 w0 = 0, w1 = 0;
        pattern_pair<PAT>(g0, seed, inv, t, w0, w1);
        CHECK(w0 == pattern_word<PAT>(g0, seed, inv));
        CHECK(w1 == pattern_word<PAT>(g0 + 1, seed, inv));
      }
    }
  }
}

static void check_patterns() {
  const u64 two32 = 1ull << 32, n = 2048;  // a memtest tile is 2048 words
  struct Tile {
    u64 g_first;
    bool uniform;
  };
  const Tile tiles[] = {
      {0, true},                    // crosses nothing
      {7, true},                    // odd start
      {two32 - n, true},            // ends on the last word before 2^32
      {5 * two32 + 4096, true},     // upper half in use
      {two32 - n / 2, false},       // crosses 2^32 in the middle
      {two32 - 1, false},           // crosses after its first word
      {3 * two32 - 1023, false},    // odd start, crosses 3 * 2^32
      {two32, true},                // starts exactly on 2^32
      {(1ull << 40), true},         // and on a higher multiple
  };
  for (const Tile& t : tiles) {
    check_pairs<kAddr>(t.g_first, n, t.uniform);
    check_pairs<kRand>(t.g_first, n, t.uniform);
    check_pairs<kZero>(t.g_first, n, t.uniform);
  }
}

// The VALU section: window constants, fp16 rounding where it can go wrong,
// the double-exactness condition and the host twins of the device builtins.
static void check_valu() {
  // windows: every operand normal, magnitudes in [2^-7, 2^8) / [2^-4, 2^5)
  CHECK(kValuF32ExpLo == 120 && kValuF32ExpHi == 134);
  CHECK(kValuF64ExpLo == 1016 && kValuF64ExpHi == 1030);
  CHECK(kValuF16ExpLo == 11 && kValuF16ExpHi == 19);
  CHECK(kValuSteps == 256 && kNumValuExact + 1 == kNumValuTests);
  u32 f32_fields = 0, f64_fields = 0, f16_fields = 0;
  for (u32 i = 0; i < 4096; ++i) {
    const u32 u = fmix32(i), v = fmix32(~i);
    const float f = valu_f32(u);
    const u32 fb = __builtin_bit_cast(u32, f), fe = (fb >> 23) & 0xFFu;
    CHECK(fe >= kValuF32ExpLo && fe <= kValuF32ExpHi && ((fb ^ u) & 0x807FFFFFu) == 0);
    CHECK(std::fabs(f) >= std::ldexp(1.0, -7) && std::fabs(f) < std::ldexp(1.0, 8));
    f32_fields |= 1u << (fe - kValuF32ExpLo);
    const double d = valu_f64(u, v);
    const u64 db = __builtin_bit_cast(u64, d);
    const u32 de = (u32)(db >> 52) & 0x7FFu;
    CHECK(de >= kValuF64ExpLo && de <= kValuF64ExpHi && (u32)db == v);
    CHECK(((u32)(db >> 32) ^ u) << 12 == 0 && (db >> 63) == (u >> 31));
    f64_fields |= 1u << (de - kValuF64ExpLo);
    const u32 h = valu_f16(u), he = (h >> 10) & 31u;
    CHECK(h < 0x10000u && he >= kValuF16ExpLo && he <= kValuF16ExpHi);
    CHECK(((h ^ u) & 0x83FFu) == 0);
    f16_fields |= 1u << (he - kValuF16ExpLo);
    CHECK(valu_pk16(u) == (valu_f16(u & 0xFFFFu) | valu_f16(u >> 16) << 16));
  }
  CHECK(f32_fields == 0x7FFFu && f64_fields == 0x7FFFu && f16_fields == 0x1FFu);

  // the double twin is exact: bits 2^-28 .. 2^10 at this window, 39 of them,
  // and 53 is the limit
  CHECK(valu_pk16_span_bits(kValuF16ExpLo, kValuF16ExpHi) == 39);
  CHECK(valu_pk16_double_exact(kValuF16ExpLo, kValuF16ExpHi));
  CHECK(valu_pk16_double_exact(4, 19) && !valu_pk16_double_exact(3, 19));

  // fp16 decode and round trip of every finite code
  for (u32 h = 0; h < 0x10000u; ++h) {
    if (((h >> 10) & 31u) == 31u) continue;
    const u32 e = (h >> 10) & 31u, m = h & 0x3FFu;
    const double mag = e == 0 ? std::ldexp(m / 1024.0, -14) : std::ldexp(1.0 + m / 1024.0, (int)e - 15);
    CHECK(f16_bits_to_double(h) == ((h & 0x8000u) ? -mag : mag));
    CHECK(f16_bits_from_double(f16_bits_to_double(h)) == h);
  }
  // ties to even, and just beside the tie
  CHECK(f16_bits_from_double(1.0 + std::ldexp(1.0, -11)) == 0x3C00u);  // tie, even below
  CHECK(f16_bits_from_double(1.0 + std::ldexp(3.0, -11)) == 0x3C02u);  // tie, even above
  CHECK(f16_bits_from_double(1.0 + std::ldexp(1.0, -11) + std::ldexp(1.0, -40)) == 0x3C01u);
  CHECK(f16_bits_from_double(1.0 + std::ldexp(1.0, -11) - std::ldexp(1.0, -40)) == 0x3C00u);
  CHECK(f16_bits_from_double(-(1.0 + std::ldexp(3.0, -11))) == 0xBC02u);
  // the subnormal boundary
  CHECK(f16_bits_from_double(std::ldexp(1.0, -14)) == 0x0400u);   // smallest normal
  CHECK(f16_bits_from_double(std::ldexp(1023.0, -24)) == 0x03FFu);  // largest subnormal
  CHECK(f16_bits_from_double(std::ldexp(1023.5, -24)) == 0x0400u);  // tie up to normal
  CHECK(f16_bits_from_double(std::ldexp(1022.5, -24)) == 0x03FEu);  // tie to even
  CHECK(f16_bits_from_double(std::ldexp(1.0, -24)) == 0x0001u);   // smallest subnormal
  CHECK(f16_bits_from_double(std::ldexp(1.0, -25)) == 0x0000u);   // tie to zero
  CHECK(f16_bits_from_double(std::ldexp(1.0, -25) + std::ldexp(1.0, -60)) == 0x0001u);
  CHECK(f16_bits_from_double(std::ldexp(1.5, -24)) == 0x0002u);   // tie to even
  CHECK(f16_bits_from_double(-std::ldexp(1.0, -28)) == 0x8000u);  // the lowest product bit
  CHECK(f16_bits_from_double(0.0) == 0x0000u && f16_bits_from_double(-0.0) == 0x8000u);
  // the largest finite value
  CHECK(f16_bits_from_double(65504.0) == 0x7BFFu);
  CHECK(f16_bits_from_double(65519.99) == 0x7BFFu);
  CHECK(f16_bits_from_double(65520.0) == 0x7C00u);  // tie: even is 2^16
  CHECK(f16_bits_from_double(-1e30) == 0xFC00u);
  // a cancelling fma lands in the subnormal range: 1.5*1.5 - 2.25 = 0, and
  // (1 + 2^-10) * (1/16 + 2^-14) - (1/16 + 2^-13) = 2^-24, the smallest subnormal
  CHECK(valu_f16_fma_twin(0x3E00u, 0x3E00u, 0xC080u) == 0x0000u);
  CHECK(valu_f16_fma_twin(0x3C01u, 0x2C01u, 0xAC02u) == 0x0001u);

  // the twins of the device builtins, by hand
  CHECK(valu_perm_twin(0xAABBCCDDu, 0x11223344u, 0x00010203u) == 0x44332211u);
  CHECK(valu_perm_twin(0xAABBCCDDu, 0x11223344u, 0x07060504u) == 0xAABBCCDDu);
  CHECK(valu_perm_twin(0xAABBCCDDu, 0x11223344u, 0x04000703u) == 0xDD44AA11u);
  CHECK(valu_sad_u8_twin(0x01FF0010u, 0xFF0100F0u, 5u) == 5u + 254u + 254u + 0u + 224u);
  CHECK(valu_sad_u8_twin(0u, 0xFFFFFFFFu, 0xFFFFFFFFu) == 4u * 255u - 1u);
  CHECK(valu_bfe_twin(0xDEADBEEFu, 8, 12) == 0xDBEu && valu_bfe_twin(0xDEADBEEFu, 28, 8) == 0xDu);
  CHECK(valu_bfe_twin(0xDEADBEEFu, 0, 0) == 0u && valu_bfe_twin(0xDEADBEEFu, 31, 31) == 1u);

  // a separate multiply and add stayed two roundings in this build: with
  // a = b = 1 + 2^-12 the product's 2^-24 is lost before the add, kept by fma
  {
    volatile float a = 1.0f + std::ldexp(1.0f, -12), c = -1.0f;
    const float p = a * a, two = p + c, one = __builtin_fmaf(a, a, c);
    CHECK(two == std::ldexp(1.0f, -11) && one == std::ldexp(1.0f, -11) + std::ldexp(1.0f, -24));
  }
}

// ---------------------------------------------------------------------------
// Sub-commands
// ---------------------------------------------------------------------------

// valu: the steps*64 result bits of one (test, round), [step][lane], a 64-bit
// result as hi << 32 | lo; then the 64 digests.
template <int TEST>
static void print_valu(u32 round, u64 seed) {
  const SeedHalves s = split_seed(seed);
  const u32 base = key_base(s.lo, s.hi, round);
  std::vector<u64> bits((size_t)kValuSteps * 64);
  for (u32 lane = 0; lane < 64; ++lane)
    valu_round<TEST>(base, lane, [&](u32 step, const ValuResult& r) {
      bits[(size_t)step * 64 + lane] = (u64)(r.wide ? r.hi : 0u) << 32 | r.lo;
    });
  for (u64 b : bits) std::printf("%llu\n", b);
  for (u32 lane = 0; lane < 64; ++lane) std::printf("%u\n", valu_digest<TEST>(base, lane));
}

static int parse_name(const char* s, const char* const* names, int n, const char* what) {
  for (int i = 0; i < n; ++i)
    if (std::strcmp(s, names[i]) == 0) return i;
  std::fprintf(stderr, "unknown %s '%s'\n", what, s);
  std::exit(2);
}

static u64 parse_u64(const char* s) {
  char* end = nullptr;
  const u64 v = std::strtoull(s, &end, 0);
  if (end == s || *end != '\0') {
    std::fprintf(stderr, "not a number: '%s'\n", s);
    std::exit(2);
  }
  return v;
}

// cu_check's tag: fmt<<28 | operand<<20 | row<<12 | k, keyed by the tile.
// gemm_check's tag: fmt<<28 | operand<<24 | k, keyed by the row.
template <int FMT>
static void print_operand(bool cu, u32 key, u32 operand, u32 rows, u32 K, u64 seed,
                          u32 range) {
  const SeedHalves s = split_seed(seed);
  std::vector<u32> codes((size_t)rows * K);
  std::vector<int> nums((size_t)rows * K);
  for (u32 row = 0; row < rows; ++row) {
    const u32 base = key_base(s.lo, s.hi, cu ? key : row);
    for (u32 k = 0; k < K; ++k) {
      const u32 tag = cu ? ((u32)FMT << 28 | operand << 20 | row << 12 | k)
                         : ((u32)FMT << 28 | operand << 24 | k);
      const u32 u = fmix32(base ^ tag);
      codes[(size_t)row * K + k] =
          cu ? elem_code<FMT, kFullRange[FMT]>(u) : elem_code<FMT>(u, range);
      nums[(size_t)row * K + k] =
          cu ? elem_int<FMT, kFullRange[FMT]>(u) : elem_int<FMT>(u, range);
    }
  }
  for (u32 c : codes) std::printf("%u\n", c);
  for (int v : nums) std::printf("%d\n", v);
}

static void print_operand(int fmt, bool cu, u32 key, u32 operand, u32 rows, u32 K,
                          u64 seed, u32 range) {
  if (fmt == kBf16) print_operand<kBf16>(cu, key, operand, rows, K, seed, range);
  if (fmt == kFp8) print_operand<kFp8>(cu, key, operand, rows, K, seed, range);
  if (fmt == kFp4) print_operand<kFp4>(cu, key, operand, rows, K, seed, range);
}

static bool legal_range(int fmt, u64 range) {
  return range >= kMinRange[fmt] && range <= kFullRange[fmt];
}

static int usage() {
  std::fprintf(stderr,
               "usage: burnin_selftest\n"
               "       burnin_selftest cu <fmt> <tile> <seed> <operand>\n"
               "       burnin_selftest gemm <kind> <operand> <rows> <K> <seed> <range>\n"
               "       burnin_selftest mem <pattern> <seed> <base_word> <n> <invert>\n"
               "       burnin_selftest exact <kind> <range> <K>\n"
               "       burnin_selftest valu <test> <round> <seed>\n");
  return 2;
}

int main(int argc, char** argv) {
  if (argc == 1) {
    check_codes<kBf16>();
    check_codes<kFp8>();
    check_codes<kFp4>();
    check_exactness();
    check_patterns();
    check_valu();
    if (g_failed) {
      std::fprintf(stderr, "burnin selftest: %d check(s) failed\n", g_failed);
      return 1;
    }
    std::printf("burnin selftest OK\n");
    return 0;
  }
  const std::string cmd = argv[1];
  if (cmd == "cu" && argc == 6) {
    constexpr u32 kCuK[kNumFormats] = {1024, 1152, 1280};
    const int fmt = parse_name(argv[2], kFormatNames, kNumFormats, "format");
    const u64 tile = parse_u64(argv[3]), operand = parse_u64(argv[5]);
    if (tile >= (1u << 18) || operand > 1) return usage();
    print_operand(fmt, true, (u32)tile, (u32)operand, 16, kCuK[fmt], parse_u64(argv[4]),
                  kFullRange[fmt]);
    return 0;
  }
  if (cmd == "gemm" && argc == 8) {
    const int kind = parse_name(argv[2], kFormatNames, kNumFormats, "kind");
    const u64 operand = parse_u64(argv[3]), rows = parse_u64(argv[4]), K = parse_u64(argv[5]),
              range = parse_u64(argv[7]);
    if (operand > 1 || rows < 1 || rows > (1u << 16) || K < 1 || K > (u64)kTwo24 ||
        !legal_range(kind, range))
      return usage();
    print_operand(kind, false, 0, (u32)operand, (u32)rows, (u32)K, parse_u64(argv[6]),
                  (u32)range);
    return 0;
  }
  if (cmd == "mem" && argc == 7) {
    const char* const names[3] = {"addr", "rand", "zero"};
    const int pat = parse_name(argv[2], names, 3, "pattern");
    const u64 seed = parse_u64(argv[3]), base = parse_u64(argv[4]), n = parse_u64(argv[5]);
    const u64 inv = parse_u64(argv[6]) ? ~0ull : 0ull;
    for (u64 i = 0; i < n; ++i) {
      const u64 g = base + i;
      const u64 w = pat == kAddr   ? pattern_word<kAddr>(g, seed, inv)
                    : pat == kRand ? pattern_word<kRand>(g, seed, inv)
                                   : pattern_word<kZero>(g, seed, inv);
      std::printf("%llu\n", w);
    }
    return 0;
  }
  if (cmd == "exact" && argc == 5) {
    const int kind = parse_name(argv[2], kFormatNames, kNumFormats, "kind");
    const u64 range = parse_u64(argv[3]), K = parse_u64(argv[4]);
    if (!legal_range(kind, range) || K < 1 || K > (u64)kTwo24) return usage();
    std::printf("%d\n", sums_exact(kind, (i64)range, (i64)K) ? 1 : 0);
    return 0;
  }
  if (cmd == "valu" && argc == 5) {
    const int test = parse_name(argv[2], kValuTestNames, kNumValuExact, "exact VALU test");
    const u64 round = parse_u64(argv[3]), seed = parse_u64(argv[4]);
    if (round >= 4096) return usage();
    if (test == kValuInt) print_valu<kValuInt>((u32)round, seed);
    if (test == kValuF32) print_valu<kValuF32>((u32)round, seed);
    if (test == kValuF64) print_valu<kValuF64>((u32)round, seed);
    if (test == kValuPk16) print_valu<kValuPk16>((u32)round, seed);
    return 0;
  }
  return usage();
}
