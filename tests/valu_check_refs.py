"""Independent reference of the per-SIMD vector ALU check (csrc/valu_check.hip,
VALU section of csrc/burnin_core.h).

The generator is written again here in numpy. Results come from exact
arithmetic: every float is decoded to an integer times a power of two, the
operation is done on Python ints, and the exact result is rounded once, to
nearest even, by round_to_format (which handles subnormals and overflow). No
f32 operation goes through float64: that would round twice. Integer
operations are written from the instructions' definitions. trans has no exact
reference: numpy's float64 functions, for a wiring check within a few ULP.
"""
from functools import lru_cache

import numpy as np

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
GOLDEN = 0x9E3779B9
STEPS = 256
TESTS = ("int", "f32", "f64", "pk16", "trans")
EXACT_TESTS = TESTS[:4]
TEST_INDEX = {t: i for i, t in enumerate(TESTS)}
OPS = {"int": 16, "f32": 8, "f64": 4, "pk16": 4, "trans": 5}
TRANS_FUNCS = ("exp2", "log2", "rcp", "rsq", "sqrt")
# exponent-field windows of the float operands, inclusive
WINDOWS = {"f32": (120, 134), "f64": (1016, 1030), "f16": (11, 19)}
# (exponent bits, mantissa bits)
FORMATS = {"f16": (5, 10), "f32": (8, 23), "f64": (11, 52)}
# rounds (seed 0) in which a packed fp16 fma cancels into the subnormal range
PK16_SUBNORMAL_ROUNDS = (2, 3, 120)


def fmix32(h: int) -> int:
    h &= M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def fmix32_np(h: np.ndarray) -> np.ndarray:
    h = h.astype(np.uint64) & np.uint64(M32)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(M32)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & np.uint64(M32)
    h ^= h >> np.uint64(16)
    return h


def key_base(seed: int, key: int) -> int:
    return fmix32((seed & M32) + key * GOLDEN) ^ (seed >> 32) & M32


def draws(test: str, rnd: int, seed: int, operand: int) -> list:
    """u[step][lane] as Python ints."""
    step = np.arange(STEPS, dtype=np.uint64)[:, None]
    lane = np.arange(64, dtype=np.uint64)[None, :]
    tag = (np.uint64(TEST_INDEX[test] << 28 | operand << 8) | step << np.uint64(12) | lane)
    return fmix32_np(np.uint64(key_base(seed, rnd)) ^ tag).tolist()


# ---------------------------------------------------------------------------
# exact floats
# ---------------------------------------------------------------------------

def decode(bits: int, fmt: str):
    """A finite float as (n, e): the value is n * 2**e, n a signed int."""
    ebits, mbits = FORMATS[fmt]
    bias = (1 << (ebits - 1)) - 1
    field = (bits >> mbits) & ((1 << ebits) - 1)
    mant = bits & ((1 << mbits) - 1)
    assert field != (1 << ebits) - 1, "not finite"
    n = mant if field == 0 else mant | 1 << mbits
    e = (1 if field == 0 else field) - bias - mbits
    return (-n if bits >> (ebits + mbits) else n), e


def round_to_format(n: int, e: int, fmt: str) -> int:
    """The bits of n * 2**e rounded once to fmt, round-to-nearest-even, with
    subnormal results and overflow to infinity. An exact zero is +0 (what
    round-to-nearest gives a cancellation)."""
    ebits, mbits = FORMATS[fmt]
    if n == 0:
        return 0
    sign, n = (1, -n) if n < 0 else (0, n)
    emin = 2 - (1 << (ebits - 1))  # exponent of the smallest normal
    top = n.bit_length() - 1 + e  # floor(log2(value))
    ulp = max(top, emin) - mbits  # exponent of the result's last place
    shift = ulp - e
    if shift <= 0:
        q = n << -shift
    else:
        q, rem = n >> shift, n & ((1 << shift) - 1)
        half = 1 << (shift - 1)
        if rem > half or (rem == half and q & 1):
            q += 1
    # a normal q holds its leading one, which counts 1 into the exponent field
    bits = ((max(top, emin) - emin) << mbits) + q
    inf = ((1 << ebits) - 1) << mbits
    return sign << (ebits + mbits) | min(bits, inf)


def fma_exact(a, b, c, fmt: str) -> int:
    """round(a*b + c) for decoded a, b, c."""
    (na, ea), (nb, eb), (nc, ec) = a, b, c
    e = min(ea + eb, ec)
    return round_to_format((na * nb << (ea + eb - e)) + (nc << (ec - e)), e, fmt)


def mul_exact(a, b, fmt: str) -> int:
    return round_to_format(a[0] * b[0], a[1] + b[1], fmt)


def add_exact(a, b, fmt: str, sub: bool = False) -> int:
    (na, ea), (nb, eb) = a, b
    e = min(ea, eb)
    return round_to_format((na << (ea - e)) + ((-nb if sub else nb) << (eb - e)), e, fmt)


def windowed(sign_mant: int, field_draw: int, fmt: str, window: str = None) -> int:
    """Bits whose sign and mantissa are sign_mant's and whose exponent field
    is forced into the window."""
    ebits, mbits = FORMATS[fmt]
    lo, hi = WINDOWS[window or fmt]
    keep = 1 << (ebits + mbits) | ((1 << mbits) - 1)
    return (sign_mant & keep) | (lo + field_draw % (hi - lo + 1)) << mbits


def f32_operand(u: int) -> int:
    return windowed(u, (u >> 23) & 0xFF, "f32")


def f64_operand(hi: int, lo: int) -> int:
    return windowed(hi << 32 | lo, (hi >> 20) & 0x7FF, "f64")


def f16_operand(h: int) -> int:
    return windowed(h & 0xFFFF, (h >> 10) & 31, "f16")


# ---------------------------------------------------------------------------
# the five tests: result(step, lane) -> (lo, hi or None)
# ---------------------------------------------------------------------------

def _s32(x: int) -> int:
    return x - (1 << 32) if x & 0x80000000 else x


def int_result(op: int, a: int, b: int, c: int, d: int, e: int):
    x, y = b << 32 | a, d << 32 | c
    wide = lambda w: (w & M32, (w >> 32) & M32)  # noqa: E731
    if op == 0:
        return (a * b) & M32, None
    if op == 1:
        return (a * b) >> 32, None
    if op == 2:
        return ((_s32(a) * _s32(b)) >> 32) & M32, None
    if op == 3:
        return wide(a * b + y)
    if op == 4:
        return wide(x + y)
    if op == 5:
        return wide(x - y)
    if op == 6:
        return (a << (b & 31)) & M32, (_s32(c) >> (b & 31)) & M32
    if op == 7:
        return wide((x >> (e & 63)) ^ (y << ((e >> 8) & 63)))
    if op == 8:  # alignbit: {a, b} shifted right, low word
        return ((a << 32 | b) >> (c & 31)) & M32, None
    if op == 9:  # bfe: width bits from offset
        return (a >> (b & 31)) & ((1 << (c & 31)) - 1), None
    if op == 10:
        return (bin(a).count("1") + b) & M32, None
    if op == 11:
        return 32 - a.bit_length(), None
    if op == 12:  # perm: bytes 0..3 are b's, 4..7 are a's
        src = b.to_bytes(4, "little") + a.to_bytes(4, "little")
        return int.from_bytes(bytes(src[(c >> 8 * i) & 7] for i in range(4)), "little"), None
    if op == 13:  # sad_u8
        return (c + sum(abs(p - q) for p, q in zip(a.to_bytes(4, "little"), b.to_bytes(4, "little")))) & M32, None
    if op == 14:
        lo = (min(a, b) + max(c, d)) & M32
        hi = (min(_s32(a), _s32(b)) + max(_s32(c), _s32(d))) & M32
        return lo, hi
    return (a & b) | (~a & c & M32), None


def f32_result(op: int, ua: int, ub: int, uc: int, ud: int):
    a, b, c = (decode(f32_operand(u), "f32") for u in (ua, ub, uc))
    if op == 0:
        return fma_exact(a, b, c, "f32")
    if op == 1:
        return mul_exact(a, b, "f32")
    if op == 2:
        return add_exact(a, b, "f32")
    if op == 3:
        return add_exact(a, b, "f32", sub=True)
    if op == 4:  # the rounded product, truncated toward zero
        n, e = decode(mul_exact(a, b, "f32"), "f32")
        mag = abs(n) << e if e >= 0 else abs(n) >> -e
        return (-mag if n < 0 else mag) & M32
    if op == 5:
        return round_to_format(_s32(ud), 0, "f32")
    if op == 6:
        return round_to_format(a[0], a[1], "f16")
    return add_exact(decode(mul_exact(a, b, "f32"), "f32"), c, "f32")  # two roundings


def f64_result(op: int, u: list):
    a, b, c = (decode(f64_operand(u[2 * i], u[2 * i + 1]), "f64") for i in range(3))
    if op == 0:
        return fma_exact(a, b, c, "f64")
    if op == 1:
        return mul_exact(a, b, "f64")
    return add_exact(a, b, "f64", sub=(op == 3))


def pk16_result(op: int, u: list):
    if op == 3:  # two f32 fmas: (u0, u1, u2) and (u3, u4, u5)
        r = [fma_exact(*(decode(f32_operand(x), "f32") for x in u[3 * i:3 * i + 3]), "f32")
             for i in range(2)]
        return r[0], r[1]
    out = 0
    for h in range(2):
        a, b, c = (decode(f16_operand((x >> 16 * h) & 0xFFFF), "f16") for x in u[:3])
        r = fma_exact(a, b, c, "f16") if op == 0 else mul_exact(a, b, "f16") if op == 1 \
            else add_exact(a, c, "f16")
        out |= r << 16 * h
    return out, None


@lru_cache(maxsize=None)
def values(test: str, rnd: int, seed: int) -> np.ndarray:
    """Raw result bits [STEPS][64] of an exact test as uint64, a 64-bit
    result as hi << 32 | lo. Read-only."""
    n_draws = {"int": 5, "f32": 4, "f64": 6, "pk16": 6}[test]
    u = [draws(test, rnd, seed, k) for k in range(n_draws)]
    out = np.zeros((STEPS, 64), dtype=np.uint64)
    for step in range(STEPS):
        op = step % OPS[test]
        for lane in range(64):
            d = [u[k][step][lane] for k in range(n_draws)]
            if test == "int":
                lo, hi = int_result(op, *d)
            elif test == "f32":
                lo, hi = f32_result(op, *d), None
            elif test == "f64":
                w = f64_result(op, d)
                lo, hi = w & M32, w >> 32
            else:
                lo, hi = pk16_result(op, d)
            assert 0 <= lo <= M32 and (hi is None or 0 <= hi <= M32)
            out[step, lane] = (hi or 0) << 32 | lo
    out.setflags(write=False)
    return out


def is_wide(test: str, op: int) -> bool:
    """Whether the operation's result has 64 bits (both words are folded)."""
    return {"int": op in (3, 4, 5, 6, 7, 14), "f64": True, "pk16": op == 3}.get(test, False)


def digests_of(test: str, vals: np.ndarray) -> np.ndarray:
    """The 64 digests of a [STEPS][64] array of result bits."""
    rows = vals.tolist()
    out = np.zeros(64, dtype=np.uint64)
    for lane in range(64):
        d = 0
        for step in range(STEPS):
            w = rows[step][lane]
            d = fmix32(d ^ (w & M32))
            if is_wide(test, step % OPS[test]):
                d = fmix32(d ^ (w >> 32))
        out[lane] = d
    return out


@lru_cache(maxsize=None)
def digests(test: str, rnd: int, seed: int) -> np.ndarray:
    out = digests_of(test, values(test, rnd, seed))
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------------------
# trans
# ---------------------------------------------------------------------------

def trans_args(rnd: int, seed: int) -> np.ndarray:
    """The float32 arguments [STEPS][64]; step s runs TRANS_FUNCS[s % 5]."""
    u = np.array(draws("trans", rnd, seed, 0), dtype=np.uint64)
    op = (np.arange(STEPS) % 5)[:, None]
    e = (u >> np.uint64(23)) & np.uint64(0xFF)
    field = np.where(op == 1, 128 + e % np.uint64(23), 107 + e % np.uint64(40)).astype(np.uint64)
    bits = ((u & np.uint64(0x7FFFFF)) | field << np.uint64(23)).astype(np.uint32)
    x = bits.view(np.float32)
    lin = ((u >> np.uint64(8)).astype(np.int64) - (1 << 23)).astype(np.float64) / 524288.0
    return np.where(op == 0, lin.astype(np.float32), x).astype(np.float32)


def trans_reference(rnd: int, seed: int) -> np.ndarray:
    """float64 results [STEPS][64] of numpy's functions on the f32 arguments."""
    x = trans_args(rnd, seed).astype(np.float64)
    op = (np.arange(STEPS) % 5)[:, None]
    with np.errstate(all="ignore"):
        return np.select(
            [op == 0, op == 1, op == 2, op == 3, op == 4],
            [np.exp2(x), np.log2(np.abs(x)), 1.0 / x, 1.0 / np.sqrt(np.abs(x)), np.sqrt(np.abs(x))])


def ulp_distance(got_bits: np.ndarray, ref: np.ndarray) -> np.ndarray:
    """|got - ref| in units of the last place of the fp32 result."""
    got = got_bits.astype(np.uint32).view(np.float32).astype(np.float64)
    return np.abs(got - ref) / np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
