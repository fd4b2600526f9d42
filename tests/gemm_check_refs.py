"""Reference for the checked GEMM loop (csrc/gemm_check.hip), in numpy.

Written from the generator's definition, not from the kernels:

    fmix32(h): h^=h>>16; h*=0x85EBCA6B; h^=h>>13; h*=0xC2B2AE35; h^=h>>16

    u(seed, fmt, operand, row, k) =
        fmix32(fmix32(seed_lo + row*0x9E3779B9) ^ seed_hi
               ^ (fmt<<28 | operand<<24 | k))

    bf16, range r:  m = (u % (2r+1)) - r, value m/16
    e4m3, range w:  j = u % (16w+1): zero, then the codes with exponent field
                    6..6+w-1, positive before negative, ascending
    e2m1:           code u & 15

fmt is 0 / 1 / 2 for bf16 / fp8 / fp4, operand 0 for A and 1 for Bt. Decoding
goes through kernel_refs' LUTs; numerators are in units of the operand granule
(1/16, 2^-4, 1/2) and checksums in product granules (2^-8, 2^-8, 2^-2).

Plain module, not a conftest: it changes nothing about collection.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

import kernel_refs as kr
from cu_check_refs import M32, fmix32

KINDS = ("bf16", "fp8", "fp4")
FMT_INDEX = {"bf16": 0, "fp8": 1, "fp4": 2}
EXACT_SET = {"bf16": "bf16", "fp8": "e4m3", "fp4": "e2m1"}
GRANULE = {"bf16": 1.0 / 16.0, "fp8": 2.0 ** -4, "fp4": 0.5}
MIN_K = {"bf16": 192, "fp8": 256, "fp4": 512}  # the GEMM bindings' smallest K
TILE = 256
POISON_BITS = 0x7FC0DEAD
TWO24 = 1 << 24


def max_numerator(kind: str, rng: int) -> int:
    """Largest numerator magnitude of the set `rng` selects."""
    if kind == "bf16":
        return int(rng)
    if kind == "fp8":
        return 15 << (int(rng) - 1)
    return 12


def e4m3_codes_of_range(w: int) -> np.ndarray:
    """Zero, then every code with exponent field 6..6+w-1: 16w + 1 codes in
    the order the generator indexes them."""
    pos = [(6 + (t >> 3)) << 3 | (t & 7) for t in range(8 * w)]
    return np.array([0] + pos + [0x80 | c for c in pos], dtype=np.uint8)


def draws(kind: str, operand: int, rows: int, K: int, seed: int) -> np.ndarray:
    """u for every (row, k): uint64 [rows][K]."""
    seed_lo, seed_hi = seed & M32, (seed >> 32) & M32
    row = np.arange(rows, dtype=np.uint64)
    base = fmix32((np.uint64(seed_lo) + row * np.uint64(0x9E3779B9)) & np.uint64(M32))
    base ^= np.uint64(seed_hi)
    tag = np.uint64(FMT_INDEX[kind] << 28 | operand << 24) | np.arange(K, dtype=np.uint64)
    return fmix32(base[:, None] ^ tag[None, :])


def codes(kind: str, operand: int, rows: int, K: int, seed: int, rng: int) -> np.ndarray:
    """Element codes [rows][K]: bf16 bit patterns (uint16), e4m3 bytes or e2m1
    nibbles (uint8)."""
    u = draws(kind, operand, rows, K, seed)
    if kind == "bf16":
        m = (u % np.uint64(2 * rng + 1)).astype(np.int64) - rng
        return kr.f32_to_bf16_bits((m.astype(np.float64) / 16.0).astype(np.float32))
    if kind == "fp8":
        return e4m3_codes_of_range(rng)[(u % np.uint64(16 * rng + 1)).astype(np.int64)]
    return (u & np.uint64(15)).astype(np.uint8)


def decode(kind: str, c: np.ndarray) -> np.ndarray:
    """Exact float64 values of element codes."""
    if kind == "bf16":
        return kr.bf16_bits_to_f64(c)
    return (kr.E4M3_LUT if kind == "fp8" else kr.E2M1_LUT)[c]


def numerators(kind: str, operand: int, rows: int, K: int, seed: int, rng: int) -> np.ndarray:
    """Integer numerators [rows][K] (int64), from the generator's definition
    and not from the codes."""
    u = draws(kind, operand, rows, K, seed)
    if kind == "bf16":
        return (u % np.uint64(2 * rng + 1)).astype(np.int64) - rng
    if kind == "fp8":
        j = (u % np.uint64(16 * rng + 1)).astype(np.int64)
        q = j - 1
        s, t = q // (8 * rng), q % (8 * rng)
        mag = (8 + (t & 7)) << (t >> 3)
        return np.where(j == 0, 0, np.where(s == 1, -mag, mag))
    c = (u & np.uint64(15)).astype(np.int64)
    e, m = (c >> 1) & 3, c & 1
    mag = np.where(e == 0, m, (2 + m) << np.maximum(e - 1, 0))
    return np.where(c & 8, -mag, mag)


def stored(kind: str, c: np.ndarray) -> np.ndarray:
    """Codes as the fill stores them: bf16 bits as int16 (for a bfloat16
    view), e4m3 bytes, e2m1 nibble pairs."""
    if kind == "bf16":
        return c.view(np.int16)
    return kr.pack_e2m1(c) if kind == "fp4" else c


def expected_sums(a: np.ndarray, b: np.ndarray):
    """(R, Q), int64 [M/256][N/256][256], of numerators a [M][K], b [N][K]."""
    tm, tn = a.shape[0] // TILE, b.shape[0] // TILE
    sa = a.reshape(tm, TILE, -1).sum(axis=1)  # [tm][K]
    sb = b.reshape(tn, TILE, -1).sum(axis=1)
    R = (a @ sb.T).reshape(tm, TILE, tn).transpose(0, 2, 1)
    Q = (b @ sa.T).reshape(tn, TILE, tm).transpose(2, 0, 1)
    return np.ascontiguousarray(R), np.ascontiguousarray(Q)


class VerifyClass(NamedTuple):
    """Who looks at element (row, col) of a 256 x 256 tile: the workgroup of
    `strip` (64 rows), in it `wave` (16 rows), whose lane `j` reports the row
    and whose `lane` loads the element as float `e` of its 16-byte vector."""
    strip: int
    wave: int
    j: int
    lane: int
    e: int

    @property
    def c(self) -> int:
        """The thread of the column check that compares this column."""
        return 4 * self.lane + self.e


def verify_class(row: int, col: int) -> VerifyClass:
    """The verifier's share of an in-tile position, from the verify section
    of the kernel file's header: a workgroup takes a strip of 64 rows, wave w
    of it the rows 16w..16w+15, and 64 lanes x float4 are one tile row."""
    if not (0 <= row < TILE and 0 <= col < TILE):
        raise ValueError(f"({row}, {col}) is outside a tile")
    return VerifyClass(row // 64, (row % 64) // 16, row % 16, col // 4, col % 4)


def operand_diff_count(kind: str, stored_a: np.ndarray, stored_b: np.ndarray) -> int:
    """Number of elements in which two stored operands differ: bf16 words,
    e4m3 bytes, e2m1 nibbles (two to the byte)."""
    if stored_a.shape != stored_b.shape or stored_a.dtype != stored_b.dtype:
        raise ValueError("operands of different shape or type")
    if kind != "fp4":
        return int(np.count_nonzero(stored_a != stored_b))
    d = stored_a.astype(np.uint8) ^ stored_b.astype(np.uint8)
    return int(np.count_nonzero(d & 0x0F) + np.count_nonzero(d & 0xF0))


def legal_other_code(kind: str, code: int, rng: int) -> int:
    """A different code of the same element set, so that an operand with it
    in place still has exact sums: bf16 (bit pattern) the neighbouring
    numerator in [-r, r], e4m3 the next code of e4m3_codes_of_range (the last
    wraps to zero), e2m1 the code with the other mantissa bit."""
    code = int(code)
    if kind == "bf16":
        m = float(kr.bf16_bits_to_f64(np.array([code], dtype=np.uint16))[0]) * 16.0
        if m != int(m) or abs(m) > rng:
            raise ValueError(f"bf16 {code:#06x} is not in the set of range {rng}")
        other = int(m) + 1 if m < rng else int(m) - 1
        return int(kr.f32_to_bf16_bits(np.array([other / 16.0], dtype=np.float32))[0])
    if kind == "fp8":
        legal = e4m3_codes_of_range(rng).tolist()
        return legal[(legal.index(code) + 1) % len(legal)]
    if not 0 <= code < 16:
        raise ValueError(f"{code} is no e2m1 code")
    return code ^ 1


def classify(C: np.ndarray, inv_granule: float, R: np.ndarray, Q: np.ndarray) -> dict:
    """The verifier's classification of an fp32 [M][N] array: malformed
    elements (not an integer number of granules of magnitude <= 2^24; they
    contribute 0), then the (tile_row, tile_col, index) of every row and
    column sum that differs from R and Q."""
    with np.errstate(invalid="ignore", over="ignore"):
        y = C.astype(np.float32) * np.float32(inv_granule)
        ok = (np.abs(y) <= np.float32(TWO24)) & (y == np.trunc(y))
    x = np.where(ok, y, 0).astype(np.int64)
    tm, tn = C.shape[0] // TILE, C.shape[1] // TILE
    t = x.reshape(tm, TILE, tn, TILE)
    rows = np.argwhere(t.sum(axis=3).transpose(0, 2, 1) != R)
    cols = np.argwhere(t.sum(axis=1) != Q)
    return {
        "malformed": [tuple(int(v) for v in rc) for rc in np.argwhere(~ok)],
        "rows": [tuple(int(v) for v in r) for r in rows],
        "cols": [tuple(int(v) for v in c) for c in cols],
    }
