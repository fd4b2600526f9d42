"""Reference for the per-CU compute check (csrc/cu_check.hip), in numpy.

Written from the generator's definition, not from the kernel:

    fmix32(h): h^=h>>16; h*=0x85EBCA6B; h^=h>>13; h*=0xC2B2AE35; h^=h>>16

    u(seed, fmt, t, operand, row, k) =
        fmix32(fmix32(seed_lo + t*0x9E3779B9) ^ seed_hi
               ^ (fmt<<28 | operand<<20 | row<<12 | k))

    bf16:  m = (u % 255) - 127, value m/16
    e4m3:  j = u % 65, code E4M3_EXACT_CODES[j]
    e2m1:  code u & 15

fmt is 0 / 1 / 2 for bf16 / fp8 / fp4, operand 0 for A and 1 for B. A tile is
A[16][K] @ B[16][K].T; decoding goes through kernel_refs' LUTs and the
reference product is float64.

Where a lane's four outputs sit: row 4*(lane>>4) + reg, column lane & 15.

LDS: word w of round r holds fmix32(w*0x9E3779B9 + seed_lo + r), after the
first verify its complement. Words are handled as 16-byte vectors v = w // 4
by 256 threads (wave = thread // 64, lane = thread % 64): vector v is written
by thread v mod 256, verified first by thread (v - 65) mod 256 and, inverted,
by thread (v - 130) mod 256.

Plain module, not a conftest: it changes nothing about collection.
"""
from __future__ import annotations

import functools

import numpy as np

import kernel_refs as kr

FMT_INDEX = {"bf16": 0, "fp8": 1, "fp4": 2}
K = {"bf16": 1024, "fp8": 1152, "fp4": 1280}
EXACT_SET = {"bf16": "bf16", "fp8": "e4m3", "fp4": "e2m1"}
M32 = 0xFFFFFFFF


def fmix32(h: np.ndarray) -> np.ndarray:
    h = np.asarray(h, dtype=np.uint64) & M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def draws(fmt: str, tile: int, seed: int, operand: int) -> np.ndarray:
    """u for every (row, k) of one operand of one tile: uint64 [16][K]."""
    seed_lo, seed_hi = seed & M32, (seed >> 32) & M32
    base = int(fmix32(np.uint64((seed_lo + tile * 0x9E3779B9) & M32))) ^ seed_hi
    row = np.arange(16, dtype=np.uint64)[:, None]
    k = np.arange(K[fmt], dtype=np.uint64)[None, :]
    tag = np.uint64(FMT_INDEX[fmt] << 28 | operand << 20) | row << 12 | k
    return fmix32(np.uint64(base) ^ tag)


def bf16_m(u: np.ndarray) -> np.ndarray:
    return (u % 255).astype(np.int64) - 127


def e4m3_codes(u: np.ndarray) -> np.ndarray:
    return kr.E4M3_EXACT_CODES[(u % 65).astype(np.int64)]


def e2m1_codes(u: np.ndarray) -> np.ndarray:
    return (u & 15).astype(np.uint8)


def operand_values(fmt: str, tile: int, seed: int, operand: int) -> np.ndarray:
    """Exact float64 values [16][K] of operand 0 (A) or 1 (B)."""
    u = draws(fmt, tile, seed, operand)
    if fmt == "bf16":
        return bf16_m(u).astype(np.float64) / 16.0
    if fmt == "fp8":
        return kr.E4M3_LUT[e4m3_codes(u)]
    return kr.E2M1_LUT[e2m1_codes(u)]


def reference_tile(fmt: str, tile: int, seed: int) -> np.ndarray:
    """float64 [16][16]: A64 @ B64.T."""
    return operand_values(fmt, tile, seed, 0) @ operand_values(fmt, tile, seed, 1).T


def lane_reg_to_row_col(lane: int, reg: int) -> tuple:
    """(row, col) of the tile element lane `lane` holds in accumulator `reg`."""
    assert 0 <= lane < 64 and 0 <= reg < 4
    return 4 * (lane >> 4) + reg, lane & 15


@functools.lru_cache(maxsize=None)
def _reference_tile_once(fmt: str, tile: int, seed: int) -> np.ndarray:
    ref = reference_tile(fmt, tile, seed)
    ref.setflags(write=False)
    return ref


def expected_bits(fmt: str, tile: int, seed: int, lane: int, reg: int) -> int:
    """fp32 bit pattern of the reference tile's element at (lane, reg)."""
    row, col = lane_reg_to_row_col(lane, reg)
    ref = _reference_tile_once(fmt, tile, seed)[row, col]
    f32 = np.float32(ref)
    assert float(f32) == float(ref), "the reference tile is exact in fp32"
    return int(f32.view(np.uint32))


def lds_word(word: int, seed: int, round: int, inverted: bool = False) -> int:
    """What LDS word `word` holds in round `round`; inverted: after the first
    verify has stored the complement."""
    seed_lo = seed & M32
    w = int(fmix32(np.uint64((word * 0x9E3779B9 + seed_lo + round) & M32)))
    return w ^ M32 if inverted else w


THREADS = 256
LDS_VERIFY_SHIFT = (65, 130)


def lds_writer(word: int) -> dict:
    """The thread that fills `word`, with its wave and lane."""
    thread = (word // 4) % THREADS
    return {"thread": thread, "wave": thread // 64, "lane": thread % 64}


def lds_verifier(word: int, phase: int) -> dict:
    """The thread that reads `word` in verify phase 0 or 1, with its wave and
    lane."""
    thread = ((word // 4) % THREADS - LDS_VERIFY_SHIFT[phase]) % THREADS
    return {"thread": thread, "wave": thread // 64, "lane": thread % 64}
