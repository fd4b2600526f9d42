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

Plain module, not a conftest: it changes nothing about collection.
"""
from __future__ import annotations

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
