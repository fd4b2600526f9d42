"""Reference implementations of the HBM memtest patterns
(csrc/hbm_memtest.hip): numpy uint64 and torch int64. The torch version runs
on either device, so the GPU tests build their expected buffers on the card.

Word g (a global u64 index) holds, for a u64 seed:

    fmix32(h): h^=h>>16; h*=0x85EBCA6B; h^=h>>13; h*=0xC2B2AE35; h^=h>>16
    addr: w = g ^ seed
    rand: x = g ^ seed; a = (u32)x; b = (u32)(x>>32)
          lo = fmix32(a + b*0x9E3779B9)
          hi = fmix32(~a + b*0x85EBCA77 + 0x27D4EB2F)
          w  = hi<<32 | lo
    zero: w = 0
    invert: w = ~w

word_class names who handles a word of a view in the kernel (tile, trip,
workgroup, wave, lane, unroll slot, half of the 16-byte vector), so that a
failing GPU assertion says which part of the kernel missed it.
"""
from typing import NamedTuple

import numpy as np

SEED = 0x0123456789ABCDEF
M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1

# rand, seed = SEED: the table of the pattern's definition
GOLDEN_RAND = [
    (0, 0x9DAE06A589DB6344),
    (1, 0x34E27C7C7258F2A8),
    (2, 0xEF52FB2E42697280),
    (2**32 - 1, 0xB38E1CE74EF96E58),
    (2**32, 0x94234A8FB2FE8DCC),
    (2**32 + 1, 0xDA90EBAAEA16BC8C),
    (2**40 + 7, 0xE26A43E94606D2BC),
]


# memtest_geometry() of the kernel as committed; the GPU tests read the
# binding and hold it to this
GEOMETRY = {"block": 256, "words_per_thread_iter": 8, "max_grid": 2048}


class WordClass(NamedTuple):
    """Who handles one body word of a view (csrc/hbm_memtest.hip)."""
    tile: int       # index of the block * unroll vectors it lies in
    trip: int       # iteration of the workgroup's grid-stride loop
    workgroup: int  # blockIdx.x
    wave: int
    lane: int
    slot: int       # unroll slot j of the tile loop
    half: int       # 0: .x of the 16-byte vector, 1: .y
    full: bool      # the tile takes the unrolled path, not the bounds-checked one


def word_class(p: int, head: int, n: int, geo=GEOMETRY):
    """Position p of an n-word view -> "head", "tail" or a WordClass.

    head is 1 for a view that is only 8-byte aligned (its first word is
    handled alone by thread 0 of workgroup 0) and 0 for a 16-byte-aligned
    one; a tail word exists where n - head is odd (thread 1 of workgroup 0).
    The rest is the body: vector vi = (p - head) // 2 belongs to tile
    vi // (block * unroll), where thread vi % block handles it in unroll slot
    (vi % (block * unroll)) // block, and tile t runs in workgroup
    t % max_grid on trip t // max_grid."""
    if head not in (0, 1):
        raise ValueError(f"head must be 0 or 1, got {head}")
    if not 0 <= p < n:
        raise ValueError(f"position {p} is outside a view of {n} words")
    if head and p == 0:
        return "head"
    if (n - head) % 2 == 1 and p == n - 1:
        return "tail"
    block = geo["block"]
    tile_vecs = block * (geo["words_per_thread_iter"] // 2)
    vi = (p - head) // 2
    tile, within = divmod(vi, tile_vecs)
    slot, thread = divmod(within, block)
    nvec = (n - head) // 2
    return WordClass(
        tile=tile,
        trip=tile // geo["max_grid"],
        workgroup=tile % geo["max_grid"],
        wave=thread // 64,
        lane=thread % 64,
        slot=slot,
        half=(p - head) % 2,
        full=(tile + 1) * tile_vecs <= nvec,
    )


def to_i64(v: int) -> int:
    """Two's-complement view of an unsigned 64-bit value (torch has no u64)."""
    v &= M64
    return v - (1 << 64) if v >= (1 << 63) else v


def to_u64(v: int) -> int:
    return int(v) & M64


# ---------------------------------------------------------------------------
# numpy
# ---------------------------------------------------------------------------

def _fmix32_np(h):
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(M32)
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & np.uint64(M32)
    h = h ^ (h >> np.uint64(16))
    return h


def pattern_np(g, pattern: str, seed: int = SEED, invert: bool = False):
    """g: array-like of u64 word indices -> np.uint64 array of pattern words."""
    g = np.asarray(g, dtype=np.uint64)
    m32 = np.uint64(M32)
    if pattern == "zero":
        w = np.zeros_like(g)
    elif pattern == "addr":
        w = g ^ np.uint64(seed)
    elif pattern == "rand":
        x = g ^ np.uint64(seed)
        a = x & m32
        b = x >> np.uint64(32)
        # 32-bit values in u64 lanes: products stay below 2^64, mask after each
        lo = _fmix32_np((a + ((b * np.uint64(0x9E3779B9)) & m32)) & m32)
        hi = _fmix32_np(
            ((a ^ m32) + ((b * np.uint64(0x85EBCA77)) & m32) + np.uint64(0x27D4EB2F)) & m32
        )
        w = (hi << np.uint64(32)) | lo
    else:
        raise ValueError(pattern)
    return ~w if invert else w


def arange_np(base: int, n: int):
    return np.uint64(base) + np.arange(n, dtype=np.uint64)


# ---------------------------------------------------------------------------
# torch (int64; every intermediate is masked to 32 bits, so nothing overflows)
# ---------------------------------------------------------------------------

def _fmix32_t(h):
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & M32
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & M32
    h = h ^ (h >> 16)
    return h


def pattern_torch(g, pattern: str, seed: int = SEED, invert: bool = False):
    """g: int64 tensor holding the bit patterns of u64 word indices (any
    device) -> int64 tensor holding the bit patterns of the pattern words."""
    import torch

    if pattern == "zero":
        w = torch.zeros_like(g)
    elif pattern == "addr":
        w = g ^ to_i64(seed)
    elif pattern == "rand":
        x = g ^ to_i64(seed)
        a = x & M32
        b = (x >> 32) & M32  # arithmetic shift: mask the sign extension off
        lo = _fmix32_t((a + ((b * 0x9E3779B9) & M32)) & M32)
        hi = _fmix32_t(((a ^ M32) + ((b * 0x85EBCA77) & M32) + 0x27D4EB2F) & M32)
        w = (hi << 32) | lo
    else:
        raise ValueError(pattern)
    return ~w if invert else w


def arange_torch(base: int, n: int, device="cpu"):
    """Word indices base .. base+n-1 as int64 bit patterns (wraps like u64)."""
    import torch

    return torch.arange(n, dtype=torch.int64, device=device) + to_i64(base)


def expected_torch(base: int, n: int, pattern: str, seed: int = SEED,
                   invert: bool = False, device="cpu"):
    return pattern_torch(arange_torch(base, n, device), pattern, seed, invert)
