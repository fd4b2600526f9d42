"""Reference helpers for the HIP kernel numerics tests.

Operand generators return the raw operand (as the kernel binding wants it)
together with its exact decoded float64 values; the reference is always
``A64 @ B64.T`` in float64 on the CPU; two comparators judge a kernel's fp32
output against it and, on failure, say *where* it is wrong (tile, wave
quadrant, fragment) instead of just "mismatch".

Exactness condition
-------------------
Let every entry of A be an integer multiple of ``granule_a`` with magnitude
at most ``max_a`` (same for B). Each product is then an integer multiple of
``g = granule_a * granule_b`` and every partial sum of at most K products, in
any order, is an integer multiple of g with magnitude at most
``max_a * max_b * K``. If

    max_a * max_b * K / (granule_a * granule_b) <= 2**24

all those integers are at most 2**24 and therefore exactly representable in
fp32 (24-bit significand; g is a power of two): an fp32-accumulating kernel
must reproduce the float64 reference bit for bit, whatever its summation
order. ``exact_condition`` evaluates the left-hand side.

Plain module, not a conftest: it changes nothing about collection.
"""
from __future__ import annotations

import numpy as np
import torch

TWO24 = float(2**24)

# 8-phase GEMM geometry used to name the place of a mismatch (csrc/gemm_*):
# 256^2 block tile, four 128^2 quadrants (qm, qn), 8 waves as 2(M) x 4(N)
# owning 64x32 per quadrant, 16x16 MFMA fragments.
TILE = 256
QUAD = 128
WAVE_M = 64
WAVE_N = 32
FRAG = 16


# ---------------------------------------------------------------------------
# Format LUTs, from the format definitions (no torch casts)
# ---------------------------------------------------------------------------

def e4m3_value(code: int) -> float:
    """OCP e4m3fn: 1 sign, 4 exponent (bias 7), 3 mantissa bits; subnormals
    at exponent field 0; no infinities; S.1111.111 is NaN."""
    sign = -1.0 if code & 0x80 else 1.0
    e = (code >> 3) & 0xF
    m = code & 0x7
    if e == 0xF and m == 0x7:
        return float("nan")
    if e == 0:
        return sign * (m / 8.0) * 2.0 ** (1 - 7)
    return sign * (1.0 + m / 8.0) * 2.0 ** (e - 7)


def e2m1_value(code: int) -> float:
    """OCP e2m1: 1 sign, 2 exponent (bias 1), 1 mantissa bit; no NaN/Inf."""
    sign = -1.0 if code & 0x8 else 1.0
    e = (code >> 1) & 0x3
    m = code & 0x1
    if e == 0:
        return sign * (m / 2.0)
    return sign * (1.0 + m / 2.0) * 2.0 ** (e - 1)


E4M3_LUT = np.array([e4m3_value(c) for c in range(256)], dtype=np.float64)
E2M1_LUT = np.array([e2m1_value(c) for c in range(16)], dtype=np.float64)

E4M3_NAN_CODES = (0x7F, 0xFF)
E4M3_FINITE_CODES = np.array(
    [c for c in range(256) if c not in E4M3_NAN_CODES], dtype=np.uint8)
# zero plus every code with exponent field 6..9 (both signs, all mantissas):
# values are multiples of 2^-4 (0.5 * 1/8) with magnitude at most 7.5
E4M3_EXACT_CODES = np.array(
    [0x00] + [c for c in range(256) if 6 <= ((c >> 3) & 0xF) <= 9],
    dtype=np.uint8)


# ---------------------------------------------------------------------------
# Exact operand sets: (max magnitude, granule, largest K the set is used at)
# ---------------------------------------------------------------------------

EXACT_SETS = {
    # m/16, integer m in [-127, 127]: 7 significant bits, exact in bf16 and f32
    "bf16": {"max": 127.0 / 16.0, "granule": 1.0 / 16.0, "k_max": 1040},
    "f32": {"max": 127.0 / 16.0, "granule": 1.0 / 16.0, "k_max": 1040},
    "e4m3": {"max": 7.5, "granule": 2.0 ** -4, "k_max": 1165},
    # all 16 codes: multiples of 0.5 up to 6
    "e2m1": {"max": 6.0, "granule": 0.5, "k_max": 2048},
}


def exact_condition(max_a: float, max_b: float, K: int, granule_a: float,
                    granule_b: float) -> float:
    """Left-hand side of the exactness condition; must be <= 2**24."""
    return max_a * max_b * K / (granule_a * granule_b)


def require_exact(kind: str, K: int) -> None:
    s = EXACT_SETS[kind]
    lhs = exact_condition(s["max"], s["max"], K, s["granule"], s["granule"])
    assert lhs <= TWO24, (
        f"{kind} exact set does not guarantee fp32-exact sums at K={K}: "
        f"{lhs} > 2^24")


# ---------------------------------------------------------------------------
# Generators (seeded, CPU). Each returns (raw operand, exact float64 values).
# ---------------------------------------------------------------------------

def _rng(seed: int) -> np.random.Generator:
    return np.random.default_rng(seed)


def _sixteenths(rows: int, cols: int, seed: int) -> np.ndarray:
    m = _rng(seed).integers(-127, 128, size=(rows, cols))
    return m.astype(np.float64) / 16.0


def exact_bf16(rows: int, cols: int, seed: int):
    v = torch.from_numpy(_sixteenths(rows, cols, seed))
    raw = v.to(torch.bfloat16)
    assert torch.equal(raw.double(), v)
    return raw, v


def exact_f32(rows: int, cols: int, seed: int):
    v = torch.from_numpy(_sixteenths(rows, cols, seed))
    raw = v.to(torch.float32)
    assert torch.equal(raw.double(), v)
    return raw, v


def real_bf16(rows: int, cols: int, seed: int, scale: float = 0.5):
    """randn rounded to bf16 (real-valued operands; sums are NOT exact)."""
    g = torch.Generator().manual_seed(seed)
    raw = (torch.randn(rows, cols, generator=g) * scale).to(torch.bfloat16)
    return raw, raw.double()


def real_f32(rows: int, cols: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(rows, cols, generator=g)
    return raw, raw.double()


def _codes_equal_frequency(codes: np.ndarray, rows: int, cols: int,
                           seed: int) -> np.ndarray:
    """Every code of `codes` with (as nearly as possible) equal frequency, in
    a seeded random arrangement."""
    n = rows * cols
    assert n >= len(codes)
    tiled = np.resize(codes, n)
    return _rng(seed).permutation(tiled).reshape(rows, cols)


def exact_e4m3(rows: int, cols: int, seed: int):
    codes = _codes_equal_frequency(E4M3_EXACT_CODES, rows, cols, seed)
    return torch.from_numpy(codes), torch.from_numpy(E4M3_LUT[codes])


def full_range_e4m3(rows: int, cols: int, seed: int):
    """Every finite e4m3 code (both zeros, all subnormals, +-448); the NaN
    codes 0x7F/0xFF never appear."""
    codes = _codes_equal_frequency(E4M3_FINITE_CODES, rows, cols, seed)
    return torch.from_numpy(codes), torch.from_numpy(E4M3_LUT[codes])


def pack_e2m1(nibbles: np.ndarray) -> np.ndarray:
    """[rows][K] nibble codes -> [rows][K/2] bytes, low nibble = even k."""
    assert nibbles.shape[1] % 2 == 0
    return (nibbles[:, 0::2] | (nibbles[:, 1::2] << 4)).astype(np.uint8)


def all_e2m1(rows: int, K: int, seed: int):
    """All 16 e2m1 codes; returns (packed [rows][K/2] uint8, float64 [rows][K])."""
    nib = _codes_equal_frequency(np.arange(16, dtype=np.uint8), rows, K, seed)
    return torch.from_numpy(pack_e2m1(nib)), torch.from_numpy(E2M1_LUT[nib])


# ---------------------------------------------------------------------------
# numpy ports of the probe operand fills (fill_bf16_hash_kernel in
# csrc/hipcore.hip, fill_e4m3_hash_kernel and fill_e2m1_hash_kernel in
# csrc/gemm_fp8_mx.hip): unsigned 32-bit arithmetic carried in uint64 and
# masked, so nothing depends on numpy's overflow behaviour.
# ---------------------------------------------------------------------------

_U32 = np.uint64(0xFFFFFFFF)
PROBE_SEEDS = (1, 7)  # A and Bt of every *_tflops probe
BF16_BELOW_ONE = 1.0 - 2.0 ** -8  # the largest bf16 below 1


def _u64(x: int) -> np.uint64:
    return np.uint64(x)


def f32_to_bf16_bits(v: np.ndarray) -> np.ndarray:
    """Round-to-nearest-even float32 -> bf16 bit patterns (finite inputs)."""
    b = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((b + _u64(0x7FFF) + ((b >> _u64(16)) & _u64(1))) >> _u64(16)).astype(np.uint16)


def bf16_bits_to_f64(bits: np.ndarray) -> np.ndarray:
    return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def fill_bf16_hash(n: int, seed: int) -> np.ndarray:
    """bf16 bit patterns (uint16) of fill_bf16_hash_kernel."""
    i = np.arange(n, dtype=np.uint64)
    h = (i * _u64(2654435761) + _u64(seed)) & _U32
    h ^= h >> _u64(15)
    h = (h * _u64(2246822519)) & _U32
    h ^= h >> _u64(13)
    # every step is exact in float32: a 24-bit integer, a power-of-two
    # division, and a difference of magnitude at most 1 on a 2^-23 grid
    v = (h & _u64(0xFFFFFF)).astype(np.float32) / np.float32(8388608.0) - np.float32(1.0)
    return f32_to_bf16_bits(np.minimum(v, np.float32(BF16_BELOW_ONE)))


def _mx_hash(n: int, seed: int) -> np.ndarray:
    i = np.arange(n, dtype=np.uint64)
    h = ((i * _u64(2654435761)) & _U32) ^ _u64(seed)
    h ^= h >> _u64(13)
    h = (h * _u64(0x85EBCA6B)) & _U32
    h ^= h >> _u64(16)
    return h


def fill_e4m3_hash(n: int, seed: int) -> np.ndarray:
    """e4m3 codes (uint8) of fill_e4m3_hash_kernel: sign = hash bit 0,
    exponent field 4 + bits 3:1, mantissa = bits 6:4."""
    h = _mx_hash(n, seed)
    return (((h & _u64(1)) << _u64(7)) | ((((h >> _u64(1)) & _u64(7)) + _u64(4)) << _u64(3))
            | ((h >> _u64(4)) & _u64(7))).astype(np.uint8)


def fill_e2m1_hash(n: int, seed: int) -> np.ndarray:
    """Packed e2m1 bytes (uint8) of fill_e2m1_hash_kernel: hash bits 7:0."""
    return (_mx_hash(n, seed) & _u64(0xFF)).astype(np.uint8)


FILL_PORTS = {"bf16": fill_bf16_hash, "e4m3": fill_e4m3_hash, "e2m1": fill_e2m1_hash}


def unpack_e2m1(packed: np.ndarray) -> np.ndarray:
    """[rows][K/2] bytes -> [rows][K] nibble codes; inverse of pack_e2m1."""
    out = np.empty((packed.shape[0], packed.shape[1] * 2), dtype=np.uint8)
    out[:, 0::2] = packed & 0xF
    out[:, 1::2] = packed >> 4
    return out


def check_fill_properties(kind: str, seed_a: np.ndarray, seed_b: np.ndarray) -> None:
    """What a probe fill must be for the TF it feeds to mean anything (zero,
    constant or sign-stuck operands inflate it). `seed_a` and `seed_b` are
    the raw fills of one kind and length from the two probe seeds; the same
    assertions run on the port and on the kernel's output."""
    assert seed_a.shape == seed_b.shape and seed_a.size >= 1 << 20
    for raw in (seed_a, seed_b):
        # everything below is read off the histogram of the raw patterns
        hist = np.bincount(raw, minlength=1 << (8 * raw.dtype.itemsize))
        used = np.flatnonzero(hist)
        if kind == "bf16":
            v = bf16_bits_to_f64(used.astype(np.uint16))
            assert v.min() >= -1.0 and v.max() < 1.0, (v.min(), v.max())
            assert used.size > 1000, "bf16 fill is (nearly) constant"
            neg = float(hist[0x8000:].sum()) / raw.size
            assert abs(neg - 0.5) < 0.005, f"bf16 fill signs: {neg:.4f} negative"
        elif kind == "e4m3":
            assert not np.isin(used, E4M3_NAN_CODES).any()
            assert sorted(set(((used >> 3) & 0xF).tolist())) == list(range(4, 12))
            assert sorted(set((used >> 7).tolist())) == [0, 1]
            assert sorted(set((used & 7).tolist())) == list(range(8))
        else:
            assert used.size == 256
    differ = float(np.mean(seed_a != seed_b))
    assert differ > 0.90, f"{kind} fills of the two seeds differ in {differ:.4f} of positions"


def reference(a64: torch.Tensor, b64: torch.Tensor) -> torch.Tensor:
    """ref[M][N] = A64[M][K] @ B64[N][K].T in float64 on the CPU."""
    assert a64.dtype == torch.float64 and b64.dtype == torch.float64
    return a64 @ b64.T


# ---------------------------------------------------------------------------
# Comparators
# ---------------------------------------------------------------------------

def locate(row: int, col: int) -> dict:
    """Name the place of element (row, col) in the 256^2 8-phase geometry."""
    tr, tc = row % TILE, col % TILE
    return {
        "tile": (row // TILE, col // TILE),
        "quadrant": (tr // QUAD, tc // QUAD),
        "wave": ((tr % QUAD) // WAVE_M, (tc % QUAD) // WAVE_N),
        "fragment": ((tr % WAVE_M) // FRAG, (tc % WAVE_N) // FRAG),
        "in_fragment": (row % FRAG, col % FRAG),
    }


NXCD = 8  # gemm_8ph::NXCD


def _xcd_start(x: int, nwg: int) -> int:
    """First tile of the contiguous range tile_coord<1> gives to XCD x."""
    q, r = divmod(nwg, NXCD)
    return x * (q + 1) if x < r else r * (q + 1) + (x - r) * q


def block_tile(bid: int, tiles_n: int, nwg: int, xcd_remap: bool):
    """(tile_row, tile_col) computed by workgroup `bid` of `nwg`: the formula
    of tile_coord in csrc/gemm_8phase_common.h."""
    if xcd_remap:
        xcd, seq = bid % NXCD, bid // NXCD
        bid = _xcd_start(xcd, nwg) + seq
    return bid // tiles_n, bid % tiles_n


def owner_block(tile_row: int, tile_col: int, tiles_n: int, nwg: int,
                xcd_remap: bool):
    """(blockIdx.x, blockIdx.x % 8) of the workgroup that computes a tile:
    the inverse of block_tile. The second value is the XCD the workgroup runs
    on under round-robin dispatch."""
    t = tile_row * tiles_n + tile_col
    assert 0 <= tile_col < tiles_n and 0 <= t < nwg, (tile_row, tile_col, tiles_n, nwg)
    bid = t
    if xcd_remap:
        xcd = max(x for x in range(NXCD) if _xcd_start(x, nwg) <= t)
        bid = (t - _xcd_start(xcd, nwg)) * NXCD + xcd
    return bid, bid % NXCD


def describe_owners(e: "KernelMismatch", tiles_n: int, nwg: int,
                    xcd_remap: bool) -> str:
    """Who computed what a KernelMismatch found bad: the block of the first
    bad element, and the blockIdx % 8 classes of all bad tiles. One class
    points at the hardware (an XCD); a pattern in tile coordinates at the
    kernel."""
    bid, xcd = owner_block(*e.where["tile"], tiles_n, nwg, xcd_remap)
    classes = sorted({owner_block(tr, tc, tiles_n, nwg, xcd_remap)[1]
                      for tr, tc in e.bad_tiles})
    return (f"first bad element computed by blockIdx.x {bid} of {nwg} "
            f"(blockIdx % 8 = {xcd}, xcd_remap={int(bool(xcd_remap))}); "
            f"{len(e.bad_tiles)} bad tiles, their blockIdx % 8 in {classes}")


class KernelMismatch(AssertionError):
    """Raised by the comparators; carries the location of the first bad
    element so tests (and people) can read off the phase or fragment."""

    def __init__(self, what: str, bad: torch.Tensor, got: torch.Tensor,
                 want: torch.Tensor, extra: str = ""):
        idx = torch.nonzero(bad)
        self.n_bad = int(idx.shape[0])
        self.first = (int(idx[0, 0]), int(idx[0, 1]))
        self.where = locate(*self.first)
        self.all_nan = bool(torch.isnan(got[bad]).all())
        rows = idx[:, 0]
        cols = idx[:, 1]
        self.bad_rows = (int(rows.min()), int(rows.max()))
        self.bad_cols = (int(cols.min()), int(cols.max()))
        self.bad_tiles = [tuple(t) for t in torch.unique(idx // TILE, dim=0).tolist()]
        r, c = self.first
        w = self.where
        msg = (
            f"{what}: {self.n_bad} of {bad.numel()} elements bad; first at "
            f"(row {r}, col {c}): got {float(got[r, c])!r}, want "
            f"{float(want[r, c])!r}; 256^2 tile {w['tile']}, quadrant "
            f"(qm,qn)={w['quadrant']}, wave (wm,wn)={w['wave']}, 16x16 "
            f"fragment (fm,fn)={w['fragment']}, in-fragment {w['in_fragment']}; "
            f"bad rows {self.bad_rows}, bad cols {self.bad_cols}; "
            + ("ALL bad elements are NaN (never written)" if self.all_nan
               else "bad elements are not all NaN (written, but wrong)")
            + extra)
        super().__init__(msg)


def _as_cpu_f32(C: torch.Tensor) -> torch.Tensor:
    assert C.dtype == torch.float32, f"kernel output must be fp32, got {C.dtype}"
    return C.detach().cpu().contiguous()


def assert_exact(C: torch.Tensor, ref: torch.Tensor) -> None:
    """Bit-equality of C with ref cast to fp32; the cast must be lossless.

    An fp32 accumulator that starts at +0 never produces -0 (x + -x = +0 and
    +0 + -0 = +0 under round-to-nearest), so zero results are required to be
    +0: the reference is normalised with `+ 0.0`, which only maps -0 to +0.
    """
    got = _as_cpu_f32(C)
    ref = ref.detach().cpu() + 0.0
    assert got.shape == ref.shape, (got.shape, ref.shape)
    want = ref.float()
    assert torch.equal(want.double(), ref), (
        "reference is not exactly representable in fp32: the operand set "
        "violates the exactness condition for this K")
    bad = got.view(torch.int32) != want.view(torch.int32)
    if bool(bad.any()):
        raise KernelMismatch("not bit-exact", bad, got, want)


def sum_bound(absA: torch.Tensor, absB: torch.Tensor, K: int) -> torch.Tensor:
    """Per-element bound K * 2^-23 * (|A| @ |B|^T), float64.

    Standard bound for K fp32 additions of exact products in any order:
    each addition perturbs the running sum by a relative error of at most
    one rounding unit, so |C - ref| <= K * u * sum|a_k b_k| to first order.
    The factor used is 2^-23 = 2u (u = 2^-24, the fp32 unit roundoff), which
    also covers an accumulator that TRUNCATES instead of rounding to nearest
    (relative error < 2^-23 per addition). That is the only assumption:
    products are formed exactly (true for bf16 x bf16, fp8 x fp8, and
    f32 x f32 within an MFMA that keeps the full product) and each
    accumulation step loses at most one fp32 ulp. Derived, not measured.
    """
    return float(K) * 2.0 ** -23 * (absA.double() @ absB.double().T)


# The MX-scaled fp8 MFMA (v_mfma_scale_f32_{16x16x128,32x32x64}_f8f6f4) does
# NOT add its products in fp32. Measured on gfx950 with crafted operands
# through the bit-exact-verified GEMM (docs/testing.md has the table): the
# products of MX_GROUP consecutive k are aligned to the group's largest
# exponent sum E = exp(a) + exp(b) and every bit below 2^(E - MX_KEPT_BITS) is
# truncated toward zero; group sums are then combined at (at least) fp32
# precision. Each of the 7 non-largest products of a group therefore loses
# less than 2^(E-13) <= 2^-13 * max|a_k b_k| <= 2^-13 * sum_group|a_k b_k|,
# which adds MX_FP8_TRUNCATION * (|A| @ |B|^T) to the bound. In the exact e4m3
# set the exponent sums of nonzero products differ by at most 6 and a product
# has 6 fraction bits, so nothing lies below 2^(E-12): it never reaches the
# cut and stays bit-exact.
MX_GROUP = 8
MX_KEPT_BITS = 13
MX_FP8_TRUNCATION = (MX_GROUP - 1) * 2.0 ** -MX_KEPT_BITS


def mx_fp8_truncated_reference(codes_a: torch.Tensor, codes_b: torch.Tensor,
                               rows_per_chunk: int = 16) -> torch.Tensor:
    """float64 model of what the MX fp8 MFMA computes for A @ B^T: exact
    products, truncated toward zero per group of 8 consecutive k at
    2^(E_max - 13), then summed exactly. Runs on the device the codes are on,
    in chunks of rows so the M*N*K temporaries stay small; returns a CPU
    tensor."""
    dev = codes_a.device
    M, K = codes_a.shape
    N = codes_b.shape[0]
    assert K % MX_GROUP == 0 and codes_b.shape[1] == K
    lut = torch.from_numpy(E4M3_LUT).to(dev)
    field = torch.arange(256, device=dev) >> 3 & 0xF
    expo = torch.where(field == 0, 1, field) - 7  # subnormals share exponent -6
    ia, ib = codes_a.long(), codes_b.long()
    vb, eb = lut[ib], expo[ib]
    out = torch.empty(M, N, dtype=torch.float64, device=dev)
    for r0 in range(0, M, rows_per_chunk):
        ra = ia[r0:r0 + rows_per_chunk]
        P = lut[ra][:, None, :] * vb[None, :, :]
        E = expo[ra][:, None, :] + eb[None, :, :]
        E = torch.where(P == 0, -1000, E)
        shape = (P.shape[0], N, K // MX_GROUP, MX_GROUP)
        Emax = E.view(shape).amax(dim=3, keepdim=True)
        q = torch.pow(2.0, (Emax - MX_KEPT_BITS).double())
        out[r0:r0 + rows_per_chunk] = (torch.trunc(P.view(shape) / q) * q).sum(dim=(2, 3))
    return out.cpu()


def assert_within_sum_bound(C: torch.Tensor, ref: torch.Tensor,
                            absA: torch.Tensor, absB: torch.Tensor,
                            K: int, extra_factor: float = 0.0,
                            bound: torch.Tensor = None) -> float:
    """Per element |C - ref| <= (K * 2^-23 + extra_factor) * (|A| @ |B|^T).
    `extra_factor` is 0 except for the MX fp8 instruction's documented
    product truncation (MX_FP8_TRUNCATION). `bound` may carry a precomputed
    sum_bound(absA, absB, K) for callers that compare many runs of one
    problem. Returns the worst observed err/bound so callers can print it."""
    got = _as_cpu_f32(C)
    ref = ref.detach().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert extra_factor in (0.0, MX_FP8_TRUNCATION)
    if bound is None:
        bound = sum_bound(absA, absB, K)
    bound = bound.cpu() * (1.0 + extra_factor / (K * 2.0 ** -23))
    err = (got.double() - ref).abs()
    bad = ~(err <= bound)  # NaN compares false -> bad
    ratio = torch.where(bound > 0, err / bound, (err > 0).double() * float("inf"))
    ratio = torch.nan_to_num(ratio, nan=float("inf"))
    worst = float(ratio.max())
    if bool(bad.any()):
        raise KernelMismatch("outside the K*2^-23*(|A|@|B|^T) bound", bad, got,
                             ref, f"; worst err/bound {worst:.3g}")
    return worst


# ---------------------------------------------------------------------------
# Poisoned output buffer with a guard zone behind it
# ---------------------------------------------------------------------------

POISON_BITS = 0x7FC0DEAD  # a quiet NaN with a recognisable payload
GUARD_FLOATS = 4096


class PoisonedOut:
    """`out` is the first rows*cols floats of a larger buffer filled with a
    NaN pattern; GUARD_FLOATS more floats lie behind it. A kernel that skips
    a store leaves NaN in `out`; one that writes past the end disturbs the
    guard."""

    def __init__(self, numel: int, device, shape=None):
        self.numel = numel
        self.buf = torch.empty(numel + GUARD_FLOATS, dtype=torch.float32,
                               device=device)
        self.out = self.buf[:numel]
        if shape is not None:
            self.out = self.out.view(*shape)
        self.poison()

    def poison(self) -> None:
        self.buf.view(torch.int32).fill_(POISON_BITS)

    def guard_intact(self) -> bool:
        g = self.buf[self.numel:].view(torch.int32)
        return bool((g == POISON_BITS).all())

    def check(self, what: str = "") -> None:
        """No NaN left in out, guard untouched."""
        assert self.guard_intact(), f"{what}: guard behind out was overwritten"
        n_nan = int(torch.isnan(self.out).sum())
        assert n_nan == 0, f"{what}: {n_nan} elements of out were never written"
