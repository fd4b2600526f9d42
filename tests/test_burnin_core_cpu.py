"""The burn-in's shared core (csrc/burnin_core.h) on the CPU.

csrc/burnin_selftest.cpp is compiled with g++ and run as a program of its
own: once bare (its own checks), then per sub-command, whose raw output is
compared bit for bit with the numpy references the GPU tests hold the kernels
to (cu_check_refs, gemm_check_refs, memtest_refs). Nothing is loaded into
this process.
"""
import os
import subprocess

import numpy as np
import pytest

import cu_check_refs as cr
import gemm_check_refs as gr
import kernel_refs as kr
import memtest_refs as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "csrc", "burnin_selftest.cpp")
HIGH_SEED = 0xFFFFFFFF00000001  # every bit of seed_hi set: the top tag bits flip
FULL_RANGE = {"bf16": 127, "fp8": 4, "fp4": 16}


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("burnin") / "burnin_selftest")
    subprocess.run(["g++", "-std=c++17", "-O1", SRC, "-o", exe], check=True)
    return exe


def _run(exe, *args) -> str:
    r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout


def _numbers(exe, *args, dtype=np.int64) -> np.ndarray:
    return np.array([int(t) for t in _run(exe, *args).split()], dtype=dtype)


def _seeds():
    from gpu_docker_api_amd.ops.hipcore import CU_CHECK_SEED, GEMM_CHECK_SEED

    return CU_CHECK_SEED, GEMM_CHECK_SEED


def _decode(kind: str, codes: np.ndarray) -> np.ndarray:
    if kind == "bf16":
        return kr.bf16_bits_to_f64(codes.astype(np.uint16))
    return (kr.E4M3_LUT if kind == "fp8" else kr.E2M1_LUT)[codes]


def test_bare_selftest(selftest):
    assert _run(selftest).strip() == "burnin selftest OK"


def test_full_ranges_are_the_references():
    """The premise of the shared generator: cu_check's code sets are
    gemm_check's at the full range."""
    assert np.array_equal(gr.e4m3_codes_of_range(4), kr.E4M3_EXACT_CODES)
    assert gr.max_numerator("bf16", 127) == 127


@pytest.mark.parametrize("seed_index", [0, 1])
@pytest.mark.parametrize("tile", [0, 5, 262143])
@pytest.mark.parametrize("operand", [0, 1])
@pytest.mark.parametrize("fmt", ["bf16", "fp8", "fp4"])
def test_cu_operands(selftest, fmt, operand, tile, seed_index):
    seed = (_seeds()[0], HIGH_SEED)[seed_index]
    out = _numbers(selftest, "cu", fmt, tile, seed, operand)
    K = cr.K[fmt]
    assert out.size == 2 * 16 * K
    codes, nums = out[: 16 * K].reshape(16, K), out[16 * K:].reshape(16, K)
    want = cr.operand_values(fmt, tile, seed, operand)
    assert np.array_equal(_decode(fmt, codes), want)
    assert np.array_equal(nums * gr.GRANULE[fmt], want)


@pytest.mark.parametrize("seed_index", [0, 1])
@pytest.mark.parametrize("operand", [0, 1])
@pytest.mark.parametrize("kind,rng", [("bf16", 127), ("bf16", 64), ("bf16", 1),
                                      ("fp8", 4), ("fp8", 1), ("fp4", 16)])
def test_gemm_operands(selftest, kind, rng, operand, seed_index):
    seed = (_seeds()[1], HIGH_SEED)[seed_index]
    rows, K = 300, 512  # crosses a 256-row tile
    out = _numbers(selftest, "gemm", kind, operand, rows, K, seed, rng)
    assert out.size == 2 * rows * K
    codes, nums = out[: rows * K].reshape(rows, K), out[rows * K:].reshape(rows, K)
    assert np.array_equal(codes, gr.codes(kind, operand, rows, K, seed, rng).astype(np.int64))
    assert np.array_equal(nums, gr.numerators(kind, operand, rows, K, seed, rng))


@pytest.mark.parametrize("base,n", [(0, 64), (2**32 - 5, 16), (2**40 + 3, 9)])
@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("pattern", ["addr", "rand", "zero"])
def test_mem_patterns(selftest, pattern, invert, base, n):
    out = _numbers(selftest, "mem", pattern, mr.SEED, base, n, int(invert), dtype=np.uint64)
    want = mr.pattern_np(mr.arange_np(base, n), pattern, mr.SEED, invert)
    assert out.size == n
    assert np.array_equal(out, want)


@pytest.mark.parametrize("K", [192, 256, 512, 1024, 4096, 8192, 65536])
@pytest.mark.parametrize("kind", ["bf16", "fp8", "fp4"])
def test_exactness(selftest, kind, K):
    from gpu_docker_api_amd.ops.hipcore import gemm_check_range

    rng = gemm_check_range(kind, K)
    assert _run(selftest, "exact", kind, rng, K).strip() == "1"
    if kind != "fp4" and rng + 1 <= FULL_RANGE[kind]:
        assert _run(selftest, "exact", kind, rng + 1, K).strip() == "0"
