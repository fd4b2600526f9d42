"""Checked GEMM loop on a real MI355X (csrc/gemm_check.hip).

Each stage is held against the numpy port of tests/gemm_check_refs.py: the
fills bit for bit, the expected checksums exactly, the verifier's findings as
sets of (tile, row or column). The GEMMs themselves are the shipped 256^2
kernels through their existing bindings, and their results on the generated
operands must also bit-equal the float64 product of the decoded operands.

One case of the issue cannot hold as it is worded. Flipping the LOWEST
mantissa bit of a result changes it by 2^-23 of its magnitude; the sums here
are far below 2^23 product granules, so the flipped value is no integer number
of granules and the verifier (rule: "x is not an integer -> malformed") names
it as a malformed element with its exact coordinates, not as one row and one
column. Both are tested: bit 0 gives one malformed element at the right
place, and the lowest bit that is still worth a whole granule (the smallest
error that is a possible sum) gives one row, one column and the right delta.
"""
import numpy as np
import pytest

import gemm_check_refs as gr
import kernel_refs as kr
from conftest import require_gpu

pytestmark = pytest.mark.gpu

SEED = 0x6E44C4EC5EED0001
SEEDS = (0, SEED)
KINDS = gr.KINDS
BIG = (512, 768, 4608)  # tiles_m != tiles_n; fp8 at its w = 3 limit


@pytest.fixture(scope="module")
def ext():
    require_gpu()
    from gpu_docker_api_amd.ops import hipcore

    return hipcore.load_ext()


def rng_of(kind, K):
    from gpu_docker_api_amd.ops.hipcore import gemm_check_range

    return gemm_check_range(kind, K)


def to_numpy(kind, t):
    import torch

    return (t.view(torch.int16) if kind == "bf16" else t).cpu().numpy()


def run_gemm(ext, kind, A, Bt, K, code=None):
    if kind == "bf16":
        return ext.gemm_bf16_8ph(A, Bt, 0 if code is None else code)
    if kind == "fp8":
        return ext.gemm_fp8_mx(A, Bt, 16 if code is None else code)
    return ext.gemm_fp4_mx(A, Bt, K, 16 if code is None else code)


def int_product(a, b):
    """a @ b.T of integer numerators, through float64 (exact far below 2^53)."""
    return (a.astype(np.float64) @ b.astype(np.float64).T).astype(np.int64)


_problems = {}


def problem(ext, kind, M, N, K, seed=SEED, code=None):
    """One generated problem, computed once and left unchanged: the GEMM's C
    on the GPU, the port's numerators and expected sums."""
    key = (kind, M, N, K, seed, code)
    if key not in _problems:
        r = rng_of(kind, K)
        A = ext.gemm_check_fill(kind, 0, M, K, seed, r)
        Bt = ext.gemm_check_fill(kind, 1, N, K, seed, r)
        a = gr.numerators(kind, 0, M, K, seed, r)
        b = gr.numerators(kind, 1, N, K, seed, r)
        R, Q = gr.expected_sums(a, b)
        _problems[key] = {
            "kind": kind, "K": K, "range": r, "A": A, "Bt": Bt, "a": a, "b": b, "R": R, "Q": Q,
            "C": run_gemm(ext, kind, A, Bt, K, code), "n": int_product(a, b),
            "inv": 1.0 / gr.GRANULE[kind] ** 2,
        }
    return _problems[key]


def granule_flip(p, row, col):
    """(mask, delta) of the lowest fp32 bit of C[row][col] that is worth a
    whole granule: XORing it changes the sum by delta = +-1 granule."""
    n = int(p["n"][row, col])
    assert n != 0
    mask = 1 << (23 - (abs(n).bit_length() - 1))
    bits = np.array([n / p["inv"]], dtype=np.float32).view(np.uint32)
    after = float((bits ^ np.uint32(mask)).view(np.float32)[0]) * p["inv"]
    assert after == int(after) and abs(int(after) - n) == 1
    return mask, int(after) - n


def nonzero_element(p, row, col):
    """The first element at or after (row, col) in its row with a nonzero sum."""
    while int(p["n"][row, col]) == 0:
        col += 1
    return row, col


def xor_bits(C, row, col, mask):
    import torch

    out = C.clone()
    flat = out.view(torch.int32)
    m = mask - (1 << 32) if mask >= 1 << 31 else mask
    flat[row, col] = flat[row, col] ^ m
    return out


def findings(raw):
    rows = sorted((r["tile_row"], r["tile_col"], r["index"]) for r in raw["records"]
                  if r["type"] == "row")
    cols = sorted((r["tile_row"], r["tile_col"], r["index"]) for r in raw["records"]
                  if r["type"] == "col")
    bad = sorted((r["tile_row"] * 256 + r["row"], r["tile_col"] * 256 + r["col"])
                 for r in raw["records"] if r["type"] == "malformed")
    return {"malformed": bad, "rows": rows, "cols": cols}


def verify(ext, p, C, seed=SEED, max_records=64):
    return ext.gemm_check_verify(p["kind"], C, p["K"], seed, p["range"], max_records)


def assert_matches_port(p, C, raw):
    """Device findings == the port's classification of the same array."""
    want = gr.classify(C.cpu().numpy(), p["inv"], p["R"], p["Q"])
    assert findings(raw) == {k: sorted(v) for k, v in want.items()}
    assert raw["errors"] == {k: len(v) for k, v in want.items()}


# ---------------------------------------------------------------------------
# stages
# ---------------------------------------------------------------------------

def test_geometry(ext):
    g = ext.gemm_check_geometry()
    assert list(g["kinds"]) == list(KINDS)
    assert dict(g["kind_index"]) == gr.FMT_INDEX
    assert dict(g["min_k"]) == gr.MIN_K
    assert dict(g["default_code"]) == {"bf16": 0, "fp8": 16, "fp4": 16}
    assert {k: 1.0 / v for k, v in dict(g["inverse_granule"]).items()} == {
        k: gr.GRANULE[k] ** 2 for k in KINDS}
    assert g["tile"] == 256 and g["strip_rows"] * g["strips"] == 256
    assert g["poison_bits"] == gr.POISON_BITS and g["max_inject"] == 64
    assert g["default_loop"] == "serial" and set(g["loops"]) >= {"serial", "overlap"}


@pytest.mark.parametrize("seed", SEEDS, ids=["seed0", "seed"])
@pytest.mark.parametrize("big_k", [False, True], ids=["min-k", "k4096"])
@pytest.mark.parametrize("kind", KINDS)
def test_fill_equals_the_port(ext, kind, big_k, seed):
    K = 4096 if big_k else gr.MIN_K[kind]
    r = rng_of(kind, K)
    for operand in (0, 1):
        got = to_numpy(kind, ext.gemm_check_fill(kind, operand, 256, K, seed, r))
        want = gr.stored(kind, gr.codes(kind, operand, 256, K, seed, r))
        assert got.shape == want.shape and got.dtype == want.dtype
        assert np.array_equal(got, want), (kind, K, operand)


def test_fill_rejects_a_range_that_is_not_exact(ext):
    for kind, K, r in (("bf16", 4096, 65), ("bf16", 256, 128), ("fp8", 4736, 3), ("fp8", 256, 5),
                       ("fp4", 512, 8), ("fp16", 256, 1)):
        with pytest.raises(RuntimeError):
            ext.gemm_check_fill(kind, 0, 256, K, SEED, r)
    with pytest.raises(RuntimeError):
        ext.gemm_check_fill("bf16", 2, 256, 256, SEED, 127)


@pytest.mark.parametrize("shape", [(512, 768), (256, 256)], ids=["512x768", "256x256"])
@pytest.mark.parametrize("kind", KINDS)
def test_expected_sums_equal_the_port(ext, kind, shape):
    M, N = shape
    K = gr.MIN_K[kind] if M == 256 else 2304
    r = rng_of(kind, K)
    R, Q = ext.gemm_check_expected(kind, M, N, K, SEED, r)
    wantR, wantQ = gr.expected_sums(gr.numerators(kind, 0, M, K, SEED, r),
                                    gr.numerators(kind, 1, N, K, SEED, r))
    assert tuple(R.shape) == tuple(Q.shape) == (M // 256, N // 256, 256)
    assert np.array_equal(R.cpu().numpy(), wantR)
    assert np.array_equal(Q.cpu().numpy(), wantQ)


@pytest.mark.parametrize("big", [False, True], ids=["one-tile", "512x768"])
@pytest.mark.parametrize("kind", KINDS)
def test_clean_gemm_verifies_clean(ext, kind, big):
    import torch

    M, N, K = BIG if big else (256, 256, gr.MIN_K[kind])
    p = problem(ext, kind, M, N, K)
    g = gr.GRANULE[kind]
    m = gr.max_numerator(kind, p["range"]) * g
    assert kr.exact_condition(m, m, K, g, g) <= 2**24
    ref = torch.from_numpy(p["n"].astype(np.float64) / p["inv"])
    kr.assert_exact(p["C"], ref)
    raw = verify(ext, p, p["C"])
    assert raw["errors"] == {"rows": 0, "cols": 0, "malformed": 0} and raw["records"] == []


# ---------------------------------------------------------------------------
# verify detects and locates
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_one_granule_off_is_one_row_one_column_and_the_delta(ext, kind):
    from gpu_docker_api_amd.ops.hipcore import gemm_check_fold

    p = problem(ext, kind, *BIG)
    row, col = nonzero_element(p, 300, 515)
    mask, delta = granule_flip(p, row, col)
    C = xor_bits(p["C"], row, col, mask)
    raw = verify(ext, p, C)
    assert raw["errors"] == {"rows": 1, "cols": 1, "malformed": 0}
    assert_matches_port(p, C, raw)
    (tile,) = gemm_check_fold(raw, 3, 6, False)["bad_tiles"]
    assert tile["tile"] == [1, 2] and tile["iter"] == 0
    assert tile["element"] == {"row": row, "col": col, "delta": delta}
    assert tile["rows"][0]["got"] - tile["rows"][0]["want"] == delta
    assert tile["rows"][0]["want"] == int(p["R"][1, 2, row - 256])
    assert tile["cols"][0]["want"] == int(p["Q"][1, 2, col - 512])


@pytest.mark.parametrize("what", ["mantissa-bit-0", "exponent-bit", "nan"])
@pytest.mark.parametrize("kind", KINDS)
def test_a_value_that_is_no_possible_sum_is_malformed(ext, kind, what):
    import torch

    p = problem(ext, kind, *BIG)
    row, col = nonzero_element(p, 17, 700)
    if what == "nan":
        C = p["C"].clone()
        C[row, col] = float("nan")
    else:
        C = xor_bits(p["C"], row, col, 1 if what == "mantissa-bit-0" else 0x40000000)
    raw = verify(ext, p, C)
    assert raw["errors"]["malformed"] == 1
    assert findings(raw)["malformed"] == [(row, col)]
    (rec,) = [r for r in raw["records"] if r["type"] == "malformed"]
    assert rec["bits"] == int(C.view(torch.int32)[row, col]) & 0xFFFFFFFF
    assert_matches_port(p, C, raw)  # its row and column miss its value


@pytest.mark.parametrize("kind", KINDS)
def test_last_element_of_the_last_tile(ext, kind):
    from gpu_docker_api_amd.ops.hipcore import gemm_check_fold

    p = problem(ext, kind, *BIG)
    M, N, _ = BIG
    if int(p["n"][M - 1, N - 1]) == 0:
        C = p["C"].clone()
        C[M - 1, N - 1] = 1.0 / p["inv"]
        delta = 1
    else:
        mask, delta = granule_flip(p, M - 1, N - 1)
        C = xor_bits(p["C"], M - 1, N - 1, mask)
    raw = verify(ext, p, C)
    assert findings(raw) == {"malformed": [], "rows": [(1, 2, 255)], "cols": [(1, 2, 255)]}
    (tile,) = gemm_check_fold(raw, 3, 6, False)["bad_tiles"]
    assert tile["element"] == {"row": M - 1, "col": N - 1, "delta": delta}
    assert (tile["block"], tile["block_mod8"]) == kr.owner_block(1, 2, 3, 6, False)


@pytest.mark.parametrize("kind", KINDS)
def test_two_elements_in_one_tile(ext, kind):
    from gpu_docker_api_amd.ops.hipcore import gemm_check_fold

    p = problem(ext, kind, *BIG)
    C = p["C"]
    spots = [nonzero_element(p, 3, 260), nonzero_element(p, 200, 300)]
    for row, col in spots:
        C = xor_bits(C, row, col, granule_flip(p, row, col)[0])
    raw = verify(ext, p, C)
    assert raw["errors"] == {"rows": 2, "cols": 2, "malformed": 0}
    assert findings(raw)["rows"] == [(0, 1, 3), (0, 1, 200)]
    assert findings(raw)["cols"] == sorted((0, 1, c - 256) for _, c in spots)
    (tile,) = gemm_check_fold(raw, 3, 6, False)["bad_tiles"]
    assert "element" not in tile and len(tile["rows"]) == len(tile["cols"]) == 2


@pytest.mark.parametrize("kind", KINDS)
def test_result_of_another_seed_is_bad_everywhere(ext, kind):
    p = problem(ext, kind, *BIG)
    M, N, K = BIG
    other = 12345
    raw = verify(ext, p, p["C"], seed=other, max_records=16)
    R, Q = gr.expected_sums(gr.numerators(kind, 0, M, K, other, p["range"]),
                            gr.numerators(kind, 1, N, K, other, p["range"]))
    want = gr.classify(p["C"].cpu().numpy(), p["inv"], R, Q)
    assert raw["errors"] == {k: len(v) for k, v in want.items()}  # counted, never capped
    assert raw["errors"]["rows"] > 0.99 * M * 3 and raw["errors"]["cols"] > 0.99 * N * 2
    assert {(t[0], t[1]) for t in want["rows"]} == {(i, j) for i in range(2) for j in range(3)}
    assert len(raw["records"]) == 16
    for rec in raw["records"]:
        key = (rec["tile_row"], rec["tile_col"], rec["index"])
        assert key in (want["rows"] if rec["type"] == "row" else want["cols"])


def test_an_unwritten_result_is_malformed_everywhere(ext):
    import torch

    p = problem(ext, "fp4", 256, 256, gr.MIN_K["fp4"])
    C = torch.full((256, 256), float("nan"), device="cuda")
    C.view(torch.int32).fill_(gr.POISON_BITS)
    raw = verify(ext, p, C, max_records=8)
    assert raw["errors"]["malformed"] == 256 * 256 and len(raw["records"]) == 8


def test_verify_rejects_bad_arguments(ext):
    import torch

    p = problem(ext, "fp4", 256, 256, gr.MIN_K["fp4"])
    for C in (p["C"][:, :128], p["C"].double(), p["C"].cpu(), p["C"][:128]):
        with pytest.raises(RuntimeError):
            verify(ext, p, C)
    with pytest.raises(RuntimeError):
        verify(ext, p, p["C"], max_records=1 << 20)
    assert torch.cuda.current_device() == 0


# ---------------------------------------------------------------------------
# driver
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("loop", ["overlap", "serial", "serial-atomic"])
@pytest.mark.parametrize("kind", KINDS)
def test_driver_clean(ext, kind, loop):
    import torch

    before = torch.cuda.current_device()
    raw = ext.gemm_check(0, kind, 512, 3, SEED, rng_of(kind, 512), -1, 32, [], loop)
    assert raw["errors"] == {"rows": 0, "cols": 0, "malformed": 0} and raw["records"] == []
    assert raw["operand_errors"] == 0 and raw["iters"] == 3
    assert raw["checked_bytes"] == 3 * 4 * 512 * 512
    assert raw["seconds"] > 0 and raw["tflops"] > 0
    assert raw["code"] == {"bf16": 0, "fp8": 16, "fp4": 16}[kind] and raw["loop"] == loop
    assert torch.cuda.current_device() == before


def test_xcd_remap_attributes_to_the_owning_block(ext):
    from gpu_docker_api_amd.ops.hipcore import gemm_check_fold

    # bf16 code 1 on 3 x 5 tiles: nwg = 15 = 8 * 1 + 7, a ragged XCD split
    p = problem(ext, "bf16", 768, 1280, 192, code=1)
    raw = verify(ext, p, p["C"])
    assert raw["errors"] == {"rows": 0, "cols": 0, "malformed": 0}
    row, col = nonzero_element(p, 2 * 256 + 9, 3 * 256 + 1)
    mask, delta = granule_flip(p, row, col)
    raw = verify(ext, p, xor_bits(p["C"], row, col, mask))
    (tile,) = gemm_check_fold(raw, 5, 15, True)["bad_tiles"]
    assert tile["tile"] == [2, 3] and tile["element"] == {"row": row, "col": col, "delta": delta}
    assert (tile["block"], tile["block_mod8"]) == kr.owner_block(2, 3, 5, 15, True)
    assert kr.block_tile(tile["block"], 5, 15, True) == (2, 3)
    assert tile["block"] != gemm_check_fold(raw, 5, 15, False)["bad_tiles"][0]["block"]


@pytest.mark.parametrize("loop", ["overlap", "serial", "serial-atomic"])
@pytest.mark.parametrize("kind", KINDS)
def test_driver_inject_is_found_at_its_iteration_and_nowhere_else(ext, kind, loop):
    from gpu_docker_api_amd.ops.hipcore import gemm_check_fold

    size, r = 512, rng_of(kind, 512)
    p = {"n": int_product(gr.numerators(kind, 0, size, size, SEED, r),
                          gr.numerators(kind, 1, size, size, SEED, r)),
         "inv": 1.0 / gr.GRANULE[kind] ** 2}
    row, col = nonzero_element(p, 300, 40)
    mask, delta = granule_flip(p, row, col)
    raw = ext.gemm_check(0, kind, size, 3, SEED, r, -1, 32, [[1, row, col, mask]], loop)
    assert raw["errors"] == {"rows": 1, "cols": 1, "malformed": 0}
    assert raw["operand_errors"] == 0
    # buffer 1 of the double-buffered loop carries the error: iterations 0 and
    # 2 (buffer 0) must not see it
    assert sorted(rec["iter"] for rec in raw["records"]) == [1, 1]
    (tile,) = gemm_check_fold(raw, 2, 4, False)["bad_tiles"]
    assert tile["iter"] == 1 and tile["tile"] == [1, 0]
    assert tile["element"] == {"row": row, "col": col, "delta": delta}
    assert (tile["block"], tile["block_mod8"]) == kr.owner_block(1, 0, 2, 4, False) == (2, 2)


def test_driver_rejects_bad_inject_and_arguments(ext):
    ok = [1, 5, 5, 1]
    for bad in ([[3, 5, 5, 1]], [[-1, 5, 5, 1]], [[1, 512, 5, 1]], [[1, 5, 512, 1]],
                [[1, 5, -1, 1]], [[1, 5, 5, 1 << 32]], [[1, 5, 5, -1]], [[1, 5, 5]],
                [ok] * 65):
        with pytest.raises(RuntimeError):
            ext.gemm_check(0, "bf16", 512, 3, SEED, 127, -1, 32, bad)
    with pytest.raises(RuntimeError):  # the unchecked loop takes no entries
        ext.gemm_check(0, "bf16", 512, 3, SEED, 127, -1, 32, [ok], "unchecked")
    for args in ((0, "bf16", 512, 0, SEED, 127), (0, "bf16", 500, 3, SEED, 127),
                 (0, "fp4", 256, 3, SEED, 16), (0, "bf16", 4096, 3, SEED, 127),
                 (99, "bf16", 512, 3, SEED, 127), (0, "bf16", 512, 3, SEED, 127, 8),
                 (0, "fp8", 512, 3, SEED, 4, 0)):
        with pytest.raises(RuntimeError):
            ext.gemm_check(*args)


def test_validate_end_to_end(ext):
    from gpu_docker_api_amd.ops import hipcore

    g = hipcore.validate_gpus(indices=[0], size=2048, iters=3, gemm_check_iters=2)["gpus"][0]
    gc = g["gemm_check"]
    assert gc["size"] == 2048 and gc["iters"] == 2 and gc["errors_total"] == 0
    assert list(gc["formats"]) == ["bf16", "fp8", "fp4"]
    for entry in gc["formats"].values():
        assert entry["errors"] == {"rows": 0, "cols": 0, "malformed": 0}
        assert entry["operand_errors"] == 0 and entry["bad_tiles"] == [] and entry["bands"] == []
        assert entry["checked_bytes"] == 2 * 4 * 2048 * 2048 and entry["tflops"] > 0
    assert g["healthy"] is True
