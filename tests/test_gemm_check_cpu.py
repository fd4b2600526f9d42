"""Checked GEMM loop, everything that needs no GPU: the operand ranges and
their exactness, the generator ports, the owner map, the fold, the
validate_gpus wiring, the route field and the CLI flag."""
import numpy as np
import pytest

import gemm_check_refs as gr
import kernel_refs as kr
from test_memtest_cpu import StubExt, _cli, client, recording_daemon  # noqa: F401

URL = "/api/v1/resources/gpus/validate"
SEEDS = (0, 0x6E44C4EC5EED0001)


# ---------------------------------------------------------------------------
# ranges
# ---------------------------------------------------------------------------

def test_range_boundaries():
    from gpu_docker_api_amd.ops.hipcore import gemm_check_range as rng

    assert [rng("bf16", k) for k in (192, 1024, 1040, 1041, 4096, 4097, 8192, 8193,
                                     16384, 16385)] == [127, 127, 127, 126, 64, 63, 45, 45, 32, 31]
    # one step past each e4m3 boundary, in K and in the kernel's K granularity
    assert [rng("fp8", k) for k in (256, 1152, 1165, 1166, 1280, 4608, 4660, 4661, 4736,
                                    16384, 18641, 18642)] == [4, 4, 4, 3, 3, 3, 3, 2, 2, 2, 2, 1]
    assert [rng("fp4", k) for k in (512, 4096, 16384)] == [16, 16, 16]
    for kind, k in (("bf16", 0), ("bf16", (1 << 24) + 1), ("fp8", 74566), ("fp4", 116509),
                    ("fp16", 256)):
        with pytest.raises(ValueError):
            rng(kind, k)


@pytest.mark.parametrize("kind", gr.KINDS)
def test_chosen_range_is_exact_and_the_largest(kind):
    from gpu_docker_api_amd.ops.hipcore import gemm_check_range as rng

    g = gr.GRANULE[kind]
    top = {"bf16": 127, "fp8": 4, "fp4": 16}[kind]
    for K in range(64, 16384 + 1, 64):
        r = rng(kind, K)
        m = gr.max_numerator(kind, r) * g
        assert kr.exact_condition(m, m, K, g, g) <= 2**24, (kind, K, r)
        if r < top:  # the next larger set would not be exact
            m = gr.max_numerator(kind, r + 1) * g
            assert kr.exact_condition(m, m, K, g, g) > 2**24, (kind, K, r)


# ---------------------------------------------------------------------------
# generator ports
# ---------------------------------------------------------------------------

def test_e4m3_codes_of_range():
    assert np.array_equal(gr.e4m3_codes_of_range(4), kr.E4M3_EXACT_CODES)
    for w in (1, 2, 3, 4):
        c = gr.e4m3_codes_of_range(w)
        assert len(c) == 16 * w + 1 == len(set(c.tolist()))
        assert set(((c[1:] >> 3) & 0xF).tolist()) == set(range(6, 6 + w))
        assert float(np.abs(kr.E4M3_LUT[c]).max()) * 16 == 15 << (w - 1)


@pytest.mark.parametrize("kind,rng", [("bf16", 127), ("bf16", 64), ("bf16", 32), ("fp8", 4),
                                      ("fp8", 3), ("fp8", 2), ("fp4", 16)])
def test_generated_operands_stay_in_the_stated_sets(kind, rng):
    for seed in SEEDS:
        for operand in (0, 1):
            c = gr.codes(kind, operand, 64, 512, seed, rng)
            n = gr.numerators(kind, operand, 64, 512, seed, rng)
            v = gr.decode(kind, c)
            assert np.array_equal(v, n * gr.GRANULE[kind])
            assert int(np.abs(n).max()) == gr.max_numerator(kind, rng)  # the set is used up
            if kind == "fp8":
                assert set(c.ravel().tolist()) == set(gr.e4m3_codes_of_range(rng).tolist())
            if kind == "fp4":
                assert set(c.ravel().tolist()) == set(range(16))
            if kind == "bf16":
                assert set(n.ravel().tolist()) == set(range(-rng, rng + 1))


def test_elements_do_not_depend_on_the_extents():
    for kind in gr.KINDS:
        small = gr.codes(kind, 1, 8, 64, SEEDS[1], 2 if kind == "fp8" else 16)
        large = gr.codes(kind, 1, 24, 256, SEEDS[1], 2 if kind == "fp8" else 16)
        assert np.array_equal(small, large[:8, :64])
    a = gr.codes("bf16", 0, 8, 64, SEEDS[1], 16)
    assert not np.array_equal(a, gr.codes("bf16", 1, 8, 64, SEEDS[1], 16))
    assert not np.array_equal(a, gr.codes("bf16", 0, 8, 64, SEEDS[0], 16))


def test_expected_sums_are_the_checksums_of_the_product():
    a = gr.numerators("fp8", 0, 512, 128, SEEDS[1], 4)
    b = gr.numerators("fp8", 1, 768, 128, SEEDS[1], 4)
    R, Q = gr.expected_sums(a, b)
    assert R.shape == Q.shape == (2, 3, 256)
    c = (a @ b.T).reshape(2, 256, 3, 256)
    assert np.array_equal(R, c.sum(axis=3).transpose(0, 2, 1))
    assert np.array_equal(Q, c.sum(axis=1))
    C = (a @ b.T).astype(np.float32) / np.float32(256)
    assert gr.classify(C, 256.0, R, Q) == {"malformed": [], "rows": [], "cols": []}
    C[300, 700] += np.float32(1 / 256)
    C[5, 5] = np.float32("nan")
    C[6, 6] = np.float32(1 / 512)  # not an integer number of granules
    C[7, 7] = np.float32(2.0 ** 17)  # 2^25 granules
    got = gr.classify(C, 256.0, R, Q)
    assert got["malformed"] == [(5, 5), (6, 6), (7, 7)]
    assert (1, 2, 300 - 256) in got["rows"] and (1, 2, 700 - 512) in got["cols"]


# ---------------------------------------------------------------------------
# helpers of the verifier and operand-check tests
# ---------------------------------------------------------------------------

def test_verify_class_is_a_bijection_with_three_values_by_hand():
    # row 150 = 2 * 64 + 22 = 2 * 64 + 1 * 16 + 6; col 77 = 19 * 4 + 1
    assert tuple(gr.verify_class(150, 77)) == (2, 1, 6, 19, 1)
    assert tuple(gr.verify_class(0, 0)) == (0, 0, 0, 0, 0)
    assert tuple(gr.verify_class(255, 255)) == (3, 3, 15, 63, 3)
    seen = set()
    for row in range(256):
        for col in range(256):
            k = gr.verify_class(row, col)
            assert 0 <= k.strip < 4 and 0 <= k.wave < 4 and 0 <= k.j < 16
            assert 0 <= k.lane < 64 and 0 <= k.e < 4
            assert k.c == col and 64 * k.strip + 16 * k.wave + k.j == row
            seen.add(tuple(k))
    assert len(seen) == 4 * 4 * 16 * 64 * 4 == 256 * 256
    for bad in ((256, 0), (0, 256), (-1, 0)):
        with pytest.raises(ValueError):
            gr.verify_class(*bad)


def test_operand_diff_count_counts_elements():
    a = np.zeros((2, 8), dtype=np.uint8)
    b = a.copy()
    b[1, 3] = 0x21  # one byte, both nibbles changed
    assert gr.operand_diff_count("fp4", a, b) == 2
    assert gr.operand_diff_count("fp8", a, b) == 1
    b[0, 0] = 0x30  # a high nibble alone, then a low nibble alone
    b[0, 7] = 0x03
    assert gr.operand_diff_count("fp4", a, b) == 4
    assert gr.operand_diff_count("fp8", a, b) == 3
    assert gr.operand_diff_count("fp4", a, a) == gr.operand_diff_count("fp8", a, a) == 0
    w = np.zeros((2, 8), dtype=np.int16)
    v = w.copy()
    v[0, 1] = -32768  # the sign bit alone
    v[1, 7] = 0x0101  # both bytes of one word
    assert gr.operand_diff_count("bf16", w, v) == 2
    with pytest.raises(ValueError):
        gr.operand_diff_count("fp8", a, a[:1])


@pytest.mark.parametrize("kind,rng", [("bf16", 127), ("bf16", 90), ("bf16", 1), ("fp8", 4),
                                      ("fp8", 3), ("fp8", 1), ("fp4", 16)])
def test_legal_other_code_stays_in_the_set_and_differs(kind, rng):
    if kind == "bf16":
        legal = kr.f32_to_bf16_bits(
            (np.arange(-rng, rng + 1) / 16.0).astype(np.float32)).tolist()
    elif kind == "fp8":
        legal = gr.e4m3_codes_of_range(rng).tolist()
    else:
        legal = list(range(16))
    others = [gr.legal_other_code(kind, c, rng) for c in legal]
    assert all(o in legal for o in others)
    assert all(o != c for o, c in zip(others, legal))
    # and in value, so that a sum through it moves (e2m1 +0 and -0 aside,
    # which the other mantissa bit never maps onto each other)
    code_t = np.uint16 if kind == "bf16" else np.uint8
    assert np.all(gr.decode(kind, np.array(others, dtype=code_t))
                  != gr.decode(kind, np.array(legal, dtype=code_t)))
    if kind == "bf16":
        with pytest.raises(ValueError):
            gr.legal_other_code(kind, 0x3F81, rng)  # 1 + 2^-7: no sixteenth


# ---------------------------------------------------------------------------
# owner map
# ---------------------------------------------------------------------------

def test_owner_equals_kernel_refs_for_every_grid():
    from gpu_docker_api_amd.ops.hipcore import gemm_check_owner

    for nwg in range(1, 2049):
        tiles_n = next(d for d in (7, 5, 4, 3, 2, 1) if nwg % d == 0)
        for remap in (False, True):
            got = [gemm_check_owner(t // tiles_n, t % tiles_n, tiles_n, nwg, remap)
                   for t in range(nwg)]
            if nwg <= 64 or nwg % 97 == 0:  # the reference inverse is quadratic: sample
                want = [kr.owner_block(t // tiles_n, t % tiles_n, tiles_n, nwg, remap)
                        for t in range(nwg)]
                assert got == want, (nwg, remap)
            # every grid: a bijection that inverts the kernel's forward map
            assert sorted(b for b, _ in got) == list(range(nwg))
            for t, (bid, mod8) in enumerate(got):
                assert mod8 == bid % 8
                assert kr.block_tile(bid, tiles_n, nwg, remap) == (t // tiles_n, t % tiles_n)
    with pytest.raises(ValueError):
        gemm_check_owner(2, 0, 2, 4, False)


# ---------------------------------------------------------------------------
# fold
# ---------------------------------------------------------------------------

def rec_sum(kind, it, tr, tc, index, got, want):
    return {"type": kind, "iter": it, "tile_row": tr, "tile_col": tc, "index": index,
            "got": got, "want": want}


def raw_of(records, rows=None, cols=None, malformed=None):
    count = lambda t: sum(r["type"] == t for r in records)  # noqa: E731
    return {"records": records,
            "errors": {"rows": count("row") if rows is None else rows,
                       "cols": count("col") if cols is None else cols,
                       "malformed": count("malformed") if malformed is None else malformed}}


def test_fold_clean():
    from gpu_docker_api_amd.ops.hipcore import gemm_check_fold

    out = gemm_check_fold(raw_of([]), 4, 16, False)
    assert out == {"errors": {"rows": 0, "cols": 0, "malformed": 0}, "bad_tiles": [],
                   "bands": [], "by_block_mod8": [0] * 8, "records_truncated": False}


def test_fold_pins_one_element():
    from gpu_docker_api_amd.ops.hipcore import gemm_check_fold

    recs = [rec_sum("col", 1, 2, 3, 17, -40, -41), rec_sum("row", 1, 2, 3, 200, 1001, 1000)]
    out = gemm_check_fold(raw_of(recs), 4, 16, False)
    assert out["bad_tiles"] == [{
        "iter": 1, "tile": [2, 3], "block": 11, "block_mod8": 3,
        "rows": [{"row": 200, "got": 1001, "want": 1000}],
        "cols": [{"col": 17, "got": -40, "want": -41}],
        "malformed": [],
        "element": {"row": 2 * 256 + 200, "col": 3 * 256 + 17, "delta": 1},
    }]
    assert out["by_block_mod8"] == [0, 0, 0, 1, 0, 0, 0, 0]
    assert out["bands"] == [] and out["records_truncated"] is False
    # with the XCD remap another workgroup computed that tile
    out = gemm_check_fold(raw_of(recs), 4, 16, True)
    assert (out["bad_tiles"][0]["block"], out["bad_tiles"][0]["block_mod8"]) == \
        kr.owner_block(2, 3, 4, 16, True)
    # unequal deltas: one row and one column, but not one element
    recs[0]["got"] = -39
    assert "element" not in gemm_check_fold(raw_of(recs), 4, 16, False)["bad_tiles"][0]


def test_fold_two_elements_in_one_tile_pins_none():
    from gpu_docker_api_amd.ops.hipcore import gemm_check_fold

    recs = [rec_sum("row", 0, 0, 0, 1, 5, 4), rec_sum("row", 0, 0, 0, 9, 8, 7),
            rec_sum("col", 0, 0, 0, 2, 5, 4), rec_sum("col", 0, 0, 0, 3, 8, 7)]
    out = gemm_check_fold(raw_of(recs), 2, 4, False)
    (tile,) = out["bad_tiles"]
    assert "element" not in tile
    assert [r["row"] for r in tile["rows"]] == [1, 9] and [c["col"] for c in tile["cols"]] == [2, 3]
    # the same element in two iterations is two tiles, each pinned
    recs = [rec_sum("row", i, 0, 1, 1, 5, 4) for i in (0, 2)] + \
           [rec_sum("col", i, 0, 1, 2, 5, 4) for i in (0, 2)]
    out = gemm_check_fold(raw_of(recs), 2, 4, False)
    assert [(t["iter"], t["element"]) for t in out["bad_tiles"]] == [
        (0, {"row": 1, "col": 258, "delta": 1}), (2, {"row": 1, "col": 258, "delta": 1})]


def test_fold_reports_malformed():
    from gpu_docker_api_amd.ops.hipcore import gemm_check_fold

    recs = [{"type": "malformed", "iter": 3, "tile_row": 1, "tile_col": 0, "row": 255, "col": 7,
             "bits": gr.POISON_BITS},
            rec_sum("row", 3, 1, 0, 255, 9, 10), rec_sum("col", 3, 1, 0, 7, 0, 1)]
    out = gemm_check_fold(raw_of(recs), 2, 4, False)
    (tile,) = out["bad_tiles"]
    assert tile["malformed"] == [{"row": 255, "col": 7, "bits": gr.POISON_BITS}]
    assert "element" not in tile  # a malformed element is named by itself, never by a delta
    assert out["errors"] == {"rows": 1, "cols": 1, "malformed": 1}


def test_fold_reports_a_band_and_counts_per_block_mod8():
    from gpu_docker_api_amd.ops.hipcore import gemm_check_fold

    # a flipped word of A: row 5 of tile row 2 is wrong in every tile column
    tiles_n, nwg = 5, 15
    recs = [rec_sum("row", 0, 2, tc, 5, 3, 2) for tc in range(tiles_n)]
    recs += [rec_sum("col", 0, 2, tc, c, 3, 2) for tc in range(tiles_n) for c in (0, 1)]
    recs.append(rec_sum("row", 1, 0, 4, 0, 1, 0))  # and one lone tile later on
    out = gemm_check_fold(raw_of(recs), tiles_n, nwg, False)
    assert out["bands"] == [{"iter": 0, "axis": "row", "index": 2, "tiles": 5}]
    assert [t["tile"] for t in out["bad_tiles"]] == [[2, 0], [2, 1], [2, 2], [2, 3], [2, 4], [0, 4]]
    want = [0] * 8
    for t in (10, 11, 12, 13, 14, 4):
        want[t % 8] += 1
    assert out["by_block_mod8"] == want
    # a column band, under the remap
    recs = [rec_sum("col", 0, tr, 1, 9, 3, 2) for tr in range(3)]
    out = gemm_check_fold(raw_of(recs), tiles_n, nwg, True)
    assert out["bands"] == [{"iter": 0, "axis": "col", "index": 1, "tiles": 3}]
    want = [0] * 8
    for tr in range(3):
        want[kr.owner_block(tr, 1, tiles_n, nwg, True)[1]] += 1
    assert out["by_block_mod8"] == want


def test_fold_says_when_records_were_capped():
    from gpu_docker_api_amd.ops.hipcore import gemm_check_fold

    out = gemm_check_fold(raw_of([rec_sum("row", 0, 0, 0, 1, 5, 4)], rows=4096, cols=4096), 2, 4,
                          False)
    assert out["records_truncated"] is True
    assert out["errors"] == {"rows": 4096, "cols": 4096, "malformed": 0}


# ---------------------------------------------------------------------------
# validate_gpus with a stub extension
# ---------------------------------------------------------------------------

class GemmStubExt(StubExt):
    """StubExt plus a gemm_check that reports `bad` (a dict of error counts
    per kind) and is clean otherwise."""

    def __init__(self, bad=None, operand_errors=0):
        super().__init__()
        self.bad = bad or {}
        self.operand_errors = operand_errors
        self.gemm_calls = []

    def gemm_check(self, device, kind, size, iters, seed, rng, code, max_records, inject):
        self.gemm_calls.append((device, kind, size, iters, seed, rng, code, max_records,
                                list(inject)))
        errors = dict({"rows": 0, "cols": 0, "malformed": 0}, **self.bad.get(kind, {}))
        recs = []
        if errors["rows"]:
            recs = [rec_sum("row", 0, 1, 1, 3, 8, 7), rec_sum("col", 0, 1, 1, 4, 8, 7)]
        return {"records": recs, "errors": errors, "operand_errors": self.operand_errors,
                "iters": iters, "seconds": 0.0123456, "tflops": 987.654,
                "checked_bytes": iters * 4 * size * size}


@pytest.fixture
def gemm_stub(monkeypatch):
    from gpu_docker_api_amd.ops import hipcore

    def install(ext=None, **kw):
        ext = ext or GemmStubExt(**kw)
        monkeypatch.setattr(hipcore, "_ext", ext)
        return ext

    return install


def test_validate_without_the_option_is_unchanged_and_never_touches_it(gemm_stub):
    from gpu_docker_api_amd.ops import hipcore

    ext = gemm_stub(ext=StubExt())  # no gemm_check attribute at all
    assert not hasattr(ext, "gemm_check")
    report = hipcore.validate_gpus(size=2048, iters=3)
    assert report == hipcore.validate_gpus(size=2048, iters=3, gemm_check_iters=0)
    assert list(report["gpus"][0]) == [
        "index", "hbm_gbps", "bf16_tflops", "fp8_tflops", "fp4_tflops", "healthy"]
    assert report["gpus"][0]["healthy"] is True
    with pytest.raises(AttributeError):  # and with the option it is the extension's call
        hipcore.validate_gpus(size=2048, iters=3, gemm_check_iters=1)


def test_validate_gemm_check_clean_keeps_healthy(gemm_stub):
    from gpu_docker_api_amd.ops import hipcore

    ext = gemm_stub()
    g = hipcore.validate_gpus(size=2048, iters=3, gemm_check_iters=4)["gpus"][0]
    assert list(g) == ["index", "hbm_gbps", "bf16_tflops", "fp8_tflops", "fp4_tflops",
                       "gemm_check", "healthy"]
    assert g["healthy"] is True
    gc = g["gemm_check"]
    assert gc["size"] == 2048 and gc["iters"] == 4 and gc["errors_total"] == 0
    assert list(gc["formats"]) == ["bf16", "fp8", "fp4"]
    for kind, entry in gc["formats"].items():
        assert entry["errors"] == {"rows": 0, "cols": 0, "malformed": 0}
        assert entry["operand_errors"] == 0 and entry["bad_tiles"] == []
        assert entry["tflops"] == 987.7 and entry["seconds"] == 0.0123
        assert entry["checked_bytes"] == 4 * 4 * 2048 * 2048
    assert [(c[0], c[1], c[2], c[3], c[5], c[6], c[8]) for c in ext.gemm_calls] == [
        (0, "bf16", 2048, 4, 90, 0, []), (0, "fp8", 2048, 4, 3, 16, []),
        (0, "fp4", 2048, 4, 16, 16, [])]
    assert all(0 <= c[4] < 2**64 for c in ext.gemm_calls)


def test_validate_gemm_check_sits_after_cu_check_and_skips_fp4_below_512(gemm_stub):
    from gpu_docker_api_amd.ops import hipcore
    from test_cu_check_cpu import CuStubExt

    class Both(GemmStubExt, CuStubExt):
        def __init__(self):
            CuStubExt.__init__(self)
            self.bad, self.operand_errors, self.gemm_calls = {}, 0, []

    gemm_stub(ext=Both())
    g = hipcore.validate_gpus(size=256, iters=3, cu_rounds=2, gemm_check_iters=1)["gpus"][0]
    keys = list(g)
    assert keys.index("gemm_check") == keys.index("cu_check") + 1
    assert list(g["gemm_check"]["formats"]) == ["bf16", "fp8"]


@pytest.mark.parametrize("kw", [{"bad": {"fp8": {"rows": 1, "cols": 1}}},
                                {"bad": {"fp4": {"malformed": 2}}},
                                {"operand_errors": 3}], ids=["sums", "malformed", "operands"])
def test_validate_gemm_check_errors_mark_unhealthy(gemm_stub, kw):
    from gpu_docker_api_amd.ops import hipcore

    gemm_stub(**kw)
    g = hipcore.validate_gpus(size=2048, iters=3, gemm_check_iters=2)["gpus"][0]
    assert g["gemm_check"]["errors_total"] > 0
    assert g["healthy"] is False
    if "bad" in kw and "fp8" in kw["bad"]:
        (tile,) = g["gemm_check"]["formats"]["fp8"]["bad_tiles"]
        assert tile["element"] == {"row": 256 + 3, "col": 256 + 4, "delta": 1}
        assert (tile["block"], tile["block_mod8"]) == (9, 1)
        assert g["gemm_check"]["formats"]["bf16"]["bad_tiles"] == []


def test_validate_async_forwards_gemm_check_iters(gemm_stub, run):
    from gpu_docker_api_amd.ops import hipcore

    ext = gemm_stub()
    report = run(hipcore.validate_gpus_async(None, 2048, 3, gemm_check_iters=7))
    assert report["gpus"][0]["gemm_check"]["iters"] == 7
    assert [c[3] for c in ext.gemm_calls] == [7, 7, 7]


# ---------------------------------------------------------------------------
# route
# ---------------------------------------------------------------------------

@pytest.fixture
def validate_kwargs(monkeypatch):
    """Records the keyword arguments the route passes, so an absent kwarg
    stays visible as absent."""
    from gpu_docker_api_amd.ops import hipcore

    calls = []

    async def fake(indices=None, size=4096, iters=5, **kw):
        calls.append(kw)
        return {"gpus": []}

    monkeypatch.setattr(hipcore, "validate_gpus_async", fake)
    return calls


def test_route_gemm_check_non_int_is_invalid_params(client, validate_kwargs):
    from gpu_docker_api_amd.routers.codes import Code

    for value in ("x", "8", 1.5, None, [1], True, False):
        r = client.post(URL, json={"gemmCheck": value})
        assert r.json()["code"] == int(Code.INVALID_PARAMS), value
    assert validate_kwargs == []


def test_route_gemm_check_clamped_and_absent_when_off(client, validate_kwargs):
    for body in ({}, {"gemmCheck": 0}, {"gemmCheck": 5}, {"gemmCheck": 10**9}, {"gemmCheck": -3},
                 {"gemmCheck": 2, "cuCheck": 8}):
        assert client.post(URL, json=body).json()["code"] == 200, body
    assert [kw.get("gemm_check_iters", "off") for kw in validate_kwargs] == [
        "off", "off", 5, 100000, 1, 2]
    assert [set(kw) for kw in validate_kwargs] == [
        {"memtest_mib"}, {"memtest_mib"}, {"memtest_mib", "gemm_check_iters"},
        {"memtest_mib", "gemm_check_iters"}, {"memtest_mib", "gemm_check_iters"},
        {"memtest_mib", "gemm_check_iters", "cu_rounds"}]


# ---------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------

def test_cli_gemm_check_flag_only_when_given(recording_daemon):
    port, bodies = recording_daemon
    for args in ((), ("--gemm-check", "20", "--size", "8192"), ("--gemm-check", "0"),
                 ("--gemm-check", "3", "--cu-check", "8")):
        out = _cli(port, "resources", "validate", *args)
        assert out.returncode == 0, out.stderr
    assert bodies == [
        (URL, {"size": 4096, "iters": 5}),
        (URL, {"size": 8192, "iters": 5, "gemmCheck": 20}),
        (URL, {"size": 4096, "iters": 5}),
        (URL, {"size": 4096, "iters": 5, "cuCheck": 8, "gemmCheck": 3}),
    ]
