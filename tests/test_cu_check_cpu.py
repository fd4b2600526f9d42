"""Per-CU compute check, everything that needs no GPU: the generator's
exactness, the fold by CU, the validate_gpus wiring, the route field and the
CLI flag."""
import numpy as np
import pytest

import cu_check_refs as cr
import kernel_refs as kr
from test_memtest_cpu import StubExt, _cli, client, recording_daemon  # noqa: F401

URL = "/api/v1/resources/gpus/validate"
SEEDS = (0, 0x5EEDC0DEC0FFEE11)


# ---------------------------------------------------------------------------
# generator
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["bf16", "fp8", "fp4"])
def test_k_satisfies_exactness_condition(fmt):
    s = kr.EXACT_SETS[cr.EXACT_SET[fmt]]
    assert cr.K[fmt] <= s["k_max"]
    lhs = kr.exact_condition(s["max"], s["max"], cr.K[fmt], s["granule"], s["granule"])
    assert lhs <= 2**24


def test_generated_operands_stay_in_the_exact_sets():
    exact = set(int(c) for c in kr.E4M3_EXACT_CODES)
    for seed in SEEDS:
        for tile in range(32):  # 2 seeds x 32 tiles = 64 tiles
            for operand in (0, 1):
                m = cr.bf16_m(cr.draws("bf16", tile, seed, operand))
                assert int(np.abs(m).max()) <= 127
                v = cr.operand_values("bf16", tile, seed, operand)
                assert np.array_equal(v * 16.0, m.astype(np.float64))
                codes = cr.e4m3_codes(cr.draws("fp8", tile, seed, operand))
                assert set(int(c) for c in np.unique(codes)) <= exact
                v = cr.operand_values("fp8", tile, seed, operand)
                assert float(np.abs(v).max()) <= 7.5 and np.array_equal(v * 16.0, np.round(v * 16.0))
                assert int(cr.e2m1_codes(cr.draws("fp4", tile, seed, operand)).max()) <= 15


def test_e4m3_code_formula_matches_the_exact_code_table():
    assert len(kr.E4M3_EXACT_CODES) == 65
    for j in range(65):
        q = j - 1
        code = 0 if j == 0 else (q >> 5) << 7 | (6 + ((q & 31) >> 3)) << 3 | (q & 7)
        assert code == int(kr.E4M3_EXACT_CODES[j]), j


def test_reference_tiles_are_exact_in_fp32_and_differ():
    seen = set()
    for fmt in ("bf16", "fp8", "fp4"):
        for tile in (0, 1, 1023):
            ref = cr.reference_tile(fmt, tile, SEEDS[0])
            assert ref.shape == (16, 16)
            assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
            seen.add(ref.tobytes())
    assert len(seen) == 9


def test_fmix32_known_values():
    # murmur3's finaliser: 0 is its fixed point, 1 -> 0x514E28B7
    assert int(cr.fmix32(np.uint64(0))) == 0
    assert int(cr.fmix32(np.uint64(1))) == 0x514E28B7


def test_lane_reg_map_is_a_bijection_onto_the_tile():
    cells = {cr.lane_reg_to_row_col(lane, reg) for lane in range(64) for reg in range(4)}
    assert cells == {(row, col) for row in range(16) for col in range(16)}
    # the corners of the layout, by hand: 4*(lane>>4) + reg, lane & 15
    assert cr.lane_reg_to_row_col(0, 0) == (0, 0)
    assert cr.lane_reg_to_row_col(15, 3) == (3, 15)
    assert cr.lane_reg_to_row_col(16, 0) == (4, 0)
    assert cr.lane_reg_to_row_col(47, 2) == (10, 15)
    assert cr.lane_reg_to_row_col(63, 3) == (15, 15)


def test_expected_bits_are_the_reference_tiles_elements():
    for fmt in ("bf16", "fp8", "fp4"):
        ref = cr.reference_tile(fmt, 9, SEEDS[1]).astype(np.float32)
        for lane, reg in ((0, 0), (15, 1), (16, 2), (47, 3), (63, 3)):
            row, col = cr.lane_reg_to_row_col(lane, reg)
            bits = cr.expected_bits(fmt, 9, SEEDS[1], lane, reg)
            assert np.uint32(bits).view(np.float32) == ref[row, col]
            assert 0 <= bits <= cr.M32


def test_lds_word_known_values():
    # word 0, seed 0, round 0: fmix32(0) = 0
    assert cr.lds_word(0, 0, 0) == 0
    # word 1, seed 0, round 0: fmix32(0x9E3779B9)
    assert cr.lds_word(1, 0, 0) == 0x92CA2F0E
    # the last word of 160 KiB, round 2, seed_lo 0xC0FFEE11:
    # 40959 * 0x9E3779B9 + 0xC0FFEE11 + 2 = 0xCEDC145A (mod 2^32)
    assert (40959 * 0x9E3779B9 + 0xC0FFEE11 + 2) & cr.M32 == 0xCEDC145A
    assert cr.lds_word(40959, SEEDS[1], 2) == 0x37C93D0B
    # seed_hi plays no part; the round does
    assert cr.lds_word(40959, SEEDS[1] & cr.M32, 2) == 0x37C93D0B
    assert cr.lds_word(40959, SEEDS[1], 1) != 0x37C93D0B


def test_lds_inverted_pattern_is_the_complement():
    for word in (0, 1, 5, 40959):
        for rnd in (0, 2):
            plain = cr.lds_word(word, SEEDS[1], rnd)
            inv = cr.lds_word(word, SEEDS[1], rnd, inverted=True)
            assert plain ^ inv == cr.M32 and 0 <= inv <= cr.M32


def test_lds_verifiers_are_other_waves_and_lanes_than_the_writer():
    vecs = 163840 // 16
    for v in range(vecs):
        w = cr.lds_writer(4 * v)
        p0 = cr.lds_verifier(4 * v, 0)
        p1 = cr.lds_verifier(4 * v, 1)
        assert w["thread"] == v % 256
        for a, b in ((w, p0), (w, p1), (p0, p1)):
            assert a["wave"] != b["wave"] and a["lane"] != b["lane"], v
        # the four words of a vector share their threads
        for j in range(1, 4):
            assert cr.lds_verifier(4 * v + j, 0) == p0 and cr.lds_verifier(4 * v + j, 1) == p1
    # each thread verifies each residue class exactly once per phase
    for phase in (0, 1):
        assert sorted(cr.lds_verifier(4 * v, phase)["thread"] for v in range(256)) == list(range(256))
    # by hand: vector 0 is read by threads 191 (wave 2, lane 63) and 126 (wave 1, lane 62)
    assert cr.lds_verifier(0, 0) == {"thread": 191, "wave": 2, "lane": 63}
    assert cr.lds_verifier(3, 1) == {"thread": 126, "wave": 1, "lane": 62}
    assert cr.lds_verifier(4 * 65, 0) == {"thread": 0, "wave": 0, "lane": 0}


# ---------------------------------------------------------------------------
# cu_check_fold on synthetic records
# ---------------------------------------------------------------------------

def hw_word(se, sh, cu, simd, wave=0, pipe=0, upper=0):
    return upper << 16 | se << 13 | sh << 12 | cu << 8 | pipe << 6 | simd << 4 | wave


def record(xcc, se, sh, cu, counts=None, first=None, workgroup=0):
    c = {"bf16": 0, "fp8": 0, "fp4": 0, "lds": 0}
    c.update(counts or {})
    return {
        "launch": 0,
        "workgroup": workgroup,
        "xcc": xcc,
        "xcc_raw": xcc,
        # bits above 15 (queue, vm, state ids) differ freely between waves
        "hw_id": [hw_word(se, sh, cu, simd, wave=simd, upper=0x1230 + simd) for simd in range(4)],
        "counts": c,
        "first": first,
    }


def test_hw_id_fields_decode():
    from gpu_docker_api_amd.ops.hipcore import hw_id_fields

    w = hw_word(se=5, sh=1, cu=0xB, simd=2, wave=7, pipe=3, upper=0xABCD)
    assert hw_id_fields(w) == {"wave": 7, "simd": 2, "pipe": 3, "cu": 0xB, "sh": 1, "se": 5}
    assert hw_id_fields(0) == {"wave": 0, "simd": 0, "pipe": 0, "cu": 0, "sh": 0, "se": 0}
    assert hw_id_fields(0xFFFF) == {"wave": 15, "simd": 3, "pipe": 3, "cu": 15, "sh": 1, "se": 7}


def test_fold_clean():
    from gpu_docker_api_amd.ops.hipcore import cu_check_fold

    recs = [record(x, se, 0, cu, workgroup=i)
            for i, (x, se, cu) in enumerate((x, se, cu) for x in range(2) for se in range(2) for cu in range(3))]
    out = cu_check_fold(recs, 12)
    assert out["cus_expected"] == 12 and out["cus_seen"] == 12
    assert out["workgroups"] == 12
    assert out["xccs"] == [{"xcc": 0, "cus": 6}, {"xcc": 1, "cus": 6}]
    assert out["simds_seen"] == [0, 1, 2, 3]
    assert out["errors"] == {"total": 0, "bf16": 0, "fp8": 0, "fp4": 0, "lds": 0}
    assert out["bad_cus"] == []
    assert out["split_workgroups"] == 0


def test_fold_merges_workgroups_of_one_cu():
    from gpu_docker_api_amd.ops.hipcore import cu_check_fold

    recs = [record(3, 1, 0, 4, workgroup=0), record(3, 1, 0, 4, workgroup=9),
            record(4, 1, 0, 4, workgroup=1)]  # same HW_ID on another XCC: another CU
    out = cu_check_fold(recs, 2)
    assert out["workgroups"] == 3 and out["cus_seen"] == 2
    assert out["xccs"] == [{"xcc": 3, "cus": 1}, {"xcc": 4, "cus": 1}]


def test_fold_one_bad_workgroup():
    from gpu_docker_api_amd.ops.hipcore import cu_check_fold, cu_check_key

    first = {"test": "fp8", "tile": 6, "wave": 2, "lane": 17, "reg": 0,
             "expected": 0x42280000, "actual": 0x42280001}
    bad = record(5, 2, 1, 0xB, counts={"fp8": 3}, first=first, workgroup=1)
    recs = [record(5, 2, 1, 0xA), bad, record(5, 2, 1, 0xB, workgroup=2)]
    out = cu_check_fold(recs, 2)
    assert out["errors"] == {"total": 3, "bf16": 0, "fp8": 3, "fp4": 0, "lds": 0}
    assert out["bad_cus"] == [{
        "xcc": 5, "se": 2, "sh": 1, "cu": 0xB, "key": cu_check_key(bad),
        "tests": {"bf16": 0, "fp8": 3, "fp4": 0, "lds": 0},
        "first": dict(first, simd=2),  # record() puts wave w on SIMD w
    }]
    # the SIMD comes from the reporting wave's own HW_ID word
    bad["hw_id"][2] = hw_word(2, 1, 0xB, simd=1, wave=5)
    assert cu_check_fold([bad], 1)["bad_cus"][0]["first"]["simd"] == 1
    assert cu_check_key(bad) == 5 << 8 | 2 << 5 | 1 << 4 | 0xB


def test_fold_reports_incomplete_coverage():
    from gpu_docker_api_amd.ops.hipcore import cu_check_fold

    out = cu_check_fold([record(0, 0, 0, c) for c in range(3)], 256)
    assert out["cus_seen"] == 3 and out["cus_expected"] == 256
    assert out["errors"]["total"] == 0


def test_fold_counts_workgroups_whose_waves_disagree():
    from gpu_docker_api_amd.ops.hipcore import cu_check_fold

    rec = record(0, 0, 0, 1)
    rec["hw_id"][3] = hw_word(0, 0, 2, 3)
    assert cu_check_fold([rec], 1)["split_workgroups"] == 1


# ---------------------------------------------------------------------------
# validate_gpus with a stub extension
# ---------------------------------------------------------------------------

class CuStubExt(StubExt):
    """StubExt plus a cu_check that reports `cus` clean CUs, with `errors`
    bf16 mismatches on the first of them."""

    def __init__(self, cus=8, seen=None, errors=0):
        super().__init__()
        self.cus = cus
        self.seen = cus if seen is None else seen
        self.cu_errors = errors
        self.cu_calls = []

    def device_info(self, i):
        return dict(super().device_info(i), multiProcessorCount=self.cus)

    def cu_check(self, device, rounds, seed, grid_mult, inject):
        self.cu_calls.append((device, rounds, seed, grid_mult, list(inject)))
        recs = [record(c // 4, 0, 0, c % 4, workgroup=c) for c in range(self.seen)]
        if self.cu_errors:
            recs[0]["counts"]["bf16"] = self.cu_errors
            recs[0]["first"] = {"test": "bf16", "tile": 0, "wave": 0, "lane": 0, "reg": 0,
                                "expected": 1, "actual": 0}
        return {"records": recs, "launches": 1, "grid": 2 * self.cus, "rounds": rounds,
                "lds_bytes": 163840, "seconds": 0.01}


@pytest.fixture
def cu_stub(monkeypatch):
    from gpu_docker_api_amd.ops import hipcore

    def install(**kw):
        ext = CuStubExt(**kw)
        monkeypatch.setattr(hipcore, "_ext", ext)
        return ext

    return install


def test_validate_cu_rounds_zero_never_touches_cu_check(cu_stub):
    from gpu_docker_api_amd.ops import hipcore

    ext = cu_stub()
    report = hipcore.validate_gpus(size=2048, iters=3)
    assert report == hipcore.validate_gpus(size=2048, iters=3, cu_rounds=0)
    assert ext.cu_calls == []
    assert "cu_check" not in report["gpus"][0]
    assert list(report["gpus"][0]) == [
        "index", "hbm_gbps", "bf16_tflops", "fp8_tflops", "fp4_tflops", "healthy"]


def test_validate_cu_check_clean_keeps_healthy(cu_stub):
    from gpu_docker_api_amd.ops import hipcore

    ext = cu_stub()
    g = hipcore.validate_gpus(size=2048, iters=3, cu_rounds=5)["gpus"][0]
    assert g["healthy"] is True
    cc = g["cu_check"]
    assert cc["errors"]["total"] == 0 and cc["bad_cus"] == []
    assert cc["cus_seen"] == cc["cus_expected"] == 8
    assert cc["rounds"] == 5 and cc["launches"] == 1 and cc["lds_bytes"] == 163840
    assert len(ext.cu_calls) == 1
    device, rounds, seed, grid_mult, inject = ext.cu_calls[0]
    assert device == 0 and rounds == 5 and grid_mult == 2 and inject == []
    assert 0 <= seed < 2**64


def test_validate_cu_check_errors_mark_unhealthy(cu_stub):
    from gpu_docker_api_amd.ops import hipcore

    cu_stub(errors=2)
    g = hipcore.validate_gpus(size=2048, iters=3, cu_rounds=5)["gpus"][0]
    assert g["cu_check"]["errors"]["total"] == 2
    assert [b["tests"]["bf16"] for b in g["cu_check"]["bad_cus"]] == [2]
    assert g["healthy"] is False


def test_validate_cu_check_incomplete_coverage_leaves_healthy(cu_stub):
    from gpu_docker_api_amd.ops import hipcore

    cu_stub(cus=8, seen=5)
    g = hipcore.validate_gpus(size=2048, iters=3, cu_rounds=5)["gpus"][0]
    assert g["cu_check"]["cus_seen"] == 5 and g["cu_check"]["cus_expected"] == 8
    assert g["healthy"] is True


def test_validate_async_forwards_cu_rounds(cu_stub, run):
    from gpu_docker_api_amd.ops import hipcore

    ext = cu_stub()
    report = run(hipcore.validate_gpus_async(None, 2048, 3, cu_rounds=7))
    assert report["gpus"][0]["cu_check"]["rounds"] == 7
    assert [c[1] for c in ext.cu_calls] == [7]


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


def test_route_cu_check_non_int_is_invalid_params(client, validate_kwargs):
    from gpu_docker_api_amd.routers.codes import Code

    for value in ("x", "8", 1.5, None, [1], True, False):
        r = client.post(URL, json={"cuCheck": value})
        assert r.json()["code"] == int(Code.INVALID_PARAMS), value
    assert validate_kwargs == []


def test_route_cu_check_clamped_and_absent_when_off(client, validate_kwargs):
    for body in ({}, {"cuCheck": 0}, {"cuCheck": 5}, {"cuCheck": 10**9}, {"cuCheck": -3}):
        assert client.post(URL, json=body).json()["code"] == 200, body
    assert [kw.get("cu_rounds", "off") for kw in validate_kwargs] == ["off", "off", 5, 4096, 1]
    assert all("cu_rounds" in kw or set(kw) == {"memtest_mib"} for kw in validate_kwargs)


# ---------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------

def test_cli_cu_check_flag_only_when_given(recording_daemon):
    port, bodies = recording_daemon
    for args in ((), ("--cu-check", "16", "--size", "2048"), ("--cu-check", "0"),
                 ("--cu-check", "8", "--memtest-mib", "2048")):
        out = _cli(port, "resources", "validate", *args)
        assert out.returncode == 0, out.stderr
    assert bodies == [
        (URL, {"size": 4096, "iters": 5}),
        (URL, {"size": 2048, "iters": 5, "cuCheck": 16}),
        (URL, {"size": 4096, "iters": 5}),
        (URL, {"size": 4096, "iters": 5, "memtestMiB": 2048, "cuCheck": 8}),
    ]
