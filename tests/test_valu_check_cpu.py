"""Per-SIMD vector ALU check, everything that needs no GPU: the reference's own
rounding, the host twin (csrc/burnin_selftest.cpp, compiled with g++) bit for
bit against the reference, the fold by SIMD, the validate_gpus wiring, the
route field and the CLI flag."""
import os
import subprocess

import numpy as np
import pytest

import valu_check_refs as vr
from test_cu_check_cpu import hw_word, validate_kwargs  # noqa: F401
from test_memtest_cpu import StubExt, _cli, client, recording_daemon  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "csrc", "burnin_selftest.cpp")
URL = "/api/v1/resources/gpus/validate"
HIGH_SEED = 0xFFFFFFFF00000001
ROUNDS = (0, 1, 4095)
TESTS = vr.TESTS


def _seeds():
    from gpu_docker_api_amd.ops.hipcore import VALU_CHECK_SEED

    return {"seed0": 0, "seed": VALU_CHECK_SEED, "high": HIGH_SEED}


# ---------------------------------------------------------------------------
# the reference's own rounding
# ---------------------------------------------------------------------------

NP_FORMATS = {"f16": (np.float16, np.uint16), "f32": (np.float32, np.uint32),
              "f64": (np.float64, np.uint64)}


@pytest.mark.parametrize("fmt", ["f16", "f32", "f64"])
def test_round_to_format_equals_numpy_on_add_and_mul(fmt):
    ftype, utype = NP_FORMATS[fmt]
    ebits, mbits = vr.FORMATS[fmt]
    rng = np.random.default_rng(7)
    # random signs and mantissas, exponents around the middle of the range so
    # that nothing overflows; fp16 products do reach the subnormal range
    span = {"f16": 12, "f32": 40, "f64": 40}[fmt]
    bias = (1 << (ebits - 1)) - 1
    field = rng.integers(bias - span, bias + span // 4, size=(2, 4000)).astype(np.uint64)
    mant = rng.integers(0, 1 << mbits, size=(2, 4000)).astype(np.uint64)
    sign = rng.integers(0, 2, size=(2, 4000)).astype(np.uint64)
    bits = (sign << np.uint64(ebits + mbits) | field << np.uint64(mbits) | mant).astype(utype)
    x, y = bits.view(ftype)
    with np.errstate(all="ignore"):
        want_add = (x + y).view(utype).tolist()
        want_mul = (x * y).view(utype).tolist()
    subnormal = 0
    for i, (a, b) in enumerate(zip(bits[0].tolist(), bits[1].tolist())):
        da, db = vr.decode(a, fmt), vr.decode(b, fmt)
        assert vr.add_exact(da, db, fmt) == want_add[i], (hex(a), hex(b))
        assert vr.mul_exact(da, db, fmt) == want_mul[i], (hex(a), hex(b))
        subnormal += 0 < (want_mul[i] & ((1 << (ebits + mbits)) - 1)) < (1 << mbits)
    if fmt == "f16":
        assert subnormal > 50, subnormal  # the subnormal path was really taken


def test_round_to_format_ties_and_subnormals_by_hand():
    r = vr.round_to_format
    # ties to even at 1.0 in fp16 (last place 2^-10)
    assert r(2048 + 1, -11, "f16") == 0x3C00
    assert r(2048 + 3, -11, "f16") == 0x3C02
    assert r((2049 << 20) + 1, -31, "f16") == 0x3C01
    assert r(-(2048 + 3), -11, "f16") == 0xBC02
    # the subnormal boundary
    assert r(1, -14, "f16") == 0x0400
    assert r(1023, -24, "f16") == 0x03FF
    assert r(2047, -25, "f16") == 0x0400  # 1023.5: tie, up to the smallest normal
    assert r(2045, -25, "f16") == 0x03FE  # 1022.5: tie to even
    assert r(1, -24, "f16") == 0x0001
    assert r(1, -25, "f16") == 0x0000     # half the smallest subnormal: tie to zero
    assert r(3, -26, "f16") == 0x0001
    assert r(3, -25, "f16") == 0x0002
    assert r(-1, -28, "f16") == 0x8000
    # the largest finite value and the tie above it
    assert r(65504, 0, "f16") == 0x7BFF
    assert r(65519, 0, "f16") == 0x7BFF
    assert r(65520, 0, "f16") == 0x7C00
    # f32 and f64: 2^24 + 1 ties down, 2^24 + 3 ties up; the smallest subnormals
    assert r((1 << 24) + 1, 0, "f32") == 0x4B800000
    assert r((1 << 24) + 3, 0, "f32") == 0x4B800002
    assert r(1, -149, "f32") == 0x00000001 and r(1, -150, "f32") == 0
    assert r(3, -150, "f32") == 0x00000002
    assert r((1 << 53) + 1, 0, "f64") == 0x4340000000000000
    assert r(1, -1074, "f64") == 1 and r(1, -1075, "f64") == 0
    # a cancelling fp16 fma: (1 + 2^-10)(1/16 + 2^-14) - (1/16 + 2^-13) = 2^-24
    d = lambda h: vr.decode(h, "f16")  # noqa: E731
    assert vr.fma_exact(d(0x3C01), d(0x2C01), d(0xAC02), "f16") == 0x0001
    assert vr.fma_exact(d(0x3E00), d(0x3E00), d(0xC080), "f16") == 0x0000


def test_windows_and_operand_builders():
    assert vr.WINDOWS == {"f32": (120, 134), "f64": (1016, 1030), "f16": (11, 19)}
    for u in (0, 0xFFFFFFFF, 0x12345678, 0x80000000):
        f = vr.f32_operand(u)
        assert 120 <= (f >> 23) & 0xFF <= 134 and (f ^ u) & 0x807FFFFF == 0
        d = vr.f64_operand(u, 0xDEADBEEF)
        assert 1016 <= (d >> 52) & 0x7FF <= 1030 and d & vr.M32 == 0xDEADBEEF
        assert (d >> 63) == u >> 31 and ((d >> 32) ^ u) & 0xFFFFF == 0
        h = vr.f16_operand(u)
        assert h < 0x10000 and 11 <= (h >> 10) & 31 <= 19 and (h ^ u) & 0x83FF == 0


def test_integer_ops_by_hand():
    op = vr.int_result
    a, b, c, d, e = 0xAABBCCDD, 0x11223344, 0x04000703, 0x80000001, 0x00000821
    assert op(0, a, b, c, d, e) == ((a * b) & vr.M32, None)
    assert op(2, 0xFFFFFFFF, 2, 0, 0, 0) == (0xFFFFFFFF, None)  # -1 * 2 = -2: high word -1
    assert op(1, 0xFFFFFFFF, 2, 0, 0, 0) == (1, None)
    assert op(6, 1, 31, 0x80000000, 0, 0) == (0x80000000, 0xFFFFFFFF)
    assert op(8, 0x1, 0x80000000, 31, 0, 0) == (0x3, None)
    assert op(9, 0xDEADBEEF, 8, 12, 0, 0) == (0xDBE, None)
    assert op(10, 0xF0F0, 0xFFFFFFFF, 0, 0, 0) == (7, None)
    assert op(11, 0, 0, 0, 0, 0) == (32, None) and op(11, 1, 0, 0, 0, 0) == (31, None)
    assert op(12, a, b, c, 0, 0) == (0xDD44AA11, None)
    assert op(13, 0x01FF0010, 0xFF0100F0, 5, 0, 0) == (5 + 254 + 254 + 224, None)
    assert op(14, 0xFFFFFFFF, 1, 0x80000000, 5, 0) == (1 + 0x80000000, 0xFFFFFFFF + 5 & vr.M32)
    assert op(15, 0xFF00FF00, 0x12345678, 0x9ABCDEF0, 0, 0) == (0x12BC56F0, None)
    assert op(7, 0, 1, 1, 0, e) == ((1 << 32 >> 33) ^ (1 << 8) & vr.M32, 0)


# ---------------------------------------------------------------------------
# the host twin against the reference
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("burnin_valu") / "burnin_selftest")
    subprocess.run(["g++", "-std=c++17", "-O1", SRC, "-o", exe], check=True)
    return exe


def _run(exe, *args):
    return subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True)


def test_bare_selftest_checks_the_valu_section(selftest):
    r = _run(selftest)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "burnin selftest OK"
    assert "check_valu" in open(SRC).read()


@pytest.mark.parametrize("seed_id", ["seed0", "seed", "high"])
@pytest.mark.parametrize("rnd", ROUNDS)
@pytest.mark.parametrize("test", vr.EXACT_TESTS)
def test_host_twin_is_bit_exact(selftest, test, rnd, seed_id):
    seed = _seeds()[seed_id]
    r = _run(selftest, "valu", test, rnd, seed)
    assert r.returncode == 0, r.stderr
    out = np.array([int(t) for t in r.stdout.split()], dtype=np.uint64)
    assert out.size == vr.STEPS * 64 + 64
    got = out[: vr.STEPS * 64].reshape(vr.STEPS, 64)
    want = vr.values(test, rnd, seed)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (
        f"{test} round {rnd} seed {seed:#x}: {len(bad)} differ, first at step {bad[0][0]} "
        f"(op {bad[0][0] % vr.OPS[test]}) lane {bad[0][1]}: "
        f"{int(got[tuple(bad[0])]):#x} != {int(want[tuple(bad[0])]):#x}")
    assert np.array_equal(out[vr.STEPS * 64:], vr.digests(test, rnd, seed))


def test_selftest_refuses_trans_and_bad_rounds(selftest):
    assert _run(selftest, "valu", "trans", 0, 0).returncode == 2
    assert _run(selftest, "valu", "int", 4096, 0).returncode == 2


def test_results_depend_on_lane_round_and_seed():
    v = vr.values("int", 0, 0)
    assert len({v[0].tobytes(), v[16].tobytes()}) == 2 and len(set(v[0].tolist())) > 60
    assert not np.array_equal(vr.digests("int", 0, 0), vr.digests("int", 1, 0))
    assert not np.array_equal(vr.digests("f32", 0, 0), vr.digests("f32", 0, HIGH_SEED))


def subnormal_halves(vals) -> int:
    """How many packed-fma halves of a pk16 round are non-zero and below 2^-14."""
    v = vals[0::4]  # the fma steps
    hits = 0
    for half in (v & np.uint64(0xFFFF), (v >> np.uint64(16)) & np.uint64(0xFFFF)):
        mag = half & np.uint64(0x7FFF)
        hits += int(((mag > 0) & (mag < 0x0400)).sum())
    return hits


def test_pk16_reaches_the_subnormal_range(selftest):
    """A packed fma's cancellation lands below 2^-14 about once in six rounds.
    The rounds named here do (seed 0), so a bit-exact comparison on them says
    whether subnormal results are kept; the host twin keeps them."""
    assert [subnormal_halves(vr.values("pk16", rnd, 0)) for rnd in vr.PK16_SUBNORMAL_ROUNDS] == [1, 1, 2]
    for rnd in vr.PK16_SUBNORMAL_ROUNDS:
        r = _run(selftest, "valu", "pk16", rnd, 0)
        got = np.array([int(t) for t in r.stdout.split()], dtype=np.uint64)[: vr.STEPS * 64]
        assert np.array_equal(got.reshape(vr.STEPS, 64), vr.values("pk16", rnd, 0))


def test_trans_arguments_stay_in_their_ranges():
    x = vr.trans_args(0, HIGH_SEED)
    op = np.arange(vr.STEPS) % 5
    assert x[op == 0].min() >= -16 and x[op == 0].max() < 16
    assert x[op == 1].min() >= 2 and x[op == 1].max() < 2 ** 24
    for k in (2, 3, 4):
        assert x[op == k].min() >= 2.0 ** -20 and x[op == k].max() < 2.0 ** 20
    ref = vr.trans_reference(0, HIGH_SEED)
    assert np.isfinite(ref).all()
    assert np.array_equal(ref[2], 1.0 / x[2].astype(np.float64))


# ---------------------------------------------------------------------------
# valu_check_fold on synthetic records
# ---------------------------------------------------------------------------

def counts_of(**kw):
    return {t: int(kw.get(t, 0)) for t in TESTS}


def record(xcc, se, sh, cu, wave_counts=None, wave_first=None, workgroup=0, simds=(0, 1, 2, 3)):
    """A workgroup's record; wave w ran on SIMD simds[w]. wave_counts and
    wave_first map a wave to its counts and first mismatch."""
    waves = []
    total = counts_of()
    for w in range(4):
        c = counts_of(**(wave_counts or {}).get(w, {}))
        for t in TESTS:
            total[t] += c[t]
        waves.append({"counts": c, "first": (wave_first or {}).get(w)})
    firsts = [w["first"] for w in waves if w["first"] is not None]
    return {
        "launch": 0, "workgroup": workgroup, "xcc": xcc, "xcc_raw": xcc,
        "hw_id": [hw_word(se, sh, cu, simds[w], wave=w, upper=0x1230 + w) for w in range(4)],
        "counts": total, "waves": waves, "first": firsts[0] if firsts else None,
    }


def test_fold_clean():
    from gpu_docker_api_amd.ops.hipcore import valu_check_fold

    recs = [record(x, se, 0, cu, workgroup=i)
            for i, (x, se, cu) in enumerate((x, se, cu) for x in range(2) for se in range(2) for cu in range(3))]
    out = valu_check_fold(recs, 12)
    assert out["cus_expected"] == 12 and out["cus_seen"] == 12 and out["simds_seen"] == 48
    assert out["workgroups"] == 12 and out["split_workgroups"] == 0
    assert out["errors"] == {"total": 0, **counts_of()}
    assert out["bad_simds"] == [] and out["trans_reference_suspect"] is False


def test_fold_one_bad_lane():
    from gpu_docker_api_amd.ops.hipcore import cu_check_key, valu_check_fold

    first = {"test": "f64", "round": 3, "wave": 2, "lane": 17,
             "expected": 0x42280000, "actual": 0x42280001}
    bad = record(5, 2, 1, 0xB, {2: {"f64": 1}}, {2: first}, workgroup=1, simds=(3, 2, 1, 0))
    out = valu_check_fold([record(5, 2, 1, 0xA), bad, record(5, 2, 1, 0xB, workgroup=2)], 2)
    assert out["errors"] == {"total": 1, **counts_of(f64=1)}
    assert out["cus_seen"] == 2 and out["simds_seen"] == 8 and out["workgroups"] == 3
    # wave 2 of that workgroup ran on SIMD 1: the SIMD is the wave's own HW_ID field
    assert out["bad_simds"] == [{
        "xcc": 5, "se": 2, "sh": 1, "cu": 0xB, "simd": 1, "key": cu_check_key(bad),
        "tests": counts_of(f64=1), "first": first,
    }]


def test_fold_two_waves_of_one_cu_on_different_simds():
    from gpu_docker_api_amd.ops.hipcore import valu_check_fold

    f0 = {"test": "int", "round": 0, "wave": 0, "lane": 1, "expected": 1, "actual": 3}
    f3 = {"test": "pk16", "round": 1, "wave": 3, "lane": 63, "expected": 2, "actual": 0}
    rec = record(1, 0, 0, 7, {0: {"int": 2}, 3: {"pk16": 5, "int": 1}}, {0: f0, 3: f3})
    again = record(1, 0, 0, 7, {0: {"int": 4}}, {0: dict(f0, lane=9)}, workgroup=1)
    out = valu_check_fold([rec, again], 1)
    assert out["errors"] == {"total": 12, **counts_of(int=7, pk16=5)}
    assert [(b["simd"], b["tests"]) for b in out["bad_simds"]] == [
        (0, counts_of(int=6)), (3, counts_of(int=1, pk16=5))]
    # the first mismatch a SIMD keeps is the first one reported for it
    assert out["bad_simds"][0]["first"] == f0 and out["bad_simds"][1]["first"] == f3
    assert out["cus_seen"] == 1 and out["simds_seen"] == 4


def test_fold_lists_bad_simds_in_key_then_simd_order():
    from gpu_docker_api_amd.ops.hipcore import valu_check_fold

    f = {"test": "int", "round": 0, "wave": 0, "lane": 0, "expected": 0, "actual": 1}
    recs = [record(3, 0, 0, 1, {1: {"int": 1}}, {1: f}), record(0, 1, 0, 2, {3: {"f32": 1}}, {3: f}),
            record(0, 1, 0, 2, {0: {"f32": 1}}, {0: f}, workgroup=5)]
    out = valu_check_fold(recs, 2)
    assert [(b["xcc"], b["simd"]) for b in out["bad_simds"]] == [(0, 0), (0, 3), (3, 1)]


def test_fold_trans_reference_suspect():
    from gpu_docker_api_amd.ops.hipcore import valu_check_fold

    f = {"test": "trans", "round": 0, "wave": 0, "lane": 0, "expected": 0, "actual": 1}
    every = {w: {"trans": 64} for w in range(4)}
    firsts = {w: dict(f, wave=w) for w in range(4)}
    # three of four CUs disagree with the table in trans only, on every SIMD
    recs = [record(0, 0, 0, c, every, firsts, workgroup=c) for c in range(3)] + [record(0, 0, 0, 3)]
    out = valu_check_fold(recs, 4)
    assert out["simds_seen"] == 16 and len(out["bad_simds"]) == 12
    assert out["trans_reference_suspect"] is True
    # exactly half is not more than half
    out = valu_check_fold(recs[1:] + [record(0, 0, 0, 4, workgroup=4)], 4)
    assert len(out["bad_simds"]) == 8 and out["trans_reference_suspect"] is False
    # the same SIMDs with an exact test wrong as well: the card, not the table
    dirty = {w: {"trans": 64, "int": 1} for w in range(4)}
    recs = [record(0, 0, 0, c, dirty, firsts, workgroup=c) for c in range(3)] + [record(0, 0, 0, 3)]
    assert valu_check_fold(recs, 4)["trans_reference_suspect"] is False
    # one bad SIMD in sixteen
    recs = [record(0, 0, 0, 0, {1: {"trans": 3}}, {1: f})] + [record(0, 0, 0, c) for c in (1, 2, 3)]
    assert valu_check_fold(recs, 4)["trans_reference_suspect"] is False


def test_fold_reports_incomplete_coverage_without_judging():
    from gpu_docker_api_amd.ops.hipcore import valu_check_fold

    out = valu_check_fold([record(0, 0, 0, c) for c in range(3)], 256)
    assert out["cus_seen"] == 3 and out["cus_expected"] == 256 and out["simds_seen"] == 12
    assert out["errors"]["total"] == 0 and out["bad_simds"] == []
    rec = record(0, 0, 0, 1)
    rec["hw_id"][3] = hw_word(0, 0, 2, 3)
    assert valu_check_fold([rec], 1)["split_workgroups"] == 1


# ---------------------------------------------------------------------------
# validate_gpus with a stub extension
# ---------------------------------------------------------------------------

class ValuStubExt(StubExt):
    """StubExt plus a valu_check that reports `cus` clean CUs, with `errors`
    f32 mismatches on wave 1 of the first."""

    def __init__(self, cus=8, errors=0):
        super().__init__()
        self.cus = cus
        self.valu_errors = errors
        self.valu_calls = []

    def device_info(self, i):
        return dict(super().device_info(i), multiProcessorCount=self.cus)

    def cu_check(self, *a):  # pragma: no cover - must never be reached here
        raise AssertionError("cu_check called")

    def valu_check(self, device, rounds, seed, grid_mult, inject):
        self.valu_calls.append((device, rounds, seed, grid_mult, list(inject)))
        recs = [record(c // 4, 0, 0, c % 4, workgroup=c) for c in range(self.cus)]
        if self.valu_errors:
            first = {"test": "f32", "round": 0, "wave": 1, "lane": 0, "expected": 1, "actual": 0}
            recs[0] = record(0, 0, 0, 0, {1: {"f32": self.valu_errors}}, {1: first})
        return {"records": recs, "launches": 1, "grid": 2 * self.cus, "rounds": rounds,
                "seconds": 0.01234567, "table_seconds": 0.00234567,
                "trans_reference": {"agree": True, "xcc": 0, "xcc_raw": 0, "hw_id": [0, 16, 32, 48],
                                    "odd_waves": [], "used": "all"}}


@pytest.fixture
def valu_stub(monkeypatch):
    from gpu_docker_api_amd.ops import hipcore

    def install(**kw):
        ext = ValuStubExt(**kw)
        monkeypatch.setattr(hipcore, "_ext", ext)
        return ext

    return install


def test_validate_valu_rounds_zero_never_touches_valu_check(valu_stub):
    from gpu_docker_api_amd.ops import hipcore

    ext = valu_stub()
    report = hipcore.validate_gpus(size=2048, iters=3)
    assert report == hipcore.validate_gpus(size=2048, iters=3, valu_rounds=0)
    assert ext.valu_calls == []
    assert list(report["gpus"][0]) == [
        "index", "hbm_gbps", "bf16_tflops", "fp8_tflops", "fp4_tflops", "healthy"]


def test_validate_valu_check_clean_keeps_healthy(valu_stub):
    from gpu_docker_api_amd.ops import hipcore

    ext = valu_stub()
    g = hipcore.validate_gpus(size=2048, iters=3, valu_rounds=5)["gpus"][0]
    assert g["healthy"] is True
    vc = g["valu_check"]
    assert vc["errors"]["total"] == 0 and vc["bad_simds"] == []
    assert vc["cus_seen"] == vc["cus_expected"] == 8 and vc["simds_seen"] == 32
    assert vc["rounds"] == 5 and vc["launches"] == 1
    assert vc["seconds"] == 0.0123 and vc["table_seconds"] == 0.0023
    assert vc["trans_reference"]["agree"] is True
    (device, rounds, seed, grid_mult, inject), = ext.valu_calls
    assert device == 0 and rounds == 5 and grid_mult == 2 and inject == []
    assert seed == hipcore.VALU_CHECK_SEED and 0 <= seed < 2**64


def test_validate_valu_check_errors_mark_unhealthy(valu_stub):
    from gpu_docker_api_amd.ops import hipcore

    valu_stub(errors=1)
    g = hipcore.validate_gpus(size=2048, iters=3, valu_rounds=5)["gpus"][0]
    assert g["valu_check"]["errors"]["total"] == 1
    assert [(b["simd"], b["tests"]["f32"]) for b in g["valu_check"]["bad_simds"]] == [(1, 1)]
    assert g["healthy"] is False


def test_validate_async_forwards_valu_rounds(valu_stub, run):
    from gpu_docker_api_amd.ops import hipcore

    ext = valu_stub()
    report = run(hipcore.validate_gpus_async(None, 2048, 3, valu_rounds=7))
    assert report["gpus"][0]["valu_check"]["rounds"] == 7
    assert [c[1] for c in ext.valu_calls] == [7]


def test_constants():
    from gpu_docker_api_amd.ops import hipcore

    assert hipcore.VALU_CHECK_ROUNDS == 8
    assert hipcore.VALU_CHECK_TESTS == TESTS


# ---------------------------------------------------------------------------
# route and CLI
# ---------------------------------------------------------------------------

def test_route_valu_check_non_int_is_invalid_params(client, validate_kwargs):
    from gpu_docker_api_amd.routers.codes import Code

    for value in ("x", "8", 1.5, None, [1], True, False):
        r = client.post(URL, json={"valuCheck": value})
        assert r.json()["code"] == int(Code.INVALID_PARAMS), value
    assert validate_kwargs == []


def test_route_valu_check_clamped_and_absent_when_off(client, validate_kwargs):
    for body in ({}, {"valuCheck": 0}, {"valuCheck": 5}, {"valuCheck": 10**9}, {"valuCheck": -3}):
        assert client.post(URL, json=body).json()["code"] == 200, body
    assert [kw.get("valu_rounds", "off") for kw in validate_kwargs] == ["off", "off", 5, 4096, 1]
    assert all("valu_rounds" in kw or set(kw) == {"memtest_mib"} for kw in validate_kwargs)


def test_cli_valu_check_flag_only_when_given(recording_daemon):
    port, bodies = recording_daemon
    for args in ((), ("--valu-check", "16", "--size", "2048"), ("--valu-check", "0"),
                 ("--valu-check", "8", "--cu-check", "2")):
        out = _cli(port, "resources", "validate", *args)
        assert out.returncode == 0, out.stderr
    assert bodies == [
        (URL, {"size": 4096, "iters": 5}),
        (URL, {"size": 2048, "iters": 5, "valuCheck": 16}),
        (URL, {"size": 4096, "iters": 5}),
        (URL, {"size": 4096, "iters": 5, "cuCheck": 2, "valuCheck": 8}),
    ]
