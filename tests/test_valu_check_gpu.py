"""Per-SIMD vector ALU check on a real MI355X (csrc/valu_check.hip).

valu_check_values is compared bit for bit with the exact-arithmetic reference
of tests/valu_check_refs.py, and valu_check_table (the host's table) with the
digests the same reference computes: device and host are held to one
reference. The passes themselves must come back clean, cover every SIMD of
every CU, and report an injected bit flip on exactly the SIMD that carried
it. Inject flips a value in a register, nothing else.
"""
import numpy as np
import pytest

import valu_check_refs as vr
from conftest import require_gpu

pytestmark = pytest.mark.gpu

SEED = 0x7A1C0DE5EED5A1D5
HIGH_SEED = 0xFFFFFFFF00000001
SEEDS = {"seed0": 0, "seed": SEED, "high": HIGH_SEED}
ROUNDS = (0, 1, 4095)
TESTS = vr.TESTS
TRANS = 4
LOW_BIT, SIGN_BIT = 0x1, 0x80000000
TRANS_ULP_BOUND = 4.0


@pytest.fixture(scope="module")
def ext():
    require_gpu()
    from gpu_docker_api_amd.ops import hipcore

    assert hipcore.VALU_CHECK_SEED == SEED
    return hipcore.load_ext()


@pytest.fixture(scope="module")
def info(ext):
    return ext.device_info(0)


def counts_of(**kw):
    return {t: int(kw.get(t, 0)) for t in TESTS}


def first_launch(raw):
    return {r["workgroup"]: r for r in raw["records"] if r["launch"] == 0}


def device_values(ext, test, rnd, seed):
    import torch

    got = ext.valu_check_values(test, rnd, seed)
    assert got.shape == (vr.STEPS, 64) and got.dtype == torch.int64
    return got.cpu().numpy().view(np.uint64)


def test_geometry_matches_the_reference(ext):
    g = ext.valu_check_geometry()
    assert g["steps"] == vr.STEPS and g["threads"] == 256 and g["waves"] == 4
    assert list(g["tests"]) == list(TESTS) and dict(g["test_index"]) == vr.TEST_INDEX
    assert dict(g["ops"]) == vr.OPS
    assert {k: tuple(v) for k, v in g["exponent_windows"].items()} == vr.WINDOWS
    assert g["wave_record_words"] == 16 and g["record_words"] == 64
    lay = dict(g["wave_record_layout"])
    assert lay["valid"] == 0 and lay["xcc"] == 1 and lay["hw_id"] == 2 and lay["counts"] == 3
    assert lay["first_test"] == 8 and sorted(lay.values()) == [0, 1, 2, 3, 8, 9, 10, 11, 12]
    assert (g["max_rounds"], g["max_inject"], g["max_grid_mult"], g["max_launches"]) == (4096, 64, 8, 8)
    assert g["inject_words"] == 6


@pytest.mark.parametrize("seed_id", list(SEEDS))
@pytest.mark.parametrize("test", vr.EXACT_TESTS)
def test_values_are_bit_exact(ext, test, seed_id):
    seed = SEEDS[seed_id]
    for rnd in ROUNDS:
        got = device_values(ext, test, rnd, seed)
        want = vr.values(test, rnd, seed)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (
            f"{test} round {rnd} seed {seed:#x}: {len(bad)} differ, first at step {bad[0][0]} "
            f"(op {bad[0][0] % vr.OPS[test]}) lane {bad[0][1]}: "
            f"{int(got[tuple(bad[0])]):#x} != {int(want[tuple(bad[0])]):#x}")


def test_packed_fp16_keeps_subnormal_results(ext):
    """Rounds in which a packed fma's cancellation lands below 2^-14: the
    reference rounds to a subnormal there, a flushing unit would give zero."""
    for rnd in vr.PK16_SUBNORMAL_ROUNDS:
        got = device_values(ext, "pk16", rnd, 0)
        want = vr.values("pk16", rnd, 0)
        bad = np.argwhere(got != want)
        print(f"pk16 round {rnd}: {len(bad)} of {got.size} results differ from the reference")
        assert bad.size == 0, [(int(s), int(l), hex(int(got[s, l])), hex(int(want[s, l])))
                               for s, l in bad[:4]]


@pytest.mark.parametrize("seed_id", ["seed", "high"])
def test_host_table_equals_the_reference_digests(ext, seed_id):
    import torch

    seed = SEEDS[seed_id]
    table = ext.valu_check_table(3, seed)
    assert table.shape == (4, 3, 64) and table.dtype == torch.int64 and table.device.type == "cpu"
    for t, test in enumerate(vr.EXACT_TESTS):
        for rnd in range(3):
            assert np.array_equal(table[t, rnd].numpy().view(np.uint64),
                                  vr.digests(test, rnd, seed)), (test, rnd)


def test_trans_values_are_the_right_functions(ext):
    """A wiring check (right function, right operand) against float64, within
    4 ULP of the fp32 result; not an accuracy claim."""
    worst = {f: 0.0 for f in vr.TRANS_FUNCS}
    for seed in SEEDS.values():
        for rnd in ROUNDS:
            got = device_values(ext, "trans", rnd, seed)
            assert int(got.max()) <= vr.M32
            dist = vr.ulp_distance(got, vr.trans_reference(rnd, seed))
            for k, f in enumerate(vr.TRANS_FUNCS):
                worst[f] = max(worst[f], float(dist[k::5].max()))
    print("trans max ULP distance from float64: " + ", ".join(f"{f} {worst[f]:.3f}" for f in worst))
    for f in vr.TRANS_FUNCS:
        assert worst[f] <= TRANS_ULP_BOUND, (f, worst[f])


@pytest.mark.parametrize("grid_mult", [0, 1], ids=["one-workgroup", "one-per-cu"])
def test_smallest_launch_is_clean(ext, info, grid_mult):
    raw = ext.valu_check(0, 1, SEED, grid_mult)
    want = 1 if grid_mult == 0 else info["multiProcessorCount"]
    assert raw["grid"] == want and len(raw["records"]) == want * raw["launches"]
    assert raw["rounds"] == 1
    for r in raw["records"]:
        assert dict(r["counts"]) == counts_of() and r["first"] is None
        assert all(dict(w["counts"]) == counts_of() and w["first"] is None for w in r["waves"])
    ref = raw["trans_reference"]
    assert ref["agree"] is True and list(ref["odd_waves"]) == [] and ref["used"] == "all"
    assert len(ref["hw_id"]) == 4


def test_default_pass_covers_every_simd(ext, info):
    from gpu_docker_api_amd.ops import hipcore

    rep = hipcore.valu_check_gpu(0, hipcore.VALU_CHECK_ROUNDS)
    print(f"valu_check default pass: {rep['seconds']} s on the device, {rep['table_seconds']} s "
          f"for the host table, {rep['launches']} launch(es), {rep['workgroups']} workgroups")
    assert rep["errors"]["total"] == 0 and rep["bad_simds"] == []
    assert rep["cus_seen"] == info["multiProcessorCount"]
    assert rep["simds_seen"] == 4 * rep["cus_seen"]
    assert rep["split_workgroups"] == 0
    assert rep["trans_reference"]["agree"] is True and rep["trans_reference_suspect"] is False


def reference_digest(ext, test, rnd, lane):
    """What the table holds: the refs' digest, or for trans the digest of the
    values the device itself computes (the reference copy)."""
    if test == "trans":
        return int(vr.digests_of("trans", device_values(ext, "trans", rnd, SEED))[lane])
    return int(vr.digests(test, rnd, SEED)[lane])


@pytest.mark.parametrize("wave", [0, 1, 2, 3])
@pytest.mark.parametrize("test", TESTS)
def test_every_lane_reports(ext, test, wave):
    t = vr.TEST_INDEX[test]
    rnd = (t + wave) % 2
    mask = LOW_BIT if (t + wave) % 2 == 0 else SIGN_BIT
    inject = [(0, t, rnd, wave, lane, mask) for lane in range(64)]
    raw = ext.valu_check(0, 2, SEED, 0, inject)
    assert raw["grid"] == 1 and raw["launches"] == 1
    rec = raw["records"][0]
    print(f"{test} wave {wave} mask {mask:#x}: counts {dict(rec['counts'])} first {rec['first']}")
    assert dict(rec["counts"]) == counts_of(**{test: 64})
    for w in range(4):
        assert dict(rec["waves"][w]["counts"]) == counts_of(**{test: 64 if w == wave else 0})
    first = rec["first"]
    assert (first["test"], first["round"], first["wave"], first["lane"]) == (test, rnd, wave, 0)
    want = reference_digest(ext, test, rnd, 0)
    assert first["expected"] == want and first["actual"] == want ^ mask


def test_inject_is_localised(ext, info):
    from gpu_docker_api_amd.ops import hipcore

    cus = info["multiProcessorCount"]
    # (workgroup, test, round, wave, lane, xor_mask): one per test
    inject = [
        (0, 0, 0, 0, 0, LOW_BIT),
        (cus // 4, 1, 1, 1, 17, SIGN_BIT),
        (cus // 2, 2, 0, 2, 63, LOW_BIT),
        (3 * cus // 4, 3, 1, 3, 17, SIGN_BIT),
        (cus - 1, 4, 1, 0, 63, LOW_BIT),
    ]
    raw = ext.valu_check(0, 2, SEED, 1, inject)
    assert raw["grid"] == cus
    recs = first_launch(raw)
    assert len(recs) == cus
    keys = [hipcore.cu_check_key(recs[e[0]]) for e in inject]
    assert len(set(keys)) == 5, "the five workgroups must sit on five CUs"
    rep = hipcore.valu_check_fold(list(recs.values()), cus)
    assert rep["errors"] == {"total": 5, **counts_of(**{t: 1 for t in TESTS})}
    bad = {(b["key"], b["simd"]): b for b in rep["bad_simds"]}
    assert len(bad) == 5
    for (wg, t, rnd, wave, lane, mask), key in zip(inject, keys):
        simd = hipcore.hw_id_fields(recs[wg]["hw_id"][wave])["simd"]
        b = bad[(key, simd)]
        assert b["tests"] == counts_of(**{TESTS[t]: 1})
        f = b["first"]
        assert (f["test"], f["round"], f["wave"], f["lane"]) == (TESTS[t], rnd, wave, lane)
        assert f["expected"] ^ f["actual"] == mask
        if TESTS[t] != "trans":
            assert f["expected"] == int(vr.digests(TESTS[t], rnd, SEED)[lane])
    hit = {e[0] for e in inject}
    assert all(dict(r["counts"]) == counts_of() and r["first"] is None
               for wg, r in recs.items() if wg not in hit)


def one_workgroup(ext, inject):
    raw = ext.valu_check(0, 3, SEED, 0, inject)
    assert raw["grid"] == 1 and raw["launches"] == 1
    rec = raw["records"][0]
    print(f"inject {inject}: counts {dict(rec['counts'])} first {rec['first']}")
    return rec


def test_fold_earlier_round_wins_over_lower_lane(ext):
    rec = one_workgroup(ext, [(0, 1, 2, 1, 0, LOW_BIT), (0, 1, 0, 1, 63, SIGN_BIT)])
    assert dict(rec["counts"]) == counts_of(f32=2)
    first = rec["first"]
    assert (first["test"], first["round"], first["wave"], first["lane"]) == ("f32", 0, 1, 63)
    want = int(vr.digests("f32", 0, SEED)[63])
    assert (first["expected"], first["actual"]) == (want, want ^ SIGN_BIT)
    # and across waves: the workgroup's first is the earliest round's
    rec = one_workgroup(ext, [(0, 0, 2, 0, 0, LOW_BIT), (0, 0, 1, 3, 40, LOW_BIT)])
    assert (rec["first"]["round"], rec["first"]["wave"], rec["first"]["lane"]) == (1, 3, 40)
    assert rec["waves"][0]["first"]["round"] == 2


def test_fold_orders_the_tests_inside_a_round(ext):
    # wave 2, round 1: the later the test, the lower the lane
    rec = one_workgroup(ext, [(0, 4, 1, 2, 0, 0x4), (0, 3, 1, 2, 5, 0x2), (0, 2, 1, 2, 31, 0x8),
                              (0, 0, 1, 2, 63, 0x100)])
    assert dict(rec["counts"]) == counts_of(int=1, f64=1, pk16=1, trans=1)
    first = rec["first"]
    assert (first["test"], first["round"], first["wave"], first["lane"]) == ("int", 1, 2, 63)
    want = int(vr.digests("int", 1, SEED)[63])
    assert (first["expected"], first["actual"]) == (want, want ^ 0x100)
    rec = one_workgroup(ext, [(0, 4, 1, 2, 0, 0x4), (0, 3, 1, 2, 5, 0x2), (0, 2, 1, 2, 31, 0x8)])
    assert (rec["first"]["test"], rec["first"]["lane"]) == ("f64", 31)
    rec = one_workgroup(ext, [(0, 4, 1, 2, 0, 0x4), (0, 3, 1, 2, 5, 0x2)])
    assert (rec["first"]["test"], rec["first"]["lane"]) == ("pk16", 5)


class _RecordingExt:
    """The extension, keeping what valu_check returned."""

    def __init__(self, ext):
        self._ext = ext
        self.raw = []

    def __getattr__(self, name):
        return getattr(self._ext, name)

    def valu_check(self, *args):
        raw = self._ext.valu_check(*args)
        self.raw.append((args, raw))
        return raw


def test_production_shape_folds_real_records(ext, info, monkeypatch):
    from gpu_docker_api_amd.ops import hipcore

    cus = info["multiProcessorCount"]
    inject = [(0, 1, 1, 2, 33, 0x00400000), (cus, 3, 0, 1, 7, 0x1000)]
    spy = _RecordingExt(ext)
    monkeypatch.setattr(hipcore, "_ext", spy)
    rep = hipcore.valu_check_gpu(0, 2, inject=inject)
    monkeypatch.undo()
    (args, raw), = spy.raw
    assert args[3] == 2 and raw["grid"] == 2 * cus and [tuple(e) for e in args[4]] == inject
    launches = raw["launches"]
    assert rep["launches"] == launches and rep["workgroups"] == launches * 2 * cus

    recs = first_launch(raw)
    assert dict(recs[0]["counts"]) == counts_of(f32=1)
    assert dict(recs[cus]["counts"]) == counts_of(pk16=1)
    f0, f1 = recs[0]["first"], recs[cus]["first"]
    assert (f0["round"], f0["wave"], f0["lane"]) == (1, 2, 33)
    assert f0["expected"] == int(vr.digests("f32", 1, SEED)[33])
    assert (f1["round"], f1["wave"], f1["lane"]) == (0, 1, 7)
    assert f1["expected"] == int(vr.digests("pk16", 0, SEED)[7])
    assert all(sum(r["counts"].values()) == 0 for wg, r in recs.items() if wg not in (0, cus))

    # the fold against sums taken here, over every launch the pass needed
    per_simd = {}
    for r in raw["records"]:
        for hw, w in zip(r["hw_id"], r["waves"]):
            acc = per_simd.setdefault((hipcore.cu_check_key(r), hipcore.hw_id_fields(hw)["simd"]),
                                      counts_of())
            for t in TESTS:
                acc[t] += w["counts"][t]
    bad = {k: c for k, c in per_simd.items() if sum(c.values())}
    print(f"{launches} launch(es), {rep['cus_seen']} CUs and {rep['simds_seen']} SIMDs seen, "
          f"bad SIMDs {sorted(bad)}")
    assert [(b["key"], b["simd"]) for b in rep["bad_simds"]] == sorted(bad)
    assert {(b["key"], b["simd"]): b["tests"] for b in rep["bad_simds"]} == bad
    totals = {t: sum(c[t] for c in per_simd.values()) for t in TESTS}
    assert totals == counts_of(f32=launches, pk16=launches)
    assert rep["errors"] == {"total": 2 * launches, **totals}
    assert rep["simds_seen"] == len(per_simd)
    assert rep["cus_seen"] == len({k for k, _ in per_simd})


def test_bad_arguments_are_rejected(ext, info):
    cus = info["multiProcessorCount"]
    for entry in [
        (cus, 0, 0, 0, 0, 1),        # workgroup outside a 1 x CUs grid
        (0, 5, 0, 0, 0, 1),          # no such test
        (0, 0, 1, 0, 0, 1),          # round outside 1 round
        (0, 0, 0, 4, 0, 1),          # no wave 4
        (0, 0, 0, 0, 64, 1),         # lane outside the wave
        (0, 0, 0, 0, 0, 1 << 32),    # mask wider than 32 bits
        (0, 0, 0, 0, 0, -1),
        (0, 0, 0, 0, 0),             # short entry
        (0, 0, 0, 0, 0, 1, 0),       # long entry
    ]:
        with pytest.raises(RuntimeError, match="inject"):
            ext.valu_check(0, 1, SEED, 1, [entry])
    with pytest.raises(RuntimeError, match="inject"):
        ext.valu_check(0, 1, SEED, 0, [(0, 0, 0, 0, 0, 1)] * 65)
    with pytest.raises(RuntimeError, match="rounds"):
        ext.valu_check(0, 0, SEED, 1)
    with pytest.raises(RuntimeError, match="rounds"):
        ext.valu_check(0, 4097, SEED, 0)
    with pytest.raises(RuntimeError, match="rounds"):
        ext.valu_check_table(0, SEED)
    with pytest.raises(RuntimeError, match="unknown test"):
        ext.valu_check_values("fp16", 0, SEED)
    with pytest.raises(RuntimeError):
        ext.valu_check_values("int", 4096, SEED)


def test_validate_gpus_carries_a_clean_valu_check(ext):
    from gpu_docker_api_amd.ops import hipcore

    plain = hipcore.validate_gpus(indices=[0], size=2048, iters=3)["gpus"][0]
    g = hipcore.validate_gpus(indices=[0], size=2048, iters=3, valu_rounds=2)["gpus"][0]
    assert "valu_check" not in plain
    assert g["valu_check"]["errors"]["total"] == 0 and g["valu_check"]["bad_simds"] == []
    assert g["valu_check"]["rounds"] == 2
    assert g["healthy"] == plain["healthy"]
