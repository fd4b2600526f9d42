"""Per-CU MFMA and LDS check on a real MI355X (csrc/cu_check.hip).

cu_check_tile is compared bit for bit with the numpy reference of
tests/cu_check_refs.py: that pins the fragment layout, the scale operand and
the generator independently of the on-device check. The passes themselves
must come back clean, cover every CU exactly once per key, and report an
injected bit flip on exactly the CU that carried it.
"""
import pytest

import cu_check_refs as cr
import kernel_refs as kr
from conftest import require_gpu

pytestmark = pytest.mark.gpu

SEED = 0x5EEDC0DEC0FFEE11
TILES = (0, 1, 2, 3, 4, 1023)
TESTS = ("bf16", "fp8", "fp4", "lds")


@pytest.fixture(scope="module")
def ext():
    require_gpu()
    from gpu_docker_api_amd.ops import hipcore

    return hipcore.load_ext()


@pytest.fixture(scope="module")
def info(ext):
    return ext.device_info(0)


def total_errors(raw):
    return sum(sum(r["counts"].values()) for r in raw["records"])


def test_geometry_matches_the_reference(ext):
    g = ext.cu_check_geometry()
    assert dict(g["k"]) == cr.K
    assert dict(g["fmt_index"]) == cr.FMT_INDEX
    assert list(g["tests"]) == list(TESTS)
    assert g["threads"] == 256 and g["waves"] == 4


@pytest.mark.parametrize("seed", [0, SEED], ids=["seed0", "seed"])
@pytest.mark.parametrize("fmt", ["bf16", "fp8", "fp4"])
def test_tile_is_bit_exact(ext, fmt, seed):
    import torch

    for tile in TILES:
        got = ext.cu_check_tile(fmt, tile, seed)
        assert got.shape == (16, 16) and got.dtype == torch.float32
        ref = torch.from_numpy(cr.reference_tile(fmt, tile, seed))
        try:
            kr.assert_exact(got, ref)
        except kr.KernelMismatch as exc:
            raise AssertionError(f"{fmt} tile {tile} seed {seed:#x}: {exc}") from None


def test_tile_rejects_bad_arguments(ext):
    with pytest.raises(RuntimeError):
        ext.cu_check_tile("fp16", 0, SEED)
    with pytest.raises(RuntimeError):
        ext.cu_check_tile("bf16", -1, SEED)


@pytest.mark.parametrize("grid_mult", [0, 1], ids=["one-workgroup", "one-per-cu"])
def test_smallest_launch_is_clean(ext, info, grid_mult):
    raw = ext.cu_check(0, 1, SEED, grid_mult)
    want = 1 if grid_mult == 0 else info["multiProcessorCount"]
    assert raw["grid"] == want and len(raw["records"]) == want * raw["launches"]
    assert total_errors(raw) == 0
    assert all(r["first"] is None for r in raw["records"])


def test_default_pass_covers_every_cu(ext, info):
    from gpu_docker_api_amd.ops import hipcore

    rep = hipcore.cu_check_gpu(0, hipcore.CU_CHECK_ROUNDS)
    print(f"cu_check default pass: {rep['seconds']} s, {rep['launches']} launch(es), "
          f"{rep['workgroups']} workgroups, xccs {rep['xccs']}")
    assert rep["errors"]["total"] == 0 and rep["bad_cus"] == []
    assert rep["cus_seen"] == info["multiProcessorCount"]
    assert len({x["cus"] for x in rep["xccs"]}) == 1, rep["xccs"]
    assert rep["simds_seen"] == [0, 1, 2, 3]
    assert rep["split_workgroups"] == 0
    assert rep["lds_bytes"] == info["sharedMemPerBlockOptin"]


def test_inject_is_localised(ext, info):
    from gpu_docker_api_amd.ops import hipcore

    cus = info["multiProcessorCount"]
    rounds = 2
    words = info["sharedMemPerBlockOptin"] // 4
    # (workgroup, test, tile_or_round, lane_or_word, xor_mask)
    inject = [
        (0, 0, 0, 0, 0x1),
        (cus // 2, 1, 5, 63, 0x80000000),
        (cus - 1, 2, 7, 17, 0x00F0A501),
        (1, 3, 1, words - 1, 0x80000001),
    ]
    raw = ext.cu_check(0, rounds, SEED, 1, inject)
    assert raw["grid"] == cus
    recs =[r for r in raw["records"] if r["launch"] == 0]
    by_wg = {r["workgroup"]: r for r in recs}
    rep = hipcore.cu_check_fold(recs, cus)
    want_keys = sorted(hipcore.cu_check_key(by_wg[e[0]]) for e in inject)
    assert len(set(want_keys)) == 4, "the four workgroups must sit on four CUs"
    assert sorted(b["key"] for b in rep["bad_cus"]) == want_keys
    assert rep["errors"] == {"total": 4, "bf16": 1, "fp8": 1, "fp4": 1, "lds": 1}
    bad = {b["key"]: b for b in rep["bad_cus"]}
    for wg, test, index, lane_or_word, mask in inject:
        b = bad[hipcore.cu_check_key(by_wg[wg])]
        name = TESTS[test]
        assert b["tests"] == {t: int(t == name) for t in TESTS}
        f = b["first"]
        assert f["test"] == name
        assert f["expected"] ^ f["actual"] == mask
        if name == "lds":
            assert f["round"] == index and f["word"] == lane_or_word
        else:
            assert f["tile"] == index and f["lane"] == lane_or_word and f["reg"] == 0
            assert f["wave"] == index % 4
    clean = [r for r in recs if r["workgroup"] not in {e[0] for e in inject}]
    assert all(sum(r["counts"].values()) == 0 and r["first"] is None for r in clean)


def test_inject_out_of_range_is_rejected(ext, info):
    cus = info["multiProcessorCount"]
    words = info["sharedMemPerBlockOptin"] // 4
    for entry in [
        (cus, 0, 0, 0, 1),       # workgroup outside a 1 x CUs grid
        (0, 4, 0, 0, 1),         # no such test
        (0, 0, 4, 0, 1),         # tile outside 1 round x 4 waves
        (0, 1, 0, 64, 1),        # lane outside the wave
        (0, 3, 1, 0, 1),         # round outside 1 round
        (0, 3, 0, words, 1),     # word outside LDS
        (0, 0, 0, 0, 1 << 32),   # mask wider than 32 bits
        (0, 0, 0, 0),            # short entry
    ]:
        with pytest.raises(RuntimeError):
            ext.cu_check(0, 1, SEED, 1, [entry])
    with pytest.raises(RuntimeError):
        ext.cu_check(0, 0, SEED, 1)


def test_validate_gpus_carries_a_clean_cu_check(ext):
    from gpu_docker_api_amd.ops import hipcore

    plain = hipcore.validate_gpus(indices=[0], size=2048, iters=3)["gpus"][0]
    g = hipcore.validate_gpus(indices=[0], size=2048, iters=3, cu_rounds=2)["gpus"][0]
    assert "cu_check" not in plain
    assert g["cu_check"]["errors"]["total"] == 0 and g["cu_check"]["bad_cus"] == []
    assert g["cu_check"]["rounds"] == 2
    assert g["healthy"] == plain["healthy"]


# ---------------------------------------------------------------------------
# The comparators, held to every lane, register and LDS word. Inject entries
# are (workgroup, test, tile_or_round, lane_or_word, xor_mask[, sub]); sub is
# the accumulator register for tests 0..2 and the phase for lds. Every
# assertion below is bit-exact or an integer count.
# ---------------------------------------------------------------------------

LOW_BIT, SIGN_BIT = 0x1, 0x80000000
LDS = 3


def counts_of(**kw):
    return {t: int(kw.get(t, 0)) for t in TESTS}


def first_launch(raw):
    return {r["workgroup"]: r for r in raw["records"] if r["launch"] == 0}


def chunks(entries, n=64):
    return [entries[i:i + n] for i in range(0, len(entries), n)]


def test_inject_geometry(ext):
    g = ext.cu_check_geometry()
    assert g["inject_words"] == 6 and g["lds_phases"] == 2 and g["max_inject"] == 64


@pytest.mark.parametrize("reg", [0, 1, 2, 3])
@pytest.mark.parametrize("fmt", ["bf16", "fp8", "fp4"])
def test_every_lane_and_register_reports(ext, fmt, reg):
    f = cr.FMT_INDEX[fmt]
    tile = reg  # one round: tile == wave, so the four registers also walk the four waves
    mask = LOW_BIT if (f + reg) % 2 == 0 else SIGN_BIT  # six calls each
    inject = [(0, f, tile, lane, mask, reg) for lane in range(64)]
    raw = ext.cu_check(0, 1, SEED, 0, inject)
    assert raw["grid"] == 1 and raw["launches"] == 1
    rec = raw["records"][0]
    print(f"{fmt} reg {reg} mask {mask:#x}: counts {dict(rec['counts'])} first {rec['first']}")
    assert dict(rec["counts"]) == counts_of(**{fmt: 64})
    first = rec["first"]
    assert (first["test"], first["tile"], first["wave"], first["lane"], first["reg"]) == \
        (fmt, tile, tile % 4, 0, reg)
    want = cr.expected_bits(fmt, tile, SEED, 0, reg)
    assert first["expected"] == want and first["actual"] == want ^ mask


ELEMENT_LANES = (0, 15, 16, 47, 63)
ELEMENT_TILES = (0, 1, 2, 3, 8, 9, 10, 11)  # rounds 0 and 2 of three, every wave


@pytest.mark.parametrize("fmt", ["bf16", "fp8", "fp4"])
def test_report_names_the_right_element(ext, info, fmt):
    cus = info["multiProcessorCount"]
    f = cr.FMT_INDEX[fmt]
    sample = [(lane, reg) for lane in ELEMENT_LANES for reg in range(4)]
    assert len(sample) == 20 and cus >= len(sample)
    inject = []
    for i, (lane, reg) in enumerate(sample):
        wg = i * (cus // len(sample))
        tile = ELEMENT_TILES[(3 * i + reg) % len(ELEMENT_TILES)]
        mask = 1 << ((7 * i + f) % 32)
        inject.append((wg, f, tile, lane, mask, reg))
    assert {e[2] // 4 for e in inject} == {0, 2} and {e[5] for e in inject} == {0, 1, 2, 3}
    raw = ext.cu_check(0, 3, SEED, 1, inject)
    recs = first_launch(raw)
    assert len(recs) == cus
    for wg, _, tile, lane, mask, reg in inject:
        rec = recs[wg]
        assert dict(rec["counts"]) == counts_of(**{fmt: 1}), (wg, rec)
        first = rec["first"]
        assert first["test"] == fmt
        assert (first["tile"], first["wave"], first["lane"], first["reg"]) == \
            (tile, tile % 4, lane, reg), (wg, first)
        want = cr.expected_bits(fmt, tile, SEED, lane, reg)
        assert first["expected"] == want, (tile, lane, reg, hex(first["expected"]), hex(want))
        assert first["actual"] == want ^ mask
    hit = {e[0] for e in inject}
    assert all(sum(r["counts"].values()) == 0 and r["first"] is None
               for wg, r in recs.items() if wg not in hit)


def lds_coverage_words(words):
    """(word, mask) pairs that reach every class of LDS word the verify loops
    distinguish; no word twice."""
    vecs = words // 4
    blocks = vecs // 256  # vectors per verifying thread
    assert words % 1024 == 0 and blocks >= 8
    out = [(w, 0xA5A5A5A5) for w in (0, 1, 2, 3, 4)]                  # vector seam
    out += [(words - 1 - j, 0x5A5A5A5A) for j in range(4)]            # the last four
    for c in range(256):                                              # every owner class,
        v = c + 256 * ((7 * c + 1) % blocks)                          # over the whole LDS
        out.append((4 * v + c % 4, 0x00010000 << (c % 16)))
    v = 256 * (blocks // 2 + 1) + 77                                  # one vector, each element
    out += [(4 * v + j, 0xFFFFFFFF) for j in range(4)]
    for b in range(32):                                               # every bit position
        v = 300 + 311 * b
        assert v < vecs
        out.append((4 * v + b % 4, 1 << b))
    picked = [w for w, _ in out]
    assert len(set(picked)) == len(picked) == 301
    classes = {(w // 4) % 256 for w in picked[9:265]}
    assert len(classes) == 256
    assert min(picked[9:265]) < 1024 and max(picked[9:265]) >= words - 2048
    return out


@pytest.mark.parametrize("phase", [0, 1])
def test_every_lds_word_class_is_read(ext, info, phase):
    words = info["sharedMemPerBlockOptin"] // 4
    picked = lds_coverage_words(words)
    rounds = 2
    calls = chunks([(0, LDS, i % rounds, w, mask, phase) for i, (w, mask) in enumerate(picked)])
    assert len(calls) == 5
    for inject in calls:
        raw = ext.cu_check(0, rounds, SEED, 0, inject)
        rec = raw["records"][0]
        print(f"phase {phase}: {len(inject)} words from {inject[0][3]}: counts {dict(rec['counts'])}")
        assert dict(rec["counts"]) == counts_of(lds=len(inject)), \
            (phase, [e[3] for e in inject])
        assert rec["first"]["test"] == "lds"


@pytest.mark.parametrize("phase", [0, 1])
def test_lds_report_names_the_right_word(ext, info, phase):
    cus = info["multiProcessorCount"]
    words = info["sharedMemPerBlockOptin"] // 4
    sample = [0, 3, 4, 259, 1023, 1024, 4 * 65, 4 * 130 + 1, words // 2 - 1, words // 2,
              words // 2 + 6, 4 * 7777 + 2, 4 * 9999 + 3, words - 1025, words - 4, words - 1]
    assert len(set(sample)) == 16 and cus >= 16
    inject = []
    for i, word in enumerate(sample):
        inject.append((i * (cus // 16), LDS, (0, 2)[i % 2], word, 1 << ((11 * i + 5) % 32), phase))
    raw = ext.cu_check(0, 3, SEED, 1, inject)
    recs = first_launch(raw)
    for wg, _, rnd, word, mask, _ in inject:
        rec = recs[wg]
        # one report per flipped word: the first verify stores the complement
        # of what it expected, so a phase 0 flip does not reach phase 1
        assert dict(rec["counts"]) == counts_of(lds=1), (wg, word, rec)
        first = rec["first"]
        who = cr.lds_verifier(word, phase)
        assert first["test"] == "lds"
        assert (first["round"], first["word"]) == (rnd, word), (wg, first)
        assert (first["wave"], first["lane"]) == (who["wave"], who["lane"]), (word, first, who)
        want = cr.lds_word(word, SEED, rnd, inverted=bool(phase))
        assert first["expected"] == want, (word, hex(first["expected"]), hex(want))
        assert first["actual"] == want ^ mask
    hit = {e[0] for e in inject}
    assert all(sum(r["counts"].values()) == 0 and r["first"] is None
               for wg, r in recs.items() if wg not in hit)


def word_verified_by(wave, lane, phase, block, elem, words):
    """A word whose verifier in `phase` is (wave, lane)."""
    v = (64 * wave + lane + cr.LDS_VERIFY_SHIFT[phase]) % 256 + 256 * block
    word = 4 * v + elem
    assert word < words
    who = cr.lds_verifier(word, phase)
    assert (who["wave"], who["lane"]) == (wave, lane)
    return word


def one_workgroup(ext, inject):
    raw = ext.cu_check(0, 3, SEED, 0, inject)
    assert raw["grid"] == 1 and raw["launches"] == 1
    rec = raw["records"][0]
    print(f"inject {inject}: counts {dict(rec['counts'])} first {rec['first']}")
    return rec


def test_fold_earlier_round_wins_over_lower_lane(ext):
    # wave 1: tile 9 is round 2, tile 1 is round 0
    rec = one_workgroup(ext, [(0, 1, 9, 0, LOW_BIT, 2), (0, 1, 1, 63, SIGN_BIT, 1)])
    assert dict(rec["counts"]) == counts_of(fp8=2)
    first = rec["first"]
    assert (first["test"], first["tile"], first["wave"], first["lane"], first["reg"]) == \
        ("fp8", 1, 1, 63, 1)
    want = cr.expected_bits("fp8", 1, SEED, 63, 1)
    assert (first["expected"], first["actual"]) == (want, want ^ SIGN_BIT)


def test_fold_orders_the_formats_inside_a_round(ext):
    # tile 6: round 1, wave 2. The later the step, the lower the lane.
    rec = one_workgroup(ext, [(0, 2, 6, 0, 0x4, 0), (0, 1, 6, 31, 0x2, 3), (0, 0, 6, 63, 0x100, 2)])
    assert dict(rec["counts"]) == counts_of(bf16=1, fp8=1, fp4=1)
    first = rec["first"]
    assert (first["test"], first["tile"], first["wave"], first["lane"], first["reg"]) == \
        ("bf16", 6, 2, 63, 2)
    want = cr.expected_bits("bf16", 6, SEED, 63, 2)
    assert (first["expected"], first["actual"]) == (want, want ^ 0x100)
    # fp8 before fp4, with bf16 clean
    rec = one_workgroup(ext, [(0, 2, 6, 0, 0x4, 0), (0, 1, 6, 31, 0x2, 3)])
    assert dict(rec["counts"]) == counts_of(fp8=1, fp4=1)
    assert (rec["first"]["test"], rec["first"]["lane"], rec["first"]["reg"]) == ("fp8", 31, 3)


def test_fold_puts_fp4_before_the_lds_verify(ext, info):
    words = info["sharedMemPerBlockOptin"] // 4
    word = word_verified_by(2, 5, 0, 17, 2, words)
    rec = one_workgroup(ext, [(0, LDS, 1, word, 0x8000, 0), (0, 2, 6, 63, 0x40, 3)])
    assert dict(rec["counts"]) == counts_of(fp4=1, lds=1)
    first = rec["first"]
    assert (first["test"], first["tile"], first["wave"], first["lane"], first["reg"]) == \
        ("fp4", 6, 2, 63, 3)
    # and the second LDS verify of round 0 before an accumulator of round 1
    word = word_verified_by(2, 40, 1, 3, 0, words)
    rec = one_workgroup(ext, [(0, 0, 6, 0, 0x40, 0), (0, LDS, 0, word, 0x8000, 1)])
    assert dict(rec["counts"]) == counts_of(bf16=1, lds=1)
    first = rec["first"]
    assert (first["test"], first["round"], first["word"], first["wave"], first["lane"]) == \
        ("lds", 0, word, 2, 40)


def test_fold_puts_the_first_lds_verify_before_the_second(ext, info):
    words = info["sharedMemPerBlockOptin"] // 4
    w0 = word_verified_by(3, 40, 0, 31, 1, words)
    w1 = word_verified_by(3, 3, 1, 2, 3, words)
    rec = one_workgroup(ext, [(0, LDS, 1, w1, 0x10, 1), (0, LDS, 1, w0, 0x20000, 0)])
    assert dict(rec["counts"]) == counts_of(lds=2)
    first = rec["first"]
    assert (first["test"], first["round"], first["word"], first["wave"], first["lane"]) == \
        ("lds", 1, w0, 3, 40)
    want = cr.lds_word(w0, SEED, 1)
    assert (first["expected"], first["actual"]) == (want, want ^ 0x20000)


class _RecordingExt:
    """The extension, keeping what cu_check returned."""

    def __init__(self, ext):
        self._ext = ext
        self.raw = []

    def __getattr__(self, name):
        return getattr(self._ext, name)

    def cu_check(self, *args):
        raw = self._ext.cu_check(*args)
        self.raw.append((args, raw))
        return raw


def test_production_shape_folds_real_records(ext, info, monkeypatch):
    from gpu_docker_api_amd.ops import hipcore

    cus = info["multiProcessorCount"]
    words = info["sharedMemPerBlockOptin"] // 4
    inject = [(0, 1, 5, 33, 0x00400000, 2), (cus, LDS, 1, words // 2 + 1, 0x1000, 1)]
    spy = _RecordingExt(ext)
    monkeypatch.setattr(hipcore, "_ext", spy)
    rep = hipcore.cu_check_gpu(0, 2, inject=inject)
    monkeypatch.undo()
    (args, raw), = spy.raw
    assert args[3] == 2 and raw["grid"] == 2 * cus and [tuple(e) for e in args[4]] == inject
    launches = raw["launches"]
    assert rep["launches"] == launches and rep["workgroups"] == launches * 2 * cus

    recs = first_launch(raw)
    assert dict(recs[0]["counts"]) == counts_of(fp8=1)
    assert dict(recs[cus]["counts"]) == counts_of(lds=1)
    f0, f1 = recs[0]["first"], recs[cus]["first"]
    assert (f0["tile"], f0["lane"], f0["reg"]) == (5, 33, 2)
    assert f0["expected"] == cr.expected_bits("fp8", 5, SEED, 33, 2)
    assert (f1["round"], f1["word"]) == (1, words // 2 + 1)
    assert f1["expected"] == cr.lds_word(words // 2 + 1, SEED, 1, inverted=True)
    assert all(sum(r["counts"].values()) == 0 for wg, r in recs.items() if wg not in (0, cus))

    # the fold against sums taken here, over every launch the pass needed
    per_cu = {}
    for r in raw["records"]:
        acc = per_cu.setdefault(hipcore.cu_check_key(r), counts_of())
        for t in TESTS:
            acc[t] += r["counts"][t]
    bad = {key: c for key, c in per_cu.items() if sum(c.values())}
    same = hipcore.cu_check_key(recs[0]) == hipcore.cu_check_key(recs[cus])
    print(f"workgroups 0 and {cus} ran on {'one CU' if same else 'two CUs'} "
          f"({hipcore.cu_check_key(recs[0]):#x}, {hipcore.cu_check_key(recs[cus]):#x}); "
          f"{launches} launch(es), {rep['cus_seen']} CUs seen")
    assert [b["key"] for b in rep["bad_cus"]] == sorted(bad)
    assert {b["key"]: b["tests"] for b in rep["bad_cus"]} == bad
    totals = {t: sum(c[t] for c in per_cu.values()) for t in TESTS}
    assert totals == counts_of(fp8=launches, lds=launches)
    assert rep["errors"] == {"total": 2 * launches, **totals}
    if launches == 1:
        assert len(bad) == (1 if same else 2)
        if same:  # the two workgroups' reports merged into one CU's
            assert rep["bad_cus"][0]["tests"] == counts_of(fp8=1, lds=1)
            assert rep["bad_cus"][0]["first"]["test"] == "fp8"
    assert rep["cus_seen"] == len(per_cu)


def test_inject_sub_out_of_range_is_rejected(ext):
    for entry in [
        (0, 0, 0, 0, 1, 4),          # no accumulator register 4
        (0, 2, 0, 0, 1, 4),
        (0, 3, 0, 0, 1, 2),          # no LDS phase 2
        (0, 3, 0, 0, 1, 3),          # a register number is no phase
        (0, 0, 0, 0, 1, 0, 0),       # seven elements
        (0, 0, 0, 0, 1, 1 << 32),    # sub wider than 32 bits
        (0, 3, 0, 0, 1, 1 << 32),
        (0, 0, 0, 0, 1, -1),
    ]:
        with pytest.raises(RuntimeError, match="inject"):
            ext.cu_check(0, 1, SEED, 0, [entry])
