"""HBM pattern memory test on a real MI355X (csrc/hbm_memtest.hip).

The tensor bindings (memtest_write / memtest_verify / memtest_verify_flip)
are compared bit for bit with the torch reference of tests/memtest_refs.py,
computed on the device. Sizes come from memtest_geometry(), so they sit on
the kernel's own edges: the odd head and tail words, one workgroup tile, one
full trip of the capped grid (W words), and an index past 2^32.
"""
import numpy as np
import pytest

import memtest_refs as mr
from conftest import require_gpu

pytestmark = pytest.mark.gpu

SEED = mr.SEED
BASE = 12345  # odd: a vector's first word is odd or even depending on the view
GUARD = 0x5A5A5A5A5A5A5A5A
NGUARD = 4  # words before the view; keeps the aligned view 16-byte aligned
COMBOS = [("addr", False), ("rand", False), ("rand", True)]
COMBO_IDS = ["addr", "rand", "rand-inverted"]


@pytest.fixture(scope="module")
def ext():
    require_gpu()
    from gpu_docker_api_amd.ops import hipcore

    return hipcore.load_ext()


@pytest.fixture(scope="module")
def geo(ext):
    g = ext.memtest_geometry()
    tile = g["block"] * g["words_per_thread_iter"]  # one workgroup iteration
    return {"tile": tile, "W": tile * g["max_grid"]}


@pytest.fixture(scope="module")
def refs(geo):
    """Expected words BASE .. BASE + 2W + 6 for every pattern under test,
    built once on the device and never written to."""
    n = 2 * geo["W"] + 6
    return {
        (p, inv): mr.expected_torch(BASE, n, p, SEED, inv, device="cuda")
        for p, inv in COMBOS
    }


def make_view(n, aligned):
    """A length-n view 8-byte aligned (and 16-byte aligned only if asked),
    with guard words on both sides."""
    import torch

    buf = torch.full((n + 2 * NGUARD + 1,), GUARD, dtype=torch.int64, device="cuda")
    off = NGUARD if aligned else NGUARD + 1
    view = buf[off : off + n]
    if n:  # an empty view has no data pointer
        assert view.data_ptr() % 8 == 0 and (view.data_ptr() % 16 == 0) == aligned
    return buf, view, off


def assert_guards(buf, off, n, what):
    assert bool((buf[:off] == GUARD).all()), f"{what}: words before the view written"
    assert bool((buf[off + n :] == GUARD).all()), f"{what}: words after the view written"


def lengths(geo):
    t, W = geo["tile"], geo["W"]
    return [0, 1, 2, 3, 7, t - 1, t, t + 1, W - 1, W, W + 1, 2 * W + 5]


def u64_records(rep):
    return sorted(tuple(int(x) for x in r) for r in rep["records"])


def corrupt(view, base, pattern, invert, positions):
    """XOR a distinct mask into each position; returns the injected set as
    sorted (g, expected, actual) and the OR of the masks."""
    import torch

    positions = sorted(set(positions))
    masks = [(1 << ((7 * i) % 64)) | (1 << ((11 * i + 3) % 64)) for i in range(len(positions))]
    idx = torch.tensor(positions, dtype=torch.int64, device=view.device)
    view[idx] ^= torch.tensor([mr.to_i64(m) for m in masks], dtype=torch.int64,
                              device=view.device)
    g = [base + p for p in positions]
    exp = [int(w) for w in mr.pattern_np(g, pattern, SEED, invert)]
    injected = sorted((gi, e, e ^ m) for gi, e, m in zip(g, exp, masks))
    bits = 0
    for m in masks:
        bits |= m
    return injected, bits


# ---------------------------------------------------------------------------
# write
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("aligned", [True, False], ids=["aligned16", "aligned8"])
@pytest.mark.parametrize("combo", COMBOS, ids=COMBO_IDS)
def test_write_bit_exact(ext, geo, refs, combo, aligned):
    import torch

    pattern, invert = combo
    ref = refs[combo]
    for n in lengths(geo):
        buf, view, off = make_view(n, aligned)
        ext.memtest_write(view, pattern, SEED, BASE, invert)
        torch.cuda.synchronize()
        assert torch.equal(view, ref[:n]), f"{pattern} invert={invert} n={n}"
        assert_guards(buf, off, n, f"{pattern} n={n}")
        del buf, view


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned16", "aligned8"])
@pytest.mark.parametrize("combo", COMBOS, ids=COMBO_IDS)
def test_write_high_index(ext, combo, aligned):
    """The carry of g into its upper half, inside one 16-byte lane (aligned
    view) and between two lanes (odd view)."""
    import torch

    pattern, invert = combo
    base, n = 2**32 - 5, 64
    buf, view, off = make_view(n, aligned)
    ext.memtest_write(view, pattern, SEED, base, invert)
    torch.cuda.synchronize()
    ref = mr.expected_torch(base, n, pattern, SEED, invert, device="cuda")
    assert torch.equal(view, ref)
    assert_guards(buf, off, n, pattern)
    # and against the numpy definition, which never saw torch
    got = view.cpu().numpy().view(np.uint64)
    assert np.array_equal(got, mr.pattern_np(mr.arange_np(base, n), pattern, SEED, invert))


def test_write_zero_is_the_scrub(ext, geo):
    """The driver's scrub step is memtest_write's "zero" pattern."""
    import torch

    for aligned in (True, False):
        n = geo["tile"] * 3 + 5
        buf, view, off = make_view(n, aligned)
        view.fill_(-1)
        ext.memtest_write(view, "zero", SEED, BASE)
        torch.cuda.synchronize()
        assert not bool(view.any())
        assert_guards(buf, off, n, "zero")
        assert ext.memtest_verify(view, "zero", SEED, BASE)["errors"] == 0


def test_bindings_reject_bad_tensors(ext):
    import torch

    good = torch.zeros(16, dtype=torch.int64, device="cuda")
    bad = [
        torch.zeros(16, dtype=torch.int32, device="cuda"),
        torch.zeros(16, dtype=torch.int64),
        torch.zeros(32, dtype=torch.int64, device="cuda")[::2],
        torch.zeros(4, 4, dtype=torch.int64, device="cuda"),
    ]
    for t in bad:
        with pytest.raises(RuntimeError):
            ext.memtest_write(t, "rand", SEED)
        with pytest.raises(RuntimeError):
            ext.memtest_verify(t, "rand", SEED)
        with pytest.raises(RuntimeError):
            ext.memtest_verify_flip(t, "rand", SEED)
    with pytest.raises(RuntimeError):
        ext.memtest_write(good, "checkerboard", SEED)


# ---------------------------------------------------------------------------
# verify
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("aligned", [True, False], ids=["aligned16", "aligned8"])
@pytest.mark.parametrize("combo", COMBOS, ids=COMBO_IDS)
def test_verify_finds_exactly_what_was_flipped(ext, geo, combo, aligned):
    import torch

    pattern, invert = combo
    t, W = geo["tile"], geo["W"]
    head = 0 if aligned else 1
    # aligned: odd length -> a tail word; odd view: head word and tail word
    n = 2 * W + 5 if aligned else 2 * W + 6
    assert (n - head) % 2 == 1
    buf, view, off = make_view(n, aligned)
    ext.memtest_write(view, pattern, SEED, BASE, invert)
    clean = ext.memtest_verify(view, pattern, SEED, BASE, invert)
    assert clean == {"errors": 0, "bad_bits": 0, "records": []}

    positions = [
        0, n - 1,                    # first and last word
        head, head + 1,              # either side of the head/body seam
        n - 3, n - 2,                # last body lane, before the tail word
        head + 20, head + 21,        # both words of one 16-byte lane
        head + t - 1, head + t,      # workgroup tile seam
        W - 1, W, W + 1,             # one full grid trip
        head + W - 1, head + W,
    ]
    injected, bits = corrupt(view, BASE, pattern, invert, positions)
    rep = ext.memtest_verify(view, pattern, SEED, BASE, invert)
    assert rep["errors"] == len(injected)
    assert rep["bad_bits"] == bits
    assert u64_records(rep) == injected
    assert_guards(buf, off, n, "verify")
    # verify does not repair: the same set is reported again
    assert u64_records(ext.memtest_verify(view, pattern, SEED, BASE, invert)) == injected
    torch.cuda.synchronize()


def test_verify_record_cap(ext):
    import torch

    n = 100_003
    buf, view, off = make_view(n, aligned=False)
    ext.memtest_write(view, "rand", SEED, BASE)
    gen = torch.Generator().manual_seed(5)
    positions = torch.randperm(n, generator=gen)[:1000].tolist()
    injected, bits = corrupt(view, BASE, "rand", False, positions)
    assert len(injected) == 1000
    rep = ext.memtest_verify(view, "rand", SEED, BASE, False, 32)
    assert rep["errors"] == 1000
    assert rep["bad_bits"] == bits
    recs = u64_records(rep)
    assert len(recs) == 32
    assert len({r[0] for r in recs}) == 32, "a word was recorded twice"
    assert set(recs) <= set(injected)
    # no records wanted: the counts still hold
    rep0 = ext.memtest_verify(view, "rand", SEED, BASE, False, 0)
    assert rep0["errors"] == 1000 and rep0["bad_bits"] == bits and rep0["records"] == []


def test_verify_flip(ext, geo):
    import torch

    n = geo["tile"] * 3 + 6
    buf, view, off = make_view(n, aligned=False)  # head word and tail word
    ext.memtest_write(view, "rand", SEED, BASE)
    injected, bits = corrupt(view, BASE, "rand", False, [0, 1, 777, geo["tile"], n - 1])
    rep = ext.memtest_verify_flip(view, "rand", SEED, BASE)
    assert rep["errors"] == len(injected) and rep["bad_bits"] == bits
    assert u64_records(rep) == injected
    # complement of the EXPECTED word everywhere, also where the word was bad
    inverted = mr.expected_torch(BASE, n, "rand", SEED, True, device="cuda")
    assert torch.equal(view, inverted)
    assert_guards(buf, off, n, "verify_flip")
    # reported once: the next, inverted verify is clean
    assert ext.memtest_verify(view, "rand", SEED, BASE, True) == {
        "errors": 0, "bad_bits": 0, "records": []}
    # flipping the inverted pattern brings the plain one back
    assert ext.memtest_verify_flip(view, "rand", SEED, BASE, True)["errors"] == 0
    assert torch.equal(view, mr.expected_torch(BASE, n, "rand", SEED, False, device="cuda"))


def test_beyond_4gib(ext):
    """Byte offsets past 2^32 in one buffer of 4 GiB + 1 MiB."""
    import torch

    n = 2**29 + 2**17
    t = torch.empty(n, dtype=torch.int64, device="cuda")
    try:
        ext.memtest_write(t, "rand", SEED, 0)
        k = 512  # 4 KiB either side of byte offset 2^32
        lo = mr.expected_torch(2**29 - k, k, "rand", SEED, device="cuda")
        hi = mr.expected_torch(2**29, k, "rand", SEED, device="cuda")
        assert torch.equal(t[2**29 - k : 2**29], lo)
        assert torch.equal(t[2**29 : 2**29 + k], hi)
        assert torch.equal(t[n - k :], mr.expected_torch(n - k, k, "rand", SEED, device="cuda"))
        injected, bits = corrupt(t, 0, "rand", False, [0, 2**29 - 1, 2**29, n - 1])
        rep = ext.memtest_verify(t, "rand", SEED, 0)
        assert rep["errors"] == 4 and rep["bad_bits"] == bits
        assert u64_records(rep) == injected
    finally:
        del t
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# driver
# ---------------------------------------------------------------------------

CHUNKS = [1 << 30, 1 << 30, (1 << 20) + 16]


def test_driver_clean(ext):
    rep = ext.hbm_memtest(0, CHUNKS, SEED)
    assert rep["errors"] == 0 and rep["bad_bits"] == 0 and rep["records"] == []
    assert rep["bytes_tested"] == sum(CHUNKS)
    assert rep["passes"] == 6
    assert rep["write_gbps"] > 0 and rep["verify_gbps"] > 0 and rep["seconds"] > 0


def test_driver_finds_injected_errors(ext):
    w0, w1, w2 = (c // 8 for c in CHUNKS)
    inject = [
        (12345, 0x1),                          # inside the first chunk
        (w0, 0x8000000000000000),              # first word of the second chunk
        (w0 + w1 + w2 - 1, 0x00FF00000000FF00),  # last word of the third chunk
    ]
    rep = ext.hbm_memtest(0, CHUNKS, SEED, inject=inject)
    assert rep["errors"] == 3
    assert rep["bad_bits"] == 0x80FF00000000FF01
    # later steps are clean: "write rand" overwrites the injected words
    assert [r["step"] for r in rep["records"]] == ["verify addr"] * 3
    got = sorted((r["g"], r["expected"], r["expected"] ^ r["actual"]) for r in rep["records"])
    assert got == sorted((g, g ^ SEED, m) for g, m in inject)
    with pytest.raises(RuntimeError):
        ext.hbm_memtest(0, CHUNKS, SEED, inject=[(w0 + w1 + w2, 1)])


def test_driver_scrub_adds_a_pass(ext):
    rep = ext.hbm_memtest(0, [(1 << 20) + 8], SEED, scrub=True)
    assert rep["errors"] == 0 and rep["passes"] == 7


def test_memtest_gpu_and_validate_report(ext):
    from gpu_docker_api_amd.ops import hipcore

    plain = hipcore.validate_gpus(indices=[0], size=2048, iters=3)["gpus"][0]
    assert "memtest" not in plain
    g = hipcore.validate_gpus(indices=[0], size=2048, iters=3, memtest_mib=2048)["gpus"][0]
    assert g["memtest"]["errors"] == 0, g
    assert g["memtest"]["bytes_tested"] == 2048 << 20
    assert g["healthy"] == plain["healthy"]


def test_memtest_throughput_floor(ext):
    """Floors are 75 % of the slowest of three 8 GiB runs recorded in
    profiles/hbm_memtest.md."""
    rep = ext.hbm_memtest(0, [1 << 30] * 8, SEED)
    print(f"memtest 8 GiB: write {rep['write_gbps']:.0f} GB/s, "
          f"verify {rep['verify_gbps']:.0f} GB/s, {rep['seconds']:.2f} s")
    assert rep["errors"] == 0
    assert rep["verify_gbps"] > VERIFY_FLOOR, (
        f"memtest verify regressed: {rep['verify_gbps']:.0f} GB/s "
        f"(floor {VERIFY_FLOOR} = 75% of measured {VERIFY_MEASURED}; "
        f"write {rep['write_gbps']:.0f} GB/s)")
    assert rep["write_gbps"] > WRITE_FLOOR, (
        f"memtest write regressed: {rep['write_gbps']:.0f} GB/s "
        f"(floor {WRITE_FLOOR} = 75% of measured {WRITE_MEASURED}; "
        f"verify {rep['verify_gbps']:.0f} GB/s)")


# slowest of three 8 GiB repeats on the MI355X (profiles/hbm_memtest.md)
VERIFY_MEASURED = 4335
WRITE_MEASURED = 5259
VERIFY_FLOOR = 3250
WRITE_FLOOR = 3940


# ---------------------------------------------------------------------------
# Every word of a tile, every instantiation, indices past 2^32
#
# The tests above reach the comparator at about 15 positions of a tile and
# never above word index 2^32. Below, every failing assertion names the first
# missing or unexpected word by memtest_refs.word_class: tile, trip,
# workgroup, wave, lane, unroll slot, half of the 16-byte vector, and whether
# the tile took the unrolled path.
# ---------------------------------------------------------------------------

ALL_COMBOS = COMBOS + [("zero", False), ("zero", True)]
ALL_COMBO_IDS = COMBO_IDS + ["zero", "zero-inverted"]
ALIGNED = pytest.mark.parametrize("aligned", [True, False], ids=["aligned16", "aligned8"])
CLEAN = {"errors": 0, "bad_bits": 0, "records": []}


@pytest.fixture(scope="module")
def geometry(ext):
    g = dict(ext.memtest_geometry())
    assert g == mr.GEOMETRY  # word_class's CPU tests ran on this geometry
    return g


def expected_for(refs, pattern, invert, n):
    """The first n expected words from BASE, from the shared refs where they
    hold the combination; never written to."""
    import torch

    if pattern == "zero":
        return torch.full((n,), -1 if invert else 0, dtype=torch.int64, device="cuda")
    if (pattern, invert) in refs:
        return refs[(pattern, invert)][:n]
    return ~refs[(pattern, not invert)][:n]


def corrupt_with(view, base, pattern, invert, positions, masks):
    """corrupt() with the caller's masks. XOR: a second call restores."""
    import torch

    assert len(positions) == len(set(positions)) == len(masks)
    idx = torch.tensor(positions, dtype=torch.int64, device=view.device)
    view[idx] ^= torch.tensor([mr.to_i64(m) for m in masks], dtype=torch.int64,
                              device=view.device)
    g = [base + p for p in positions]
    exp = [int(w) for w in mr.pattern_np(g, pattern, SEED, invert)]
    injected = sorted((gi, e, e ^ m) for gi, e, m in zip(g, exp, masks))
    bits = 0
    for m in masks:
        bits |= m
    return injected, bits


def one_bit(p):
    """Over the 1024 .x words of a tile, and over its 1024 .y words, every one
    of the 64 bits comes up (test_every_word_of_a_tile_is_compared checks)."""
    return 1 << ((p + p // 64) % 64)


def where(p, base, head, n, geometry):
    return f"position {p} (g={(base + p) % 2**64:#x}): {mr.word_class(p, head, n, geometry)}"


def assert_report(rep, injected, bits, base, head, n, geometry, what):
    """errors, bad_bits and the record set equal what was injected."""
    got, want = set(u64_records(rep)), set(injected)
    if got != want or len(rep["records"]) != len(injected):
        parts = []
        for label, recs in (("missing", want - got), ("unexpected", got - want)):
            if recs:
                g, e, a = min(recs)
                p = (g - base) % 2**64
                cls = where(p, base, head, n, geometry) if p < n else f"g={g:#x}, outside the view"
                parts.append(f"{len(recs)} {label}, first at {cls}, "
                             f"expected {e:#018x}, actual {a:#018x}")
        if not parts:
            parts.append(f"{len(rep['records'])} records for {len(injected)} words")
        raise AssertionError(f"{what}: records differ from the {len(injected)} injected: "
                             + "; ".join(parts))
    first = where((injected[0][0] - base) % 2**64, base, head, n, geometry) if injected else "-"
    assert rep["errors"] == len(injected), (
        f"{what}: errors {rep['errors']} for {len(injected)} bad words, first at {first}")
    assert rep["bad_bits"] == bits, (
        f"{what}: bad_bits {rep['bad_bits']:#018x}, injected {bits:#018x}, first at {first}")


def assert_view(view, want, base, head, n, geometry, what):
    import torch

    if not torch.equal(view, want):
        bad = (view != want).nonzero().flatten()
        p = int(bad[0])
        raise AssertionError(
            f"{what}: {bad.numel()} of {n} words differ, first at "
            f"{where(p, base, head, n, geometry)}, holds {mr.to_u64(int(view[p])):#018x}, "
            f"expected {mr.to_u64(int(want[p])):#018x}")


def tile_words(tile, head, n, geo):
    """Positions of the body words of one tile."""
    body_end = head + 2 * ((n - head) // 2)
    lo = head + tile * geo["tile"]
    return list(range(lo, min(lo + geo["tile"], body_end)))


# --- indices at and past 2^32 ----------------------------------------------

def high_cases(t):
    """(id, base, length for an aligned view, the multiple of 2^32 in or next
    to the view). Lengths 3T + 5 (aligned) and 3T + 6 (odd view) make n - head
    odd: three full tiles, a bounds-checked one and a tail word."""
    return [
        ("2^32", 2**32, 3 * t + 5, 2**32),               # hoisted terms, new b
        ("5*2^32+12345", 5 * 2**32 + 12345, 3 * t + 5, None),
        ("2^40+7", 2**40 + 7, 3 * t + 5, None),
        ("2^63-3", 2**63 - 3, 3 * t + 5, 2**63),          # sign bit of the int64 view
        # 2^32 inside tile 1, a full unrolled tile whose terms are not
        # uniform; between two vectors or inside one, depending on alignment
        ("2^32-3T/2", 2**32 - 3 * t // 2, 3 * t + 5, 2**32),
        ("2^32-3T/2-1", 2**32 - 3 * t // 2 - 1, 3 * t + 5, 2**32),
        ("2^32-5", 2**32 - 5, 64, 2**32),                 # test_write_high_index's
    ]


HIGH_IDS = [c[0] for c in high_cases(2048)]


@ALIGNED
@pytest.mark.parametrize("combo", ALL_COMBOS, ids=ALL_COMBO_IDS)
@pytest.mark.parametrize("case", range(len(HIGH_IDS)), ids=HIGH_IDS)
def test_high_index_write_verify_flip(ext, geo, geometry, case, combo, aligned):
    import torch

    pattern, invert = combo
    t = geo["tile"]
    name, base, n, boundary = high_cases(t)[case]
    head = 0 if aligned else 1
    if n != 64:
        n += head
        assert (n - head) % 2 == 1
    what = f"{pattern} invert={invert} base={name} head={head} n={n}"
    buf, view, off = make_view(n, aligned)
    want = mr.expected_torch(base, n, pattern, SEED, invert, device="cuda")
    flipped = mr.expected_torch(base, n, pattern, SEED, not invert, device="cuda")

    ext.memtest_write(view, pattern, SEED, base, invert)
    torch.cuda.synchronize()
    assert_view(view, want, base, head, n, geometry, f"write {what}")
    assert_guards(buf, off, n, f"write {what}")
    # T words around the boundary against the numpy definition
    pb = boundary - base if boundary is not None else 0
    lo = max(0, min(pb - t // 2, n - t))
    k = min(t, n)
    got = view[lo : lo + k].cpu().numpy().view(np.uint64)
    ref = mr.pattern_np(mr.arange_np(base + lo, k), pattern, SEED, invert)
    assert np.array_equal(got, ref), (
        f"write {what}: differs from pattern_np, first at "
        f"{where(lo + int(np.flatnonzero(got != ref)[0]), base, head, n, geometry)}")

    assert ext.memtest_verify(view, pattern, SEED, base, invert) == CLEAN, (
        f"verify {what}: a clean buffer is reported")

    positions = {0, n - 1}
    if boundary is not None:
        positions |= {p for p in (pb - 1, pb, pb + 1) if 0 <= p < n}
        if head <= pb < head + 2 * ((n - head) // 2):  # both words of its vector
            v = pb - (pb - head) % 2
            positions |= {v, v + 1}
    ntiles = -(-((n - head) // 2) // (t // 2))
    for tile in range(ntiles):
        words = tile_words(tile, head, n, geo)
        positions |= {words[0], words[-1]}
    if n != 64:
        assert mr.word_class(n - 1, head, n, geometry) == "tail"
        if name.startswith("2^32-3T/2"):
            c = mr.word_class(pb, head, n, geometry)
            assert c.tile == 1 and c.full and c.half == (pb - head) % 2
    injected, bits = corrupt(view, base, pattern, invert, positions)
    rep = ext.memtest_verify(view, pattern, SEED, base, invert, 64)
    assert_report(rep, injected, bits, base, head, n, geometry, f"verify {what}")
    rep = ext.memtest_verify_flip(view, pattern, SEED, base, invert, 64)
    assert_report(rep, injected, bits, base, head, n, geometry, f"verify_flip {what}")
    assert_view(view, flipped, base, head, n, geometry, f"verify_flip {what}")
    assert_guards(buf, off, n, f"verify_flip {what}")
    assert ext.memtest_verify(view, pattern, SEED, base, not invert) == CLEAN, (
        f"verify after verify_flip {what}")


# --- every word of a tile ---------------------------------------------------

@ALIGNED
@pytest.mark.parametrize("combo", ALL_COMBOS, ids=ALL_COMBO_IDS)
@pytest.mark.parametrize("mode", ["verify", "verify_flip"])
def test_every_word_of_a_tile_is_compared(ext, geo, geometry, refs, mode, combo, aligned):
    """Each target tile is corrupted in three calls of its own: all its words,
    its .x words, its .y words, one bit per word."""
    pattern, invert = combo
    t, W, G = geo["tile"], geo["W"], geometry["max_grid"]
    head = 0 if aligned else 1
    run = getattr(ext, f"memtest_{mode}")
    views = [
        (3 * t + 6, [("full first-trip tile", 1, True), ("bounds-checked last tile", 3, False)]),
        # not in the issue's list: a bounds-checked tile that still has all
        # four slots and nearly every thread
        (2 * t - 3, [("bounds-checked tile, 1022 vectors", 1, False)]),
        (W + 2 * t + 5, [("second-trip tile", G, True),
                         ("bounds-checked tile after two trips", G + 2, False)]),
    ]
    for n, targets in views:
        buf, view, off = make_view(n, aligned)
        inv = invert
        ext.memtest_write(view, pattern, SEED, BASE, inv)
        for label, tile, full in targets:
            words = tile_words(tile, head, n, geo)
            c = mr.word_class(words[0], head, n, geometry)
            assert (c.tile, c.trip, c.workgroup, c.full) == (tile, tile // G, tile % G, full)
            assert len(words) == t or not full
            for half_name, half in (("all", None), (".x", 0), (".y", 1)):
                positions = [p for p in words if half is None or (p - head) % 2 == half]
                masks = [one_bit(p) for p in positions]
                if full and half is not None:
                    assert len(positions) == t // 2 and len(set(masks)) == 64
                what = (f"{mode} {pattern} invert={inv} head={head} n={n}, "
                        f"{label} {tile}, {half_name} words")
                injected, bits = corrupt_with(view, BASE, pattern, inv, positions, masks)
                rep = run(view, pattern, SEED, BASE, inv, 4096)
                assert_report(rep, injected, bits, BASE, head, n, geometry, what)
                assert_guards(buf, off, n, what)
                if mode == "verify":
                    corrupt_with(view, BASE, pattern, inv, positions, masks)  # restore
                else:
                    inv = not inv
                    assert ext.memtest_verify(view, pattern, SEED, BASE, inv) == CLEAN, (
                        f"{what}: the verify after it is not clean")
                assert_view(view, expected_for(refs, pattern, inv, n), BASE, head, n,
                            geometry, f"{what}: the view afterwards")
        del buf, view


@pytest.mark.parametrize("pattern", ["addr", "zero"])
def test_verify_flip_addr_and_zero(ext, geo, geometry, pattern):
    """test_verify_flip for the two patterns it leaves out."""
    n = geo["tile"] * 3 + 6
    buf, view, off = make_view(n, aligned=False)  # head word and tail word
    ext.memtest_write(view, pattern, SEED, BASE)
    injected, bits = corrupt(view, BASE, pattern, False, [0, 1, 777, geo["tile"], n - 1])
    rep = ext.memtest_verify_flip(view, pattern, SEED, BASE)
    assert_report(rep, injected, bits, BASE, 1, n, geometry, f"verify_flip {pattern}")
    # complement of the EXPECTED word everywhere, also where the word was bad
    inverted = mr.expected_torch(BASE, n, pattern, SEED, True, device="cuda")
    assert_view(view, inverted, BASE, 1, n, geometry, f"verify_flip {pattern}")
    assert_guards(buf, off, n, "verify_flip")
    # reported once: the next, inverted verify is clean
    assert ext.memtest_verify(view, pattern, SEED, BASE, True) == CLEAN
    # flipping the inverted pattern brings the plain one back
    assert ext.memtest_verify_flip(view, pattern, SEED, BASE, True) == CLEAN
    assert_view(view, mr.expected_torch(BASE, n, pattern, SEED, False, device="cuda"),
                BASE, 1, n, geometry, f"second verify_flip {pattern}")


# --- the per-wave reduction of cnt and bits ---------------------------------

def position_of(tile, wave, lane, slot, half, head, geometry):
    block = geometry["block"]
    unroll = geometry["words_per_thread_iter"] // 2
    vi = (tile * unroll + slot) * block + wave * 64 + lane
    return head + 2 * vi + half


@pytest.mark.parametrize("mode", ["verify", "verify_flip"])
def test_wave_reduction_counts_every_lane(ext, geo, geometry, mode):
    """One bad word in each of the 64 lanes of wave 2 of workgroup 1, then one
    in lane 63 alone of each wave: every lane's count reaches the report."""
    pattern, head = "rand", 1
    n = 3 * geo["tile"] + 6
    buf, view, off = make_view(n, aligned=False)
    run = getattr(ext, f"memtest_{mode}")
    inv = False
    ext.memtest_write(view, pattern, SEED, BASE, inv)
    calls = [("64 lanes of wave 2",
              [position_of(1, 2, lane, lane % 4, (lane // 4) % 2, head, geometry)
               for lane in range(64)])]
    calls += [(f"lane 63 of wave {w}", [position_of(1, w, 63, w, w % 2, head, geometry)])
              for w in range(4)]
    calls += [(f"lane {lane} of wave 1", [position_of(1, 1, lane, 2, 1, head, geometry)])
              for lane in (0, 1, 15, 16, 31, 32, 47, 48)]
    for label, positions in calls:
        classes = [mr.word_class(p, head, n, geometry) for p in positions]
        assert all(c.tile == 1 and c.full for c in classes)
        assert len({c.wave for c in classes}) == 1
        assert len({c.lane for c in classes}) == len(positions)
        masks = [one_bit(p) for p in positions]
        what = f"{mode}, {label}"
        injected, bits = corrupt_with(view, BASE, pattern, inv, positions, masks)
        rep = run(view, pattern, SEED, BASE, inv, 128)
        assert_report(rep, injected, bits, BASE, head, n, geometry, what)
        assert rep["errors"] == len(positions)
        if mode == "verify":
            corrupt_with(view, BASE, pattern, inv, positions, masks)
        else:
            inv = not inv
    assert ext.memtest_verify(view, pattern, SEED, BASE, inv) == CLEAN
    assert_guards(buf, off, n, mode)


@pytest.mark.parametrize("mode", ["verify", "verify_flip"])
def test_last_workgroup_of_the_grid_reports(ext, geo, geometry, refs, mode):
    """Bad words in workgroup max_grid - 1 only, in every wave."""
    pattern, head = "rand", 0
    G = geometry["max_grid"]
    n = geo["W"] + 5
    buf, view, off = make_view(n, aligned=True)
    ext.memtest_write(view, pattern, SEED, BASE)
    positions = [position_of(G - 1, w, lane, slot, half, head, geometry)
                 for w in range(4) for lane, slot, half in ((0, 0, 0), (17, 1, 1), (63, 3, 1))]
    assert all(mr.word_class(p, head, n, geometry).workgroup == G - 1 for p in positions)
    assert mr.word_class(positions[-1], head, n, geometry) == (G - 1, 0, G - 1, 3, 63, 3, 1, True)
    masks = [one_bit(p) for p in positions]
    injected, bits = corrupt_with(view, BASE, pattern, False, positions, masks)
    rep = getattr(ext, f"memtest_{mode}")(view, pattern, SEED, BASE, False, 64)
    assert_report(rep, injected, bits, BASE, head, n, geometry, f"{mode}, workgroup {G - 1}")
    if mode == "verify_flip":
        assert_view(view, expected_for(refs, pattern, True, n), BASE, head, n, geometry, mode)
    assert_guards(buf, off, n, mode)


# --- driver: every step reports, odd chunks, a base past 2^32 ---------------

STEPS = ["write addr", "verify addr", "write rand", "verify rand", "verify_flip rand",
         "verify rand inverted"]
TILE = mr.GEOMETRY["block"] * mr.GEOMETRY["words_per_thread_iter"]
# an odd word count (the next chunk's base g is odd), a chunk smaller than one
# vector pair, a single word, two full tiles
ODD_CHUNKS = [8 * (TILE + 3), 8 * 5, 8 * 1, 8 * (2 * TILE)]
ODD_STARTS = [0, TILE + 3, TILE + 8, TILE + 9]
ODD_WORDS = 3 * TILE + 9


def driver_expected(entries, base_word):
    """What a run with these (word, mask[, step]) entries must report:
    sorted (step index, g, expected, actual), and the OR of the reported
    masks. A flip before a write is overwritten; a verify does not repair, so
    a flip before "verify rand" is seen again by "verify_flip rand", which
    stores the complement of the expected word and so ends it."""
    recs, bits = [], 0
    for word, mask, *rest in entries:
        step = rest[0] if rest else 1
        g = base_word + word
        addr = int(mr.pattern_np([g], "addr", SEED)[0])
        rand = int(mr.pattern_np([g], "rand", SEED)[0])
        seen = {0: [], 1: [(1, addr)], 2: [], 3: [(3, rand), (4, rand)], 4: [(4, rand)],
                5: [(5, rand ^ mr.M64)]}[step]
        for s, e in seen:
            recs.append((s, g, e, e ^ mask))
            bits |= mask
    return sorted(recs), bits


def assert_driver(rep, entries, base_word, passes, what):
    want, bits = driver_expected(entries, base_word)
    names = [r["step"] for r in rep["records"]]
    assert all(nm in STEPS for nm in names), f"{what}: {names}"
    order = [STEPS.index(nm) for nm in names]
    assert order == sorted(order), f"{what}: records are not in run order: {names}"
    got = sorted((STEPS.index(r["step"]), r["g"], r["expected"], r["actual"])
                 for r in rep["records"])
    assert got == want, (
        f"{what}: missing {[(STEPS[s], hex(g)) for s, g, _, _ in sorted(set(want) - set(got))]}, "
        f"unexpected {[(STEPS[s], hex(g), hex(e), hex(a)) for s, g, e, a in sorted(set(got) - set(want))]}")
    assert rep["errors"] == len(want), f"{what}: errors {rep['errors']}, expected {len(want)}"
    assert rep["bad_bits"] == bits, f"{what}: bad_bits {rep['bad_bits']:#x}, expected {bits:#x}"
    assert rep["passes"] == passes
    assert rep["bytes_tested"] == sum(ODD_CHUNKS)


# one flip per step: (word, mask, step); the words sit on chunk edges
STEP_FLIPS = [
    (5, 0x1, 0),
    (TILE + 2, 0x8000000000000000, 1),       # tail word of chunk 0
    (TILE + 8, 0xFFFFFFFFFFFFFFFF, 2),       # the single word of chunk 2
    (TILE + 3, 0x0000000100000000, 3),       # first word of chunk 1, odd g
    (TILE + 9, 0x00FF00000000FF00, 4),       # first word of chunk 3
    (3 * TILE + 8, 0x4000000000000002, 5),   # last word of chunk 3
]


@pytest.mark.parametrize("scrub", [False, True], ids=["plain", "scrub"])
@pytest.mark.parametrize("step", range(6), ids=[s.replace(" ", "-") for s in STEPS])
def test_driver_flip_before_each_step(ext, step, scrub):
    entry = STEP_FLIPS[step]
    assert entry[2] == step
    rep = ext.hbm_memtest(0, ODD_CHUNKS, SEED, scrub=scrub, inject=[entry])
    assert_driver(rep, [entry], 0, 7 if scrub else 6, f"flip before {STEPS[step]!r}")
    reported = {1: ["verify addr"], 3: ["verify rand", "verify_flip rand"],
                4: ["verify_flip rand"], 5: ["verify rand inverted"]}.get(step, [])
    assert [r["step"] for r in rep["records"]] == reported
    assert rep["errors"] == len(reported)


@pytest.mark.parametrize("scrub", [False, True], ids=["plain", "scrub"])
def test_driver_flips_before_all_steps_in_one_run(ext, scrub):
    rep = ext.hbm_memtest(0, ODD_CHUNKS, SEED, scrub=scrub, inject=STEP_FLIPS)
    assert_driver(rep, STEP_FLIPS, 0, 7 if scrub else 6, "one flip before every step")
    assert [r["step"] for r in rep["records"]] == [
        "verify addr", "verify rand", "verify_flip rand", "verify_flip rand",
        "verify rand inverted"]
    assert rep["errors"] == 5
    # a two-element entry is a flip before "verify addr"
    two = ext.hbm_memtest(0, ODD_CHUNKS, SEED, inject=[(TILE + 2, 0x8000000000000000)])
    one = ext.hbm_memtest(0, ODD_CHUNKS, SEED, inject=[(TILE + 2, 0x8000000000000000, 1)])
    assert two["records"] == one["records"] and two["errors"] == one["errors"] == 1


def edge_words():
    """Last word of chunk 0, first of chunk 1, the word of chunk 2, first and
    last of chunk 3."""
    return [TILE + 2, TILE + 3, TILE + 8, TILE + 9, 3 * TILE + 8]


def test_driver_odd_chunks(ext):
    assert ODD_STARTS == [sum(ODD_CHUNKS[:i]) // 8 for i in range(4)]
    assert ODD_WORDS == sum(ODD_CHUNKS) // 8 and edge_words()[-1] == ODD_WORDS - 1
    clean = ext.hbm_memtest(0, ODD_CHUNKS, SEED)
    assert clean["errors"] == 0 and clean["bad_bits"] == 0 and clean["records"] == []
    assert clean["passes"] == 6 and clean["bytes_tested"] == sum(ODD_CHUNKS)
    for step in (None, 3, 5):
        entries = [(w, 1 << ((9 * i + 7 * (step or 1)) % 64)) + (() if step is None else (step,))
                   for i, w in enumerate(edge_words())]
        rep = ext.hbm_memtest(0, ODD_CHUNKS, SEED, inject=entries)
        assert_driver(rep, entries, 0, 6, f"odd chunks, flips before step {step}")


@pytest.mark.parametrize("base_word", [2**32 - TILE - 4, 2**32],
                         ids=["2^32-T-4", "2^32"])
def test_driver_high_base(ext, base_word):
    """The same chunks with g running through 2^32 (inside the 5-word chunk,
    so chunk 3's full tiles take the hoisted path with a new upper half) and
    starting at it."""
    clean = ext.hbm_memtest(0, ODD_CHUNKS, SEED, base_word=base_word)
    assert clean["errors"] == 0 and clean["bad_bits"] == 0 and clean["records"] == []
    words = sorted({g - base_word for g in (2**32 - 1, 2**32, 2**32 + 1)
                    if 0 <= g - base_word < ODD_WORDS} | set(edge_words()))
    assert {base_word + w for w in words} >= {2**32, 2**32 + 1}
    for step in (1, 3, 5):
        entries = [(w, 1 << ((5 * i + 11 * step) % 64), step) for i, w in enumerate(words)]
        rep = ext.hbm_memtest(0, ODD_CHUNKS, SEED, inject=entries, base_word=base_word)
        assert_driver(rep, entries, base_word, 6,
                      f"base_word {base_word:#x}, flips before step {step}")
        assert {r["g"] for r in rep["records"]} == {base_word + w for w in words}
    # inject words stay positions: the range check does not move with the base
    with pytest.raises(RuntimeError):
        ext.hbm_memtest(0, ODD_CHUNKS, SEED, inject=[(ODD_WORDS, 1)], base_word=base_word)


def test_driver_rejects_malformed_inject_entries(ext):
    for bad in ([(5, 1, 6)], [(5, 1, -1)], [(5, 1, 2**40)], [(5,)], [(5, 1, 1, 1)], [()],
                [(5, 1), (6, 1, 7)], [5], [(-1, 1)], [(5, 2**64)]):
        with pytest.raises((RuntimeError, TypeError)):
            ext.hbm_memtest(0, ODD_CHUNKS, SEED, inject=bad)
    # entries may be lists, and the run after the rejections is clean
    rep = ext.hbm_memtest(0, ODD_CHUNKS, SEED, inject=[[5, 1, 1]])
    assert rep["errors"] == 1 and rep["records"][0]["g"] == 5
