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
