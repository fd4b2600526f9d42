"""The checked GEMM loop's comparators on a real MI355X (csrc/gemm_check.hip).

tests/test_gemm_check_gpu.py holds each stage to the numpy port at a handful
of places. This file holds what the verifier and the operand check compare:
every row, column, row slot, lane and element of a tile, the integer widths of
the two combines at their limits, the malformed rule at its boundary, the
expected sums past one pass of eight tiles, the fill and the operand check
past one grid trip, and a flipped operand word through GEMM, verifier, fold
and operand check. Every verifier case runs with the column sums combined
through the slab and through the atomic accumulator; every assertion is
bit-exact or an integer count, and a missing or unexpected row or column is
named by gemm_check_refs.verify_class.

Corruptions are made by storing (n + d) granules, n from the port's product,
into a clone of the GEMM's result: exact, and it works where n == 0.
"""
import numpy as np
import pytest

import gemm_check_refs as gr
import kernel_refs as kr
from test_gemm_check_gpu import (SEED, SEEDS, KINDS, assert_matches_port, ext,  # noqa: F401
                                 findings, int_product, problem, rng_of, run_gemm, to_numpy)

pytestmark = pytest.mark.gpu

ATOMIC = pytest.mark.parametrize("atomic", [False, True], ids=["slab", "atomic"])
TILES_N, NWG = 3, 6  # of the base problem
TWO24 = gr.TWO24
PERMS = {
    "identity": lambda r: r,
    "reversal": lambda r: 255 - r,
    "affine": lambda r: (37 * r + 11) % 256,  # row slot, lane and element vary independently
}
PERM = pytest.mark.parametrize("perm", list(PERMS))
CLEAN = {"rows": 0, "cols": 0, "malformed": 0}


def base(ext, kind):
    """2 x 3 tiles at the kind's smallest K: the verifier does not depend on K."""
    return problem(ext, kind, 512, 768, gr.MIN_K[kind])


def verify(ext, p, C, atomic, max_records=1024, seed=SEED):
    return ext.gemm_check_verify(p["kind"], C, p["K"], seed, p["range"], max_records, atomic)


def store_granules(p, rows, cols, y):
    """A clone of C with y (integers, product granules) at (rows, cols)."""
    import torch

    y = np.asarray(y, dtype=np.int64)
    assert int(np.abs(y).max()) <= TWO24  # then y * granule is exact in fp32
    C = p["C"].clone()
    C[torch.as_tensor(np.asarray(rows), device="cuda"),
      torch.as_tensor(np.asarray(cols), device="cuda")] = torch.tensor(
          y.astype(np.float64) / p["inv"], dtype=torch.float32, device="cuda")
    return C


def store_bits(p, rows, cols, bits):
    """A clone of C with the fp32 bit patterns `bits` at (rows, cols)."""
    import torch

    b = np.asarray(bits, dtype=np.uint32).view(np.int32)
    C = p["C"].clone()
    C.view(torch.int32)[torch.as_tensor(np.asarray(rows), device="cuda"),
                        torch.as_tensor(np.asarray(cols), device="cuda")] = torch.as_tensor(
                            b, device="cuda")
    return C


def lines(raw, kind_):
    """{(tile_row, tile_col, index): (got, want)} of the row or col records."""
    out = {}
    for r in raw["records"]:
        if r["type"] == kind_:
            key = (r["tile_row"], r["tile_col"], r["index"])
            assert key not in out, f"{kind_} {key} reported twice"
            out[key] = (r["got"], r["want"])
    return out


def assert_lines(raw, kind_, want, elements, what):
    """The row (col) records are exactly `want`; `elements` maps a line to
    the in-tile (row, col) that was corrupted in it, for the message."""
    got = set(lines(raw, kind_))
    missing, extra = sorted(set(want) - got), sorted(got - set(want))
    if missing or extra:
        first = (missing or extra)[0]
        rc = elements.get(first)
        where = f"element {rc}: {gr.verify_class(*rc)}, col_check thread {rc[1]}" if rc else \
            "no corrupted element"
        raise AssertionError(
            f"{what}: {len(missing)} {kind_}s missing, {len(extra)} unexpected; first "
            f"{'missing' if missing else 'unexpected'} {kind_} {first[2]} of tile "
            f"({first[0]}, {first[1]}), {where}")


def tile_case(p, ti, tj, pi):
    """Rows, columns (global) and the maps line -> in-tile element of the 256
    elements (r, pi(r)) of tile (ti, tj)."""
    r = np.arange(256)
    c = pi(r)
    assert sorted(c.tolist()) == list(range(256))
    row_el = {(ti, tj, int(a)): (int(a), int(b)) for a, b in zip(r, c)}
    col_el = {(ti, tj, int(b)): (int(a), int(b)) for a, b in zip(r, c)}
    return ti * 256 + r, tj * 256 + c, row_el, col_el


# ---------------------------------------------------------------------------
# 1. every row and every column reports
# ---------------------------------------------------------------------------

@ATOMIC
@PERM
@pytest.mark.parametrize("kind", KINDS)
def test_every_row_and_column_reports(ext, kind, perm, atomic):
    p = base(ext, kind)
    for ti, tj in ((1, 2), (0, 1), (1, 0)):  # (1, 2) is the last tile
        rows, cols, row_el, col_el = tile_case(p, ti, tj, PERMS[perm])
        d = np.where(np.arange(256) % 2 == 0, 1, -1)
        C = store_granules(p, rows, cols, p["n"][rows, cols] + d)
        raw = verify(ext, p, C, atomic)
        what = f"{kind} {perm} tile ({ti}, {tj})"
        assert_lines(raw, "row", row_el, row_el, what)
        assert_lines(raw, "col", col_el, col_el, what)
        assert raw["errors"] == {"rows": 256, "cols": 256, "malformed": 0}, what
        assert len(raw["records"]) == 512
        for key, (got, want) in lines(raw, "row").items():
            assert got - want == d[row_el[key][0]], (what, "row", key, gr.verify_class(*row_el[key]))
            assert want == int(p["R"][key]), (what, "row", key)
        for key, (got, want) in lines(raw, "col").items():
            assert got - want == d[col_el[key][0]], (what, "col", key, gr.verify_class(*col_el[key]))
            assert want == int(p["Q"][key]), (what, "col", key)
        assert_matches_port(p, C, raw)


# ---------------------------------------------------------------------------
# 2. one error alone, at every class
# ---------------------------------------------------------------------------

LANES = (0, 15, 16, 31, 32, 47, 48, 63)


def lone_cases():
    """64 (tile_row, tile_col, row, col, delta): every strip x wave pair four
    times, every row slot, every element of a vector and the eight lanes at
    the edges of the 16-lane groups."""
    out = []
    for i in range(64):
        s, w, q = i // 16, (i // 4) % 4, i % 4
        j = (4 * q + w + s) % 16
        lane, e = LANES[(i + i // 8) % 8], (i + i // 4) % 4
        t = i % NWG
        out.append((t // TILES_N, t % TILES_N, 64 * s + 16 * w + j, 4 * lane + e,
                    (1 + i % 3) * (1 if i % 2 else -1)))
    k = [gr.verify_class(c[2], c[3]) for c in out]
    assert {(x.strip, x.wave) for x in k} == {(s, w) for s in range(4) for w in range(4)}
    assert {x.j for x in k} == set(range(16)) and {x.e for x in k} == set(range(4))
    assert {x.lane for x in k} == set(LANES)
    assert {(x.lane, x.e) for x in k} >= {(0, 0), (63, 3)}  # the tile's first and last column
    return out


@ATOMIC
@pytest.mark.parametrize("kind", KINDS)
def test_one_error_alone_at_every_class(ext, kind, atomic):
    from gpu_docker_api_amd.ops.hipcore import gemm_check_fold

    p = base(ext, kind)
    for ti, tj, r, c, d in lone_cases():
        row, col = ti * 256 + r, tj * 256 + c
        what = f"{kind} tile ({ti}, {tj}) element ({r}, {c}): {gr.verify_class(r, c)}"
        C = store_granules(p, [row], [col], [int(p["n"][row, col]) + d])
        raw = verify(ext, p, C, atomic)
        assert raw["errors"] == {"rows": 1, "cols": 1, "malformed": 0}, what
        assert lines(raw, "row") == {(ti, tj, r): (int(p["R"][ti, tj, r]) + d,
                                                   int(p["R"][ti, tj, r]))}, what
        assert lines(raw, "col") == {(ti, tj, c): (int(p["Q"][ti, tj, c]) + d,
                                                   int(p["Q"][ti, tj, c]))}, what
        assert_matches_port(p, C, raw)
        (tile,) = gemm_check_fold(raw, TILES_N, NWG, False)["bad_tiles"]
        assert tile["tile"] == [ti, tj], what
        assert tile["element"] == {"row": row, "col": col, "delta": d}, what
        assert (tile["block"], tile["block_mod8"]) == kr.owner_block(ti, tj, TILES_N, NWG, False)


# ---------------------------------------------------------------------------
# 3. the integer widths
# ---------------------------------------------------------------------------

def tile_of_granules(p, ti, tj, y):
    """A clone of C with tile (ti, tj) set to y [256][256] granules."""
    import torch

    assert int(np.abs(y).max()) <= TWO24
    C = p["C"].clone()
    C[ti * 256:(ti + 1) * 256, tj * 256:(tj + 1) * 256] = torch.tensor(
        y.astype(np.float64) / p["inv"], dtype=torch.float32, device="cuda")
    return C


def assert_tile_sums(p, raw, ti, tj, y, what):
    """Every record is of tile (ti, tj), with `got` the sums of y and `want`
    the port's; rows and columns whose sum equals the port's are absent."""
    R, Q = p["R"][ti, tj], p["Q"][ti, tj]
    row_sum, col_sum = y.sum(axis=1), y.sum(axis=0)
    want_rows = {(ti, tj, i): (int(row_sum[i]), int(R[i])) for i in range(256)
                 if row_sum[i] != R[i]}
    want_cols = {(ti, tj, i): (int(col_sum[i]), int(Q[i])) for i in range(256)
                 if col_sum[i] != Q[i]}
    for kind_, want, el in (("row", want_rows, {k: (k[2], 0) for k in want_rows}),
                            ("col", want_cols, {k: (0, k[2]) for k in want_cols})):
        assert_lines(raw, kind_, want, el, what)
        for key, pair in sorted(lines(raw, kind_).items()):
            assert pair == want[key], (
                f"{what}: {kind_} {key[2]} of tile ({ti}, {tj}) has (got, want) {pair}, "
                f"the sums of what was stored and the port give {want[key]}")
    assert raw["errors"] == {"rows": len(want_rows), "cols": len(want_cols), "malformed": 0}, what


@ATOMIC
@pytest.mark.parametrize("kind", KINDS)
def test_integer_widths_of_the_row_and_column_combines(ext, kind, atomic):
    """A 16-lane partial reaches 2^30, the four-group row sum 2^32, a strip's
    column sum 2^30 and the four-strip column sum 2^32 in magnitude."""
    p = base(ext, kind)
    ti, tj = 1, 2
    n = p["n"][ti * 256:(ti + 1) * 256, tj * 256:(tj + 1) * 256]
    cases = [("whole tile +2^24", np.full((256, 256), TWO24, dtype=np.int64)),
             ("whole tile -2^24", np.full((256, 256), -TWO24, dtype=np.int64))]
    for strip in range(4):
        y = np.full((256, 256), -TWO24, dtype=np.int64)
        y[64 * strip:64 * strip + 64] = TWO24
        cases.append((f"strip {strip} +2^24, the others -2^24", y))
    for strip, wave in ((1, 2), (3, 0), (0, 3)):
        y = n.copy()
        y[64 * strip + 16 * wave:64 * strip + 16 * wave + 16] = TWO24
        cases.append((f"wave {wave} of strip {strip} +2^24, the rest clean", y))
    for name, y in cases:
        what = f"{kind} {name}"
        C = tile_of_granules(p, ti, tj, y)
        raw = verify(ext, p, C, atomic)
        assert_tile_sums(p, raw, ti, tj, y, what)
        rows, cols = lines(raw, "row"), lines(raw, "col")
        if name.startswith("whole"):
            sign = 1 if "+" in name else -1
            assert len(rows) == len(cols) == 256, what
            assert {g for g, _ in rows.values()} == {sign * 2**32}, what
            assert {g for g, _ in cols.values()} == {sign * 2**32}, what
        elif name.startswith("strip"):
            assert len(rows) == len(cols) == 256, what
            assert {g for g, _ in cols.values()} == {-2**31}, what
            assert sorted({g for g, _ in rows.values()}) == [-2**32, 2**32], what
        else:
            assert len(rows) == 16 and {g for g, _ in rows.values()} == {2**32}, what
        assert_matches_port(p, C, raw)


# ---------------------------------------------------------------------------
# 4. the malformed boundary and coordinates
# ---------------------------------------------------------------------------

def f32_bits(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def boundary_table(p):
    """(name, fp32 bits, accepted as y granules or None if malformed)."""
    g = 1.0 / p["inv"]  # a power of two: scaling by it is exact
    top = f32_bits(TWO24 * g)
    return [
        ("+2^24", top, TWO24),
        ("-2^24", top | 0x80000000, -TWO24),
        ("next above +2^24", top + 1, None),
        ("next below -2^24", (top + 1) | 0x80000000, None),
        ("+Inf", 0x7F800000, None),
        ("-Inf", 0xFF800000, None),
        ("NaN with the sign bit", 0xFFC00001, None),
        ("smallest denormal", 0x00000001, None),
        ("half a granule", f32_bits(0.5 * g), None),
        ("minus half a granule", f32_bits(-0.5 * g), None),
        ("-0.0", 0x80000000, 0),
    ]


@ATOMIC
@pytest.mark.parametrize("kind", KINDS)
def test_malformed_boundary_at_one_element(ext, kind, atomic):
    p = base(ext, kind)
    ti, tj, r, c = 1, 2, 44, 3
    while int(p["n"][ti * 256 + r, tj * 256 + c]) == 0:
        c += 1
    row, col = ti * 256 + r, tj * 256 + c
    n = int(p["n"][row, col])
    for name, bits, y in boundary_table(p):
        what = f"{kind} {name} ({bits:#010x}) at ({row}, {col})"
        C = store_bits(p, [row], [col], [bits])
        raw = verify(ext, p, C, atomic)
        delta = (0 if y is None else y) - n  # a malformed element contributes 0
        assert delta != 0
        assert raw["errors"] == {"rows": 1, "cols": 1, "malformed": int(y is None)}, what
        bad = [rec for rec in raw["records"] if rec["type"] == "malformed"]
        if y is None:
            (rec,) = bad
            assert (rec["tile_row"], rec["tile_col"], rec["row"], rec["col"]) == (ti, tj, r, c), what
            assert rec["bits"] == bits, what
        else:
            assert bad == [], what
        R, Q = int(p["R"][ti, tj, r]), int(p["Q"][ti, tj, c])
        assert lines(raw, "row") == {(ti, tj, r): (R + delta, R)}, what
        assert lines(raw, "col") == {(ti, tj, c): (Q + delta, Q)}, what
        assert_matches_port(p, C, raw)


@ATOMIC
@PERM
@pytest.mark.parametrize("kind", KINDS)
def test_malformed_records_name_every_row_and_column(ext, kind, perm, atomic):
    p = base(ext, kind)
    ti, tj = 0, 1
    rows, cols, _, _ = tile_case(p, ti, tj, PERMS[perm])
    r, c = rows - ti * 256, cols - tj * 256
    bits = 0x7FC00000 | (r << 8) | c  # NaNs, each with its place as payload
    C = store_bits(p, rows, cols, bits)
    raw = verify(ext, p, C, atomic)
    assert raw["errors"]["malformed"] == 256
    got = sorted((rec["tile_row"], rec["tile_col"], rec["row"], rec["col"], rec["bits"])
                 for rec in raw["records"] if rec["type"] == "malformed")
    want = sorted((ti, tj, int(a), int(b), int(v)) for a, b, v in zip(r, c, bits))
    if got != want:
        first = sorted(set(want) - set(got) or set(got) - set(want))[0]
        raise AssertionError(f"{kind} {perm}: {len(set(want) - set(got))} malformed records "
                             f"missing, {len(set(got) - set(want))} unexpected; first {first}: "
                             f"{gr.verify_class(first[2], first[3])}")
    # each row and column misses its element's n: as the port says
    n = p["n"][rows, cols]
    assert raw["errors"]["rows"] == raw["errors"]["cols"] == int(np.count_nonzero(n))
    for (_, _, i), (g, w) in lines(raw, "row").items():
        assert g - w == -int(n[i]) and w == int(p["R"][ti, tj, i])
    assert_matches_port(p, C, raw)


@ATOMIC
@pytest.mark.parametrize("kind", KINDS)
def test_a_poisoned_tile_is_malformed_in_full_and_alone(ext, kind, atomic):
    import torch

    p = base(ext, kind)
    ti, tj = 1, 1
    C = p["C"].clone()
    C.view(torch.int32)[ti * 256:(ti + 1) * 256, tj * 256:(tj + 1) * 256] = gr.POISON_BITS
    cap = 65536  # the most a call takes: 65536 of the 65536 + 512 findings get a record
    raw = verify(ext, p, C, atomic, max_records=cap)
    want = gr.classify(C.cpu().numpy(), p["inv"], p["R"], p["Q"])
    assert len(want["malformed"]) == 65536
    assert {(a // 256, b // 256) for a, b in want["malformed"]} == {(ti, tj)}
    # every sum of the tile is 0 now, and none of the expected ones is
    assert len(want["rows"]) == len(want["cols"]) == 256
    assert raw["errors"] == {"rows": 256, "cols": 256, "malformed": 65536}
    assert len(raw["records"]) == cap
    assert {(rec["tile_row"], rec["tile_col"]) for rec in raw["records"]} == {(ti, tj)}
    f = findings(raw)
    assert len(set(f["malformed"])) == len(f["malformed"])
    assert set(f["malformed"]) <= set(want["malformed"])
    assert set(f["rows"]) <= set(want["rows"]) and set(f["cols"]) <= set(want["cols"])
    assert all(rec["bits"] == gr.POISON_BITS for rec in raw["records"]
               if rec["type"] == "malformed")
    for key, (g, w) in list(lines(raw, "row").items()) + list(lines(raw, "col").items()):
        assert g == 0 and w != 0


# ---------------------------------------------------------------------------
# 5. expected sums past eight tiles
# ---------------------------------------------------------------------------

PAST_EIGHT = [(256, 2304), (2304, 256), (4352, 512), (2048, 2304)]

_ports = {}


def port_sums(kind, M, N, K, seed, r):
    key = (kind, M, N, K, seed, r)
    if key not in _ports:
        _ports[key] = gr.expected_sums(gr.numerators(kind, 0, M, K, seed, r),
                                       gr.numerators(kind, 1, N, K, seed, r))
    return _ports[key]


def assert_sums_equal(got, want, name, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i, j, x = (int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {want.size} entries of {name} differ, first "
                             f"{name}[{i}][{j}][{x}] = {int(got[i, j, x])}, the port has "
                             f"{int(want[i, j, x])}")


@pytest.mark.parametrize("seed", SEEDS, ids=["seed0", "seed"])
@pytest.mark.parametrize("shape", PAST_EIGHT, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", KINDS)
def test_expected_sums_past_eight_tiles(ext, kind, shape, seed):
    M, N = shape
    K = gr.MIN_K[kind]
    r = rng_of(kind, K)
    R, Q = ext.gemm_check_expected(kind, M, N, K, seed, r)
    wantR, wantQ = port_sums(kind, M, N, K, seed, r)
    what = f"{kind} {M}x{N}x{K} seed {seed:#x}"
    assert_sums_equal(R, wantR, "R", what)
    assert_sums_equal(Q, wantQ, "Q", what)


@pytest.mark.parametrize("shape", [(256, 2304), (2304, 256)], ids=["256x2304", "2304x256"])
@pytest.mark.parametrize("kind", ["bf16", "fp8"])
def test_expected_sums_with_a_partial_last_lane_trip(ext, kind, shape):
    M, N = shape
    K = 200  # 3 * 64 + 8: lanes 8..63 sit out the last trip
    r = rng_of(kind, K)
    R, Q = ext.gemm_check_expected(kind, M, N, K, SEED, r)
    wantR, wantQ = port_sums(kind, M, N, K, SEED, r)
    assert_sums_equal(R, wantR, "R", f"{kind} {M}x{N}x{K}")
    assert_sums_equal(Q, wantQ, "Q", f"{kind} {M}x{N}x{K}")


@ATOMIC
@pytest.mark.parametrize("shape", [(256, 2304), (2304, 256)], ids=["256x2304", "2304x256"])
@pytest.mark.parametrize("kind", KINDS)
def test_ninth_tile_verifies_clean_and_reports(ext, kind, shape, atomic):
    from gpu_docker_api_amd.ops.hipcore import gemm_check_fold

    M, N = shape
    p = problem(ext, kind, M, N, gr.MIN_K[kind])
    ref = p["n"].astype(np.float64) / p["inv"]
    import torch

    kr.assert_exact(p["C"], torch.from_numpy(ref))
    raw = verify(ext, p, p["C"], atomic)
    assert raw["errors"] == CLEAN and raw["records"] == []
    ti, tj = (0, 8) if N > M else (8, 0)
    r, c, d = 150, 77, -1
    row, col = ti * 256 + r, tj * 256 + c
    C = store_granules(p, [row], [col], [int(p["n"][row, col]) + d])
    raw = verify(ext, p, C, atomic)
    assert raw["errors"] == {"rows": 1, "cols": 1, "malformed": 0}
    assert lines(raw, "row") == {(ti, tj, r): (int(p["R"][ti, tj, r]) + d, int(p["R"][ti, tj, r]))}
    assert lines(raw, "col") == {(ti, tj, c): (int(p["Q"][ti, tj, c]) + d, int(p["Q"][ti, tj, c]))}
    assert_matches_port(p, C, raw)
    (tile,) = gemm_check_fold(raw, N // 256, (M // 256) * (N // 256), False)["bad_tiles"]
    assert tile["tile"] == [ti, tj]
    assert tile["element"] == {"row": row, "col": col, "delta": d}


# ---------------------------------------------------------------------------
# 6, 7. fill and operand check, beyond one grid trip too
# ---------------------------------------------------------------------------

TWO_TRIP = (4608, 2048)  # bf16: 1,179,648 vectors; one trip of the grid is 1,048,576
TRIP_VECS = 4096 * 256
_two_trip = {}


def two_trip_port(operand):
    """The port's stored bf16 operand of TWO_TRIP, computed once."""
    if operand not in _two_trip:
        rows, K = TWO_TRIP
        r = rng_of("bf16", K)
        _two_trip[operand] = (gr.codes("bf16", operand, rows, K, SEED, r), r)
    return _two_trip[operand]


@pytest.mark.parametrize("operand", [0, 1], ids=["A", "Bt"])
def test_fill_beyond_one_grid_trip_equals_the_port(ext, operand):
    rows, K = TWO_TRIP
    assert rows * K // 8 == 1179648 > TRIP_VECS
    c, r = two_trip_port(operand)
    want = gr.stored("bf16", c)
    got = to_numpy("bf16", ext.gemm_check_fill("bf16", operand, rows, K, SEED, r))
    assert got.shape == want.shape and got.dtype == want.dtype
    tail = (rows * K // 8 - TRIP_VECS) * 8  # the elements of the second trip
    assert tail == 131072 * 8
    assert np.array_equal(got.ravel()[-tail:], want.ravel()[-tail:]), "second trip"
    assert np.array_equal(got, want)


def upload(kind, s):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(s)).cuda()
    return t.view(torch.bfloat16) if kind == "bf16" else t


def with_other_codes(kind, c, flat, r):
    """The codes [rows][K] with legal other codes at the flat element indices."""
    out = c.copy().ravel()
    for i in flat:
        out[i] = gr.legal_other_code(kind, int(out[i]), r)
    return out.reshape(c.shape)


OPERAND_K = 512
PER_WORD = {"bf16": 2, "fp8": 4, "fp4": 8}


@pytest.mark.parametrize("operand", [0, 1], ids=["A", "Bt"])
@pytest.mark.parametrize("kind", KINDS)
def test_operand_check_counts_every_element_that_differs(ext, kind, operand):
    rows, K = 256, max(gr.MIN_K[kind], OPERAND_K)
    r = rng_of(kind, K)
    c = gr.codes(kind, operand, rows, K, SEED, r)
    clean = gr.stored(kind, c)
    fill = ext.gemm_check_fill(kind, operand, rows, K, SEED, r)
    assert ext.gemm_check_operand(kind, operand, fill, K, SEED, r) == 0
    assert ext.gemm_check_operand(kind, operand, upload(kind, clean), K, SEED, r) == 0
    # against the other operand's generator, or another seed's, it counts
    # what the port counts: most of the operand
    for other_op, other_seed in ((1 - operand, SEED), (operand, SEED ^ 1)):
        want = gr.operand_diff_count(
            kind, clean, gr.stored(kind, gr.codes(kind, other_op, rows, K, other_seed, r)))
        assert want > rows * K // 2
        got = ext.gemm_check_operand(kind, other_op, fill, K, other_seed, r)
        assert got == want, f"{kind} operand {operand} against operand {other_op}, seed " \
                            f"{other_seed:#x}: counted {got} of {want}"

    pw = PER_WORD[kind]
    pv = 4 * pw  # elements of a 16-byte vector
    nvec = rows * K // pv
    assert nvec % 256 == 0 and nvec // 256 <= 4096  # one trip: vector v is thread v
    v0 = 5 * 256 + 2 * 64 + 37  # workgroup 5, wave 2, lane 37
    wave0 = 3 * 256 + 1 * 64  # workgroup 3, wave 1
    cases = {"first element": [0], "last element": [rows * K - 1]}
    for w in range(4):
        cases[f"word {w} of a vector"] = [v0 * pv + w * pw + (w % pw)]
    for j in range(pw):
        cases[f"slot {j} of a word"] = [v0 * pv + 2 * pw + j]
    cases["a whole vector"] = list(range(v0 * pv, v0 * pv + pv))
    cases["every lane of one wave"] = [(wave0 + lane) * pv + (7 * lane + 3) % pv
                                       for lane in range(64)]
    cases["lane 63 of each wave of a workgroup"] = [(9 * 256 + 64 * w + 63) * pv + (5 * w + 1) % pv
                                                    for w in range(4)]
    if kind == "fp4":
        cases["both nibbles of one byte"] = [v0 * pv + 10, v0 * pv + 11]
    for name, flat in cases.items():
        bad = gr.stored(kind, with_other_codes(kind, c, flat, r))
        want = gr.operand_diff_count(kind, clean, bad)
        assert want == len(flat), name
        got = ext.gemm_check_operand(kind, operand, upload(kind, bad), K, SEED, r)
        assert got == want, f"{kind} operand {operand}, {name}: counted {got} of {want}"
    assert len(cases["a whole vector"]) == {"bf16": 8, "fp8": 16, "fp4": 32}[kind]


@pytest.mark.parametrize("operand", [0, 1], ids=["A", "Bt"])
def test_operand_check_beyond_one_grid_trip(ext, operand):
    rows, K = TWO_TRIP
    c, r = two_trip_port(operand)
    clean = gr.stored("bf16", c)
    assert ext.gemm_check_operand("bf16", operand, upload("bf16", clean), K, SEED, r) == 0
    for name, flat in (("the last vector", [rows * K - 3]),
                       ("the first vector of the second trip", [TRIP_VECS * 8 + 1])):
        bad = gr.stored("bf16", with_other_codes("bf16", c, flat, r))
        assert gr.operand_diff_count("bf16", clean, bad) == 1
        got = ext.gemm_check_operand("bf16", operand, upload("bf16", bad), K, SEED, r)
        assert got == 1, f"operand {operand}, {name}: counted {got} of 1"


def test_operand_check_rejects_bad_arguments(ext):
    import torch

    K = 512
    ok = {kind: ext.gemm_check_fill(kind, 0, 256, K, SEED, rng_of(kind, K)) for kind in KINDS}
    r = {kind: rng_of(kind, K) for kind in KINDS}
    bf, f8, f4 = ok["bf16"], ok["fp8"], ok["fp4"]
    assert f4.shape == (256, K // 2)
    flat = torch.zeros(256 * K + 16, dtype=torch.uint8, device="cuda")
    off = flat[8:8 + 256 * K].view(256, K)  # contiguous, 8 bytes off a 16-byte boundary
    assert off.is_contiguous() and off.data_ptr() % 16 == 8
    bad = [
        ("bf16", 0, bf.view(torch.int16), K, r["bf16"]),       # wrong dtype
        ("bf16", 0, bf.float(), K, r["bf16"]),
        ("fp8", 0, f8.view(torch.int8), K, r["fp8"]),
        ("fp8", 0, bf, K, r["fp8"]),
        ("fp8", 0, f8, K // 2, r["fp8"]),                      # wrong width
        ("fp8", 0, f8, 2 * K, r["fp8"]),
        ("fp4", 0, f8, K, r["fp4"]),                           # fp4 rows hold K/2 bytes
        ("bf16", 0, bf[:, :K // 2], K // 2, r["bf16"]),        # not contiguous
        ("fp8", 0, f8.t(), 256, r["fp8"]),
        ("fp8", 0, f8.view(-1), K, r["fp8"]),                  # not 2-D
        ("fp8", 0, off, K, r["fp8"]),                          # misaligned
        ("fp8", 0, f8.cpu(), K, r["fp8"]),                     # not on the GPU
        ("fp8", 2, f8, K, r["fp8"]),                           # operand 2
        ("fp8", -1, f8, K, r["fp8"]),
        ("bf16", 0, bf, K, 0),                                 # no range
        ("fp8", 0, torch.zeros(256, 4736, dtype=torch.uint8, device="cuda"), 4736, 3),  # inexact
        ("fp4", 0, f4, K, 8),
        ("fp16", 0, bf, K, 1),                                 # unknown kind
    ]
    for kind, operand, t, k, rng in bad:
        with pytest.raises(RuntimeError):
            ext.gemm_check_operand(kind, operand, t, k, SEED, rng)
    for kind in KINDS:  # and the same tensors are taken as they are
        assert ext.gemm_check_operand(kind, 0, ok[kind], K, SEED, r[kind]) == 0
    assert torch.cuda.current_device() == 0


# ---------------------------------------------------------------------------
# 8. a flipped operand word: GEMM, verifier, fold and operand check agree
# ---------------------------------------------------------------------------

def replace_element(kind, T, row, k, code):
    """A clone of the stored operand T with element (row, k) set to `code`."""
    import torch

    out = T.clone()
    if kind == "bf16":
        out.view(torch.int16)[row, k] = int(np.array([code], dtype=np.uint16).view(np.int16)[0])
    elif kind == "fp8":
        out[row, k] = code
    else:
        old = int(out[row, k // 2])
        out[row, k // 2] = (old & 0xF0) | code if k % 2 == 0 else (old & 0x0F) | (code << 4)
    return out


@ATOMIC
@pytest.mark.parametrize("operand", [0, 1], ids=["A", "Bt"])
@pytest.mark.parametrize("kind", KINDS)
def test_a_flipped_operand_word_is_a_band(ext, kind, operand, atomic):
    import torch
    from gpu_docker_api_amd.ops.hipcore import gemm_check_fold

    p = base(ext, kind)
    K, r = p["K"], p["range"]
    own, other = (p["a"], p["b"]) if operand == 0 else (p["b"], p["a"])
    line = 300 if operand == 0 else 700  # row of A in tile row 1, row of Bt in tile column 2
    # the other operand's tile sums at k must all be non-zero, or a tile of
    # the band keeps its sum
    S = other.reshape(other.shape[0] // 256, 256, K).sum(axis=1)
    k = int(np.flatnonzero(np.all(S != 0, axis=0))[5])
    c = gr.codes(kind, operand, own.shape[0], K, SEED, r)
    new = gr.legal_other_code(kind, int(c[line, k]), r)
    code_t = np.uint16 if kind == "bf16" else np.uint8
    m = float(gr.decode(kind, np.array([new], dtype=code_t))[0]) / gr.GRANULE[kind]
    assert m == int(m) and int(m) != int(own[line, k])
    own2 = own.copy()
    own2[line, k] = int(m)
    stored_name = "A" if operand == 0 else "Bt"
    T2 = replace_element(kind, p[stored_name], line, k, new)
    A2, Bt2 = (T2, p["Bt"]) if operand == 0 else (p["A"], T2)
    a2, b2 = (own2, p["b"]) if operand == 0 else (p["a"], own2)

    # the kernel is honest: it computes the product of what is stored
    C = run_gemm(ext, kind, A2, Bt2, K)
    kr.assert_exact(C, torch.from_numpy(int_product(a2, b2).astype(np.float64) / p["inv"]))

    # the verifier, against the uncorrupted generator, blames one line
    raw = verify(ext, p, C, atomic)
    assert raw["errors"]["malformed"] == 0
    assert_matches_port(p, C, raw)
    hit = np.flatnonzero(other[:, k] != 0)  # the lines of the other operand it reaches
    if operand == 0:
        want_rows = {(line // 256, j, line % 256) for j in range(3)}
        want_cols = {(line // 256, int(x) // 256, int(x) % 256) for x in hit}
    else:
        want_cols = {(i, line // 256, line % 256) for i in range(2)}
        want_rows = {(int(x) // 256, line // 256, int(x) % 256) for x in hit}
    assert set(lines(raw, "row")) == want_rows
    assert set(lines(raw, "col")) == want_cols
    folded = gemm_check_fold(raw, TILES_N, NWG, False)
    assert folded["records_truncated"] is False
    assert folded["bands"] == [{"iter": 0, "axis": "row" if operand == 0 else "col",
                                "index": line // 256, "tiles": 3 if operand == 0 else 2}]

    # and the operand check says whose fault it is
    assert ext.gemm_check_operand(kind, 0, A2, K, SEED, r) == (1 if operand == 0 else 0)
    assert ext.gemm_check_operand(kind, 1, Bt2, K, SEED, r) == (1 if operand == 1 else 0)
    want = gr.operand_diff_count(kind, to_numpy(kind, p[stored_name]), to_numpy(kind, T2))
    assert want == 1
