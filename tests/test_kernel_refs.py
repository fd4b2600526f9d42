"""CPU tests of tests/kernel_refs.py: the generators really satisfy the
exactness condition, the LUTs match the formats, and the comparators catch
(and locate) the corruptions a broken kernel would produce."""
import numpy as np
import pytest
import torch

import kernel_refs as kr


import test_gpu_kernels as tgk

# largest K each exact set is used with, read off the GPU test matrix itself
USED_K = {
    "bf16": max(s[2] for s in tgk.SHAPES_8PH + tgk.SHAPES_128 + tgk.SHAPES_MFMA["bf16"]),
    "f32": max(s[2] for s in tgk.SHAPES_MFMA["f32"]),
    "e4m3": max(s[2] for s in tgk.SHAPES_FP8),
    "e2m1": max(s[2] for s in tgk.SHAPES_FP4),
}


@pytest.mark.parametrize("kind", sorted(kr.EXACT_SETS))
def test_exact_sets_satisfy_condition(kind):
    s = kr.EXACT_SETS[kind]
    assert USED_K[kind] <= s["k_max"]
    for K in (USED_K[kind], s["k_max"]):
        lhs = kr.exact_condition(s["max"], s["max"], K, s["granule"], s["granule"])
        assert lhs <= kr.TWO24, (kind, K, lhs)
        kr.require_exact(kind, K)
    # the stated limits are tight for the sets whose limit matters
    if kind in ("bf16", "f32", "e4m3"):
        over = kr.exact_condition(s["max"], s["max"], s["k_max"] + 1,
                                  s["granule"], s["granule"])
        assert over > kr.TWO24
        with pytest.raises(AssertionError):
            kr.require_exact(kind, s["k_max"] + 1)


def _generated(kind, rows, K, seed):
    if kind == "bf16":
        return kr.exact_bf16(rows, K, seed)[1]
    if kind == "f32":
        return kr.exact_f32(rows, K, seed)[1]
    if kind == "e4m3":
        return kr.exact_e4m3(rows, K, seed)[1]
    return kr.all_e2m1(rows, K, seed)[1]


@pytest.mark.parametrize("kind", sorted(kr.EXACT_SETS))
def test_generated_values_stay_inside_their_set(kind):
    s = kr.EXACT_SETS[kind]
    v = _generated(kind, 64, 512, seed=3)
    assert float(v.abs().max()) == s["max"]  # the extreme value does occur
    q = v / s["granule"]
    assert torch.equal(q, q.round()), "values are not multiples of the granule"


@pytest.mark.parametrize("kind", sorted(kr.EXACT_SETS))
def test_three_summation_orders_are_bit_identical(kind):
    K = kr.EXACT_SETS[kind]["k_max"]
    K -= K % 32
    a = _generated(kind, 24, K, seed=11)
    b = _generated(kind, 40, K, seed=12)
    ref = kr.reference(a, b)
    prod = (a.float()[:, None, :] * b.float()[None, :, :])  # exact products
    assert torch.equal(prod.double(), a[:, None, :] * b[None, :, :])

    def seq_sum(p):  # strictly sequential fp32 accumulation along k
        acc = torch.zeros(p.shape[:2], dtype=torch.float32)
        for k in range(p.shape[2]):
            acc = acc + p[:, :, k]
        return acc

    fwd = seq_sum(prod)
    rev = seq_sum(prod.flip(2))
    blocks = prod.view(24, 40, K // 32, 32)
    part = torch.zeros(24, 40, K // 32, dtype=torch.float32)
    for j in range(32):
        part = part + blocks[:, :, :, j]
    blk = seq_sum(part)
    for got in (fwd, rev, blk):
        assert got.dtype == torch.float32
        assert torch.equal(got.view(torch.int32), fwd.view(torch.int32))
        assert torch.equal(got.double(), ref)
        kr.assert_exact(got, ref)


def test_e4m3_lut_matches_torch_for_all_finite_codes():
    codes = torch.from_numpy(kr.E4M3_FINITE_CODES.copy())
    assert codes.numel() == 254
    via_torch = codes.view(torch.float8_e4m3fn).float().double()
    lut = torch.from_numpy(kr.E4M3_LUT[kr.E4M3_FINITE_CODES])
    assert torch.equal(via_torch, lut)
    # signed zeros keep their sign
    assert np.signbit(kr.E4M3_LUT[0x80]) and not np.signbit(kr.E4M3_LUT[0x00])
    assert kr.E4M3_LUT[0x7E] == 448.0 and kr.E4M3_LUT[0xFE] == -448.0
    assert kr.E4M3_LUT[0x01] == 2.0 ** -9  # smallest subnormal
    assert np.isnan(kr.E4M3_LUT[0x7F]) and np.isnan(kr.E4M3_LUT[0xFF])


def test_e2m1_lut_matches_existing_fp4_table():
    # the table in tests/test_gpu.py::test_gemm_fp4_mx_numerics_and_throughput
    table = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0,
             -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0]
    assert kr.E2M1_LUT.tolist() == table
    assert np.signbit(kr.E2M1_LUT[8])


def test_full_range_generator_emits_every_finite_code_and_no_nan():
    raw, v = kr.full_range_e4m3(256, 512, seed=5)
    assert raw.dtype == torch.uint8
    counts = np.bincount(raw.numpy().ravel(), minlength=256)
    assert counts[0x7F] == 0 and counts[0xFF] == 0
    finite = counts[kr.E4M3_FINITE_CODES]
    assert finite.min() > 0
    assert finite.max() - finite.min() <= 1  # equal frequency
    assert not bool(torch.isnan(v).any())
    assert float(v.max()) == 448.0 and float(v.min()) == -448.0
    assert torch.equal(v, torch.from_numpy(kr.E4M3_LUT[raw.numpy()]))


def test_exact_e4m3_generator_uses_only_its_codes():
    raw, v = kr.exact_e4m3(128, 256, seed=6)
    used = set(np.unique(raw.numpy()).tolist())
    assert used == set(kr.E4M3_EXACT_CODES.tolist())
    assert len(used) == 1 + 2 * 4 * 8


def test_fp4_packing_low_nibble_is_even_k():
    nib = np.array([[1, 2, 3, 4], [15, 0, 7, 8]], dtype=np.uint8)
    assert kr.pack_e2m1(nib).tolist() == [[0x21, 0x43], [0x0F, 0x87]]
    packed, v = kr.all_e2m1(16, 64, seed=7)
    assert packed.shape == (16, 32) and v.shape == (16, 64)
    lo = packed.numpy() & 0xF
    hi = packed.numpy() >> 4
    assert np.array_equal(kr.E2M1_LUT[lo], v.numpy()[:, 0::2])
    assert np.array_equal(kr.E2M1_LUT[hi], v.numpy()[:, 1::2])
    assert set(np.unique(np.concatenate([lo.ravel(), hi.ravel()]))) == set(range(16))


# ---------------------------------------------------------------------------
# comparator self-checks: a corrupted C must be rejected, with coordinates
# ---------------------------------------------------------------------------

# K=16 keeps the derived bound (at most 16 * 2^-23 * 16 * (127/16)^2 ~ 0.0019)
# below one product granule of the bf16 set (2^-8 ~ 0.0039), so the bound
# comparator can see a one-granule error as well as the exact one.
M, N, K = 512, 768, 16
assert K * 2.0 ** -23 * K * (127.0 / 16.0) ** 2 < 2.0 ** -8


@pytest.fixture(scope="module")
def problem():
    a_raw, a = kr.exact_bf16(M, K, seed=21)
    b_raw, b = kr.exact_bf16(N, K, seed=22)
    ref = kr.reference(a, b)
    good = ref.float()
    return a, b, ref, good


def _both(C, problem):
    """Run both comparators; return the two KernelMismatch (or None)."""
    a, b, ref, _ = problem
    out = []
    for fn in (lambda: kr.assert_exact(C, ref),
               lambda: kr.assert_within_sum_bound(C, ref, a.abs(), b.abs(), K)):
        try:
            fn()
            out.append(None)
        except kr.KernelMismatch as e:
            out.append(e)
    return out


def test_comparators_accept_the_correct_result(problem):
    assert _both(problem[3].clone(), problem) == [None, None]
    a, b, ref, good = problem
    assert kr.assert_within_sum_bound(good, ref, a.abs(), b.abs(), K) == 0.0


def test_one_element_off_by_one_granule_is_caught(problem):
    C = problem[3].clone()
    r, c = 300, 517  # tile (1,2), quadrant (0,0), wave (0,0), frag (2,0)
    C[r, c] += 1.0 / 256.0  # one granule of a bf16 x bf16 product here
    for e in _both(C, problem):
        assert e is not None
        assert e.n_bad == 1 and e.first == (r, c)
        assert e.where["tile"] == (1, 2)
        assert e.where["quadrant"] == (0, 0)
        assert e.where["wave"] == (0, 0)
        assert e.where["fragment"] == (2, 0)
        assert e.where["in_fragment"] == (12, 5)
        assert not e.all_nan
        assert "row 300, col 517" in str(e)


def test_one_transposed_fragment_is_caught(problem):
    C = problem[3].clone()
    r0, c0 = 256 + 128 + 64 + 16, 256 + 128 + 32 + 16
    C[r0:r0 + 16, c0:c0 + 16] = problem[3][r0:r0 + 16, c0:c0 + 16].T
    for e in _both(C, problem):
        assert e is not None
        assert e.where["tile"] == (1, 1)
        assert e.where["quadrant"] == (1, 1)
        assert e.where["wave"] == (1, 1)
        assert e.where["fragment"] == (1, 1)
        # everything bad lies inside that one fragment, off its diagonal
        assert r0 <= e.bad_rows[0] and e.bad_rows[1] < r0 + 16
        assert c0 <= e.bad_cols[0] and e.bad_cols[1] < c0 + 16
        assert 16 * 15 // 2 < e.n_bad <= 16 * 15
        assert not e.all_nan


def test_one_unwritten_tile_is_caught(problem):
    C = problem[3].clone()
    C[256:512, 512:768] = float("nan")
    for e in _both(C, problem):
        assert e is not None
        assert e.n_bad == 256 * 256
        assert e.first == (256, 512)
        assert e.where["tile"] == (1, 2)
        assert e.where["quadrant"] == (0, 0)
        assert e.bad_rows == (256, 511) and e.bad_cols == (512, 767)
        assert e.all_nan
        assert "never written" in str(e)


def test_assert_exact_rejects_a_lossy_reference():
    ref = torch.tensor([[1.0 + 2.0 ** -30]], dtype=torch.float64)
    with pytest.raises(AssertionError, match="exactly representable"):
        kr.assert_exact(ref.float(), ref)


def test_sum_bound_is_the_stated_formula_and_tight_enough():
    a = torch.tensor([[1.0, -2.0]], dtype=torch.float64)
    b = torch.tensor([[3.0, 4.0]], dtype=torch.float64)
    bound = kr.sum_bound(a.abs(), b.abs(), 2)
    assert bound.item() == 2 * 2.0 ** -23 * 11.0
    ref = kr.reference(a, b)
    ok = (ref + 0.9 * bound).float()
    kr.assert_within_sum_bound(ok, ref, a.abs(), b.abs(), 2)
    with pytest.raises(kr.KernelMismatch):
        kr.assert_within_sum_bound((ref + 1.5 * bound).float(), ref, a.abs(),
                                   b.abs(), 2)


def test_real_valued_fp32_accumulation_respects_the_bound():
    """A genuine fp32 accumulation of bf16 products (sequential, the worst
    order) stays inside the derived bound, far from its edge."""
    Kr = 512
    a_raw, a = kr.real_bf16(64, Kr, seed=31)
    b_raw, b = kr.real_bf16(48, Kr, seed=32)
    ref = kr.reference(a, b)
    acc = torch.zeros(64, 48, dtype=torch.float32)
    af, bf = a_raw.float(), b_raw.float()
    for k in range(Kr):
        acc = acc + af[:, k:k + 1] * bf[:, k:k + 1].T
    worst = kr.assert_within_sum_bound(acc, ref, a.abs(), b.abs(), Kr)
    assert worst < 1.0


def test_poisoned_out_detects_missing_and_stray_writes():
    p = kr.PoisonedOut(6, "cpu", shape=(2, 3))
    assert p.out.shape == (2, 3) and bool(torch.isnan(p.out).all())
    assert p.guard_intact()
    with pytest.raises(AssertionError, match="never written"):
        p.check("partial")
    p.out.fill_(1.0)
    p.check("full")
    p.buf[6] = 0.0  # first guard element
    assert not p.guard_intact()
    with pytest.raises(AssertionError, match="guard"):
        p.check("overrun")
    p.poison()
    assert p.guard_intact() and bool(torch.isnan(p.out).all())


# ---------------------------------------------------------------------------
# the MX fp8 product-truncation model and the term it adds to the bound
# ---------------------------------------------------------------------------

def _code(v):
    return int(np.flatnonzero((kr.E4M3_LUT == v) & (np.signbit(kr.E4M3_LUT) == np.signbit(v)))[0])


def test_mx_truncation_model_reproduces_the_measured_two_term_facts():
    """The hardware table in docs/testing.md: next to 448*448 (exponent sum
    16) a product below 2^3 vanishes and one of 2^3 survives; next to 448*1
    (exponent sum 8) the cut is 2^-5; 127 small partners lose exactly the 7
    that share the big product's group."""
    K = 128
    b = np.full((2, K), _code(1.0), dtype=np.uint8)
    b[0, 0] = _code(448.0)           # row 0: big product 448*448
    for small, kept in ((4.0, False), (8.0, True)):
        a = np.zeros((1, K), dtype=np.uint8)
        a[0, 0], a[0, 1] = _code(448.0), _code(small)
        got = kr.mx_fp8_truncated_reference(torch.from_numpy(a), torch.from_numpy(b))
        assert got[0, 0].item() == 200704.0 + (small if kept else 0.0)
    for small, kept in ((2.0 ** -6, False), (2.0 ** -5, True)):
        a = np.zeros((1, K), dtype=np.uint8)
        a[0, 0], a[0, 1] = _code(448.0), _code(small)
        got = kr.mx_fp8_truncated_reference(torch.from_numpy(a), torch.from_numpy(b))
        assert got[0, 1].item() == 448.0 + (small if kept else 0.0)
    a = np.full((1, K), _code(2.0 ** -9), dtype=np.uint8)
    a[0, 0] = _code(448.0)
    got = kr.mx_fp8_truncated_reference(torch.from_numpy(a), torch.from_numpy(b))
    assert got[0, 0].item() == 200704.0 + 120 * 2.0 ** -9


def test_mx_truncation_term_bounds_the_model_and_exact_set_is_untouched():
    ra, a = kr.full_range_e4m3(64, 256, seed=41)
    rb, b = kr.full_range_e4m3(96, 256, seed=42)
    ref = kr.reference(a, b)
    model = kr.mx_fp8_truncated_reference(ra, rb)
    S = a.abs() @ b.abs().T
    assert bool(((model - ref).abs() <= kr.MX_FP8_TRUNCATION * S).all())
    assert float((model - ref).abs().max()) > 0  # the truncation is real here
    # the scaled bound accepts the model output; whether the plain bound
    # does depends on the data, so only the scaled one is asserted
    kr.assert_within_sum_bound(model.float(), ref, a.abs(), b.abs(), 256,
                               extra_factor=kr.MX_FP8_TRUNCATION)
    # the exact e4m3 set never reaches the cut: model == reference
    ea, a = kr.exact_e4m3(64, 256, seed=43)
    eb, b = kr.exact_e4m3(96, 256, seed=44)
    assert torch.equal(kr.mx_fp8_truncated_reference(ea, eb), kr.reference(a, b))


# ---------------------------------------------------------------------------
# workgroup -> tile map (tile_coord in csrc/gemm_8phase_common.h)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("xcd_remap", [False, True])
def test_block_to_tile_map_is_a_bijection_for_every_grid_size(xcd_remap):
    """Every nwg in 1..2048: the blocks cover tiles 0..nwg-1 exactly once
    (tiles_n = 1 makes the tile row the linear tile index), and owner_block
    inverts block_tile."""
    for nwg in range(1, 2049):
        tiles = [kr.block_tile(b, 1, nwg, xcd_remap)[0] for b in range(nwg)]
        assert sorted(tiles) == list(range(nwg)), (nwg, xcd_remap)
        if nwg in (1, 7, 8, 9, 16, 306, 2047, 2048):
            for b, t in enumerate(tiles):
                assert kr.owner_block(t, 0, 1, nwg, xcd_remap) == (b, b % 8)


def test_owner_block_spot_values():
    # without the remap a block computes the tile of its own index
    assert kr.owner_block(2, 1, 3, 9, False) == (7, 7)
    assert kr.owner_block(16, 17, 18, 306, False) == (305, 1)
    # nwg = 9 (q = 1, r = 1): XCD 0 gets tiles 0, 1; XCD x > 0 gets tile x + 1
    assert [kr.block_tile(b, 3, 9, True) for b in range(9)] == [
        (0, 0), (0, 2), (1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2), (0, 1)]
    assert kr.owner_block(0, 1, 3, 9, True) == (8, 0)
    assert kr.owner_block(2, 2, 3, 9, True) == (7, 7)
    # nwg = 16 (q = 2, r = 0): XCD x gets tiles 2x, 2x + 1
    assert kr.owner_block(0, 1, 4, 16, True) == (8, 0)
    assert kr.owner_block(3, 3, 4, 16, True) == (15, 7)
    assert kr.owner_block(1, 2, 4, 16, True) == (3, 3)
    # nwg = 306 (q = 38, r = 2): XCDs 0, 1 get 39 tiles, the others 38
    assert kr.owner_block(0, 0, 18, 306, True) == (0, 0)
    assert kr.owner_block(2, 2, 18, 306, True) == (38 * 8, 0)      # tile 38, last of XCD 0
    assert kr.owner_block(2, 3, 18, 306, True) == (1, 1)           # tile 39, first of XCD 1
    assert kr.owner_block(4, 5, 18, 306, True) == (38 * 8 + 1, 1)  # tile 77, last of XCD 1
    assert kr.owner_block(4, 6, 18, 306, True) == (2, 2)           # tile 78, first of XCD 2
    assert kr.owner_block(16, 17, 18, 306, True) == (37 * 8 + 7, 7)  # the last tile
    # blocks 304, 305 are the 39th of XCDs 0 and 1; no block beyond them
    assert kr.block_tile(305, 18, 306, True) == (4, 5)
    with pytest.raises(AssertionError):
        kr.owner_block(17, 0, 18, 306, True)


def test_mismatch_message_names_the_owning_block(problem):
    a, b, ref, good = problem  # 512 x 768: 2 x 3 tiles, nwg = 6
    C = good.clone()
    C[300, 517] += 1.0 / 256.0  # tile (1, 2) = tile 5
    C[10, 300] += 1.0 / 256.0   # tile (0, 1) = tile 1
    with pytest.raises(kr.KernelMismatch) as ei:
        kr.assert_exact(C, ref)
    e = ei.value
    assert e.bad_tiles == [(0, 1), (1, 2)]
    text = kr.describe_owners(e, 3, 6, True)
    assert "blockIdx.x 1 of 6 (blockIdx % 8 = 1, xcd_remap=1)" in text
    assert "2 bad tiles, their blockIdx % 8 in [1, 5]" in text


# ---------------------------------------------------------------------------
# the full-machine shapes and their exactness
# ---------------------------------------------------------------------------

def test_full_machine_shapes_and_k():
    import test_gpu_kernels_full as full

    s = full.full_shapes(256)
    assert s == {"one-per-cu": (16, 16), "second-round": (17, 18)}
    assert divmod(16 * 16, 8) == (32, 0) and divmod(17 * 18, 8) == (38, 2)
    for cus in (64, 104, 228, 256, 304):
        s = full.full_shapes(cus)
        one, two = s["one-per-cu"], s["second-round"]
        assert one[0] * one[1] == cus
        assert two[0] * two[1] > cus and (two[0] * two[1]) % 8 >= 2
    for kind, K in full.K_FULL.items():
        kr.require_exact(kind, K)
    # 19 kernels x (2 idle shapes + 1 contended), ordered so that the cases
    # of one problem are neighbours (full_problem keeps only the latest)
    assert len(full.CASES) == 19 * 3
    keys = [c[:2] for c in full.CASES]
    assert len({k for k in keys}) == sum(a != b for a, b in zip(keys, keys[1:])) + 1
    # no operand fits one XCD's 4 MiB of L2 next to the other (bytes per row:
    # bf16 2K, fp8 K, fp4 K/2; the smallest is fp4 at exactly 4 MiB)
    assert 4096 * min(1024 * 2, 1152, 2048 // 2) >= 4 << 20


# ---------------------------------------------------------------------------
# numpy ports of the probe fills
# ---------------------------------------------------------------------------

FILL_N = 1 << 20


def test_bf16_rounding_port_matches_torch():
    g = torch.Generator().manual_seed(5)
    v = torch.cat([torch.rand(4096, generator=g) * 2 - 1,
                   torch.tensor([1 - 2.0 ** -9, 1 - 2.0 ** -9 - 2.0 ** -20, 1 - 2.0 ** -8,
                                 0.0, -1.0, 2.0 ** -9 + 2.0 ** -17])])
    want = v.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    bits = kr.f32_to_bf16_bits(v.numpy())
    assert np.array_equal(bits, want)
    assert np.array_equal(kr.bf16_bits_to_f64(bits), v.to(torch.bfloat16).double().numpy())


def test_fill_ports_first_values_by_hand():
    """Element 0 and 1 of each port, worked through the C expressions with
    Python integers."""
    def bf16(i, seed):
        h = (i * 2654435761 + seed) & 0xFFFFFFFF
        h ^= h >> 15
        h = (h * 2246822519) & 0xFFFFFFFF
        h ^= h >> 13
        v = min((h & 0xFFFFFF) / 8388608.0 - 1.0, kr.BF16_BELOW_ONE)
        return int(torch.tensor(v, dtype=torch.float32).to(torch.bfloat16)
                   .view(torch.int16).item()) & 0xFFFF

    def mx(i, seed):
        h = ((i * 2654435761) & 0xFFFFFFFF) ^ seed
        h ^= h >> 13
        h = (h * 0x85EBCA6B) & 0xFFFFFFFF
        return h ^ (h >> 16)

    for seed in kr.PROBE_SEEDS:
        idx = [0, 1, 2, FILL_N // 2, FILL_N - 1]
        assert [int(kr.fill_bf16_hash(FILL_N, seed)[i]) for i in idx] == \
            [bf16(i, seed) for i in idx]
        assert [int(kr.fill_e2m1_hash(FILL_N, seed)[i]) for i in idx] == \
            [mx(i, seed) & 0xFF for i in idx]
        assert [int(kr.fill_e4m3_hash(FILL_N, seed)[i]) for i in idx] == \
            [((mx(i, seed) & 1) << 7) | ((((mx(i, seed) >> 1) & 7) + 4) << 3)
             | ((mx(i, seed) >> 4) & 7) for i in idx]


@pytest.mark.parametrize("kind", sorted(kr.FILL_PORTS))
def test_fill_ports_have_the_properties_the_probes_need(kind):
    a, b = (kr.FILL_PORTS[kind](FILL_N, s) for s in kr.PROBE_SEEDS)
    assert a.dtype == (np.uint16 if kind == "bf16" else np.uint8)
    kr.check_fill_properties(kind, a, b)
    # a prefix of a longer fill is the shorter fill; an empty one is empty
    assert np.array_equal(kr.FILL_PORTS[kind](1000, 7), b[:1000])
    assert kr.FILL_PORTS[kind](0, 7).shape == (0,)


def test_bf16_fill_is_held_below_one():
    """Finding behind the fminf in fill_bf16_hash_kernel: the hash value lies
    in [-1, 1) as a float, but one in 1024 of them is at least 1 - 2^-9 and
    rounds to bf16 1.0. The clamp holds those at 1 - 2^-8."""
    bits = kr.fill_bf16_hash(FILL_N, 1)
    v = kr.bf16_bits_to_f64(bits)
    top = float(np.mean(v == kr.BF16_BELOW_ONE))
    # of the range of width 2: 2^-8 that round to it, 2^-9 that are clamped
    assert abs(top - 1.5 * 2.0 ** -8 / 2) < 2e-4, top
    assert v.max() == kr.BF16_BELOW_ONE and v.min() >= -1.0


@pytest.mark.parametrize("kind", sorted(kr.FILL_PORTS))
def test_fill_property_check_rejects_broken_fills(kind):
    a, b = (kr.FILL_PORTS[kind](FILL_N, s) for s in kr.PROBE_SEEDS)
    with pytest.raises(AssertionError, match="differ in"):
        kr.check_fill_properties(kind, a, a.copy())  # seed ignored
    broken = []
    if kind == "bf16":
        broken = [a & 0x7FFF,                                   # sign stuck
                  np.where(np.arange(FILL_N) == 5, 0x3F80, a).astype(a.dtype),  # a 1.0
                  np.zeros_like(a)]
    elif kind == "e4m3":
        broken = [a & 0x7F, a | 0x80,                           # sign stuck
                  np.where(np.arange(FILL_N) == 5, 0x7F, a).astype(a.dtype),  # a NaN
                  a & 0xF8,                                     # mantissa stuck
                  np.where((a >> 3) & 0xF == 11, a - 8, a).astype(a.dtype),  # exponent 11 lost
                  np.where(np.arange(FILL_N) == 5, 0x18, a).astype(a.dtype)]  # exponent 3
    else:
        broken = [a & 0x7F, a | 0x01, np.zeros_like(a)]
    for bad in broken:
        with pytest.raises(AssertionError):
            kr.check_fill_properties(kind, bad, b)
