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
