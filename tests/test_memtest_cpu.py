"""HBM memtest, everything that needs no GPU: the pattern references, the
chunk plan, the validate_gpus wiring, the route field and the CLI flag."""
import http.server
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import memtest_refs as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GIB = 1 << 30


# ---------------------------------------------------------------------------
# pattern references
# ---------------------------------------------------------------------------

def test_golden_table_numpy():
    g = [g for g, _ in mr.GOLDEN_RAND]
    got = mr.pattern_np(g, "rand", mr.SEED)
    assert [int(w) for w in got] == [w for _, w in mr.GOLDEN_RAND]


def test_golden_table_torch():
    import torch

    g = torch.tensor([mr.to_i64(g) for g, _ in mr.GOLDEN_RAND], dtype=torch.int64)
    got = mr.pattern_torch(g, "rand", mr.SEED)
    assert [mr.to_u64(w) for w in got.tolist()] == [w for _, w in mr.GOLDEN_RAND]


def test_addr_zero_and_invert_definitions():
    g = [0, 1, 2**32, 2**63 + 5]
    addr = mr.pattern_np(g, "addr", mr.SEED)
    assert [int(w) for w in addr] == [x ^ mr.SEED for x in g]
    inv = mr.pattern_np(g, "addr", mr.SEED, invert=True)
    assert [int(w) for w in inv] == [(x ^ mr.SEED) ^ mr.M64 for x in g]
    assert not mr.pattern_np(g, "zero").any()
    assert [int(w) for w in mr.pattern_np(g, "zero", invert=True)] == [mr.M64] * 4


@pytest.mark.parametrize("pattern", ["addr", "rand"])
@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize(
    "base",
    [0, 2**32 - 4096, 2**33 - 7, 2**63 - 3],
    ids=["zero", "straddle-2^32", "straddle-2^33", "straddle-sign"],
)
def test_references_agree(pattern, invert, base):
    import torch

    n = (1 << 20) if base == 0 else 8192
    a = mr.pattern_np(mr.arange_np(base, n), pattern, mr.SEED, invert)
    b = mr.expected_torch(base, n, pattern, mr.SEED, invert)
    assert np.array_equal(a, b.numpy().view(np.uint64))
    assert b.dtype == torch.int64


# ---------------------------------------------------------------------------
# word_class: which tile, workgroup, wave, lane, slot and half owns a word
# ---------------------------------------------------------------------------

GEO = mr.GEOMETRY
T = GEO["block"] * GEO["words_per_thread_iter"]
W = T * GEO["max_grid"]


@pytest.mark.parametrize("head", [0, 1])
def test_word_class_is_a_bijection_on_a_tile(head):
    """The 2048 body words of a tile map one to one onto 4 waves x 64 lanes x
    4 slots x 2 halves, for a full first-trip tile, a second-trip tile and
    the tile before the bounds-checked one."""
    n = W + 2 * T + 5
    for tile in (0, 1, GEO["max_grid"], GEO["max_grid"] + 1):
        seen = set()
        for p in range(head + tile * T, head + (tile + 1) * T):
            c = mr.word_class(p, head, n, GEO)
            assert c.tile == tile and c.full
            assert c.workgroup == tile % GEO["max_grid"]
            assert c.trip == tile // GEO["max_grid"]
            seen.add((c.wave, c.lane, c.slot, c.half))
        assert len(seen) == T
        assert seen == {(w, l, s, h) for w in range(4) for l in range(64)
                        for s in range(4) for h in range(2)}
    # one vector is one (wave, lane, slot); consecutive vectors are
    # consecutive lanes: the coalesced 16 B per lane of the header
    a, b, c = (mr.word_class(head + q, head, n, GEO) for q in (0, 1, 2))
    assert a[:6] == b[:6] and (a.half, b.half) == (0, 1)
    assert (c.lane, c.slot, c.half) == (1, 0, 0)


def test_word_class_head_and_tail():
    # n = 0: no position at all
    for head in (0, 1):
        with pytest.raises(ValueError):
            mr.word_class(0, head, 0, GEO)
    # n = 1: the one word is the tail of an aligned view, the head of an odd one
    assert mr.word_class(0, 0, 1, GEO) == "tail"
    assert mr.word_class(0, 1, 1, GEO) == "head"
    # n = 2: one vector, or head and tail with no body between them
    assert [mr.word_class(p, 0, 2, GEO) for p in (0, 1)] == [
        (0, 0, 0, 0, 0, 0, 0, False), (0, 0, 0, 0, 0, 0, 1, False)]
    assert [mr.word_class(p, 1, 2, GEO) for p in (0, 1)] == ["head", "tail"]
    # the views of the GPU tests: a tail exists exactly where n - head is odd
    for head, n, tail in ((0, 3 * T + 5, True), (1, 3 * T + 6, True),
                          (0, 3 * T + 6, False), (1, 3 * T + 5, False)):
        classes = [mr.word_class(p, head, n, GEO) for p in range(n)]
        assert (classes[0] == "head") == bool(head)
        assert (classes[-1] == "tail") == tail
        body = classes[head : n - 1 if tail else n]
        assert "head" not in body and "tail" not in body
        assert len(body) % 2 == 0
    with pytest.raises(ValueError):
        mr.word_class(5, 0, 5, GEO)
    with pytest.raises(ValueError):
        mr.word_class(-1, 0, 5, GEO)
    with pytest.raises(ValueError):
        mr.word_class(0, 2, 5, GEO)


def test_word_class_by_hand():
    assert (T, W) == (2048, 4194304)
    # aligned, n = 6150 (3075 vectors): p = 4097 is .y of vector 2048, the
    # first vector of tile 2; 3 * 1024 <= 3075, so tile 2 is full
    assert mr.word_class(4097, 0, 6150, GEO) == (2, 0, 2, 0, 0, 0, 1, True)
    # odd view, n = 6150: 6149 body-and-tail words, the last is the tail;
    # p = 6148 is body word 6147, .y of vector 3073 = tile 3, thread 1 of
    # slot 0; 3074 vectors < 4 * 1024, so tile 3 is bounds-checked
    assert mr.word_class(6149, 1, 6150, GEO) == "tail"
    assert mr.word_class(6148, 1, 6150, GEO) == (3, 0, 3, 0, 1, 0, 1, False)
    # odd view, n = W + 2T + 5: vector 2048 * 1024 + 3 * 256 + 191 is tile
    # 2048 (workgroup 0 on its second trip), slot 3, thread 191 = wave 2
    # lane 63; its .x is p = 1 + 2 * 2098111
    assert mr.word_class(4196223, 1, W + 2 * T + 5, GEO) == (
        2048, 1, 0, 2, 63, 3, 0, True)


# ---------------------------------------------------------------------------
# memtest_plan
# ---------------------------------------------------------------------------

def test_plan_sum_and_multiple_of_16():
    from gpu_docker_api_amd.ops.hipcore import memtest_plan

    plan = memtest_plan(200 * GIB, 4 * GIB)
    assert plan == [GIB] * 4
    want = 3 * GIB + 1000 * 1000 + 7  # not a multiple of 16
    plan = memtest_plan(200 * GIB, want)
    assert sum(plan) == want // 16 * 16
    assert all(c % 16 == 0 and c > 0 for c in plan)


def test_plan_want_exceeds_free_minus_reserve():
    from gpu_docker_api_amd.ops.hipcore import memtest_plan

    free = 10 * GIB + 24
    plan = memtest_plan(free, 64 * GIB)
    assert sum(plan) == (free - 2 * GIB) // 16 * 16
    plan = memtest_plan(free, 64 * GIB, reserve_bytes=4 * GIB)
    assert sum(plan) == (free - 4 * GIB) // 16 * 16


def test_plan_last_short_chunk():
    from gpu_docker_api_amd.ops.hipcore import memtest_plan

    plan = memtest_plan(200 * GIB, 2 * GIB + 4096 + 8)
    assert plan == [GIB, GIB, 4096]
    plan = memtest_plan(200 * GIB, 3 * GIB, chunk_bytes=2 * GIB)
    assert plan == [2 * GIB, GIB]


def test_plan_empty_below_one_gib():
    from gpu_docker_api_amd.ops.hipcore import memtest_plan

    assert memtest_plan(200 * GIB, GIB - 16) == []
    assert memtest_plan(200 * GIB, GIB) == [GIB]
    assert memtest_plan(3 * GIB - 16, 8 * GIB) == []  # free - reserve < 1 GiB
    assert memtest_plan(GIB, 8 * GIB) == []  # free below the reserve
    assert memtest_plan(3 * GIB, 8 * GIB) == [GIB]


# ---------------------------------------------------------------------------
# validate_gpus with a stub extension
# ---------------------------------------------------------------------------

class StubExt:
    def __init__(self, free=100 * GIB, errors=0):
        self.free = free
        self.errors = errors
        self.memtest_calls = []

    def device_count(self):
        return 1

    def stream_bandwidth_gbps(self, i, mib, iters):
        return 5000.0

    def gemm_bf16_8ph_tflops(self, i, size, iters):
        return 1000.0

    def gemm_fp8_mx_tflops(self, i, size, iters):
        return 1900.0

    def gemm_fp4_mx_tflops(self, i, size, iters):
        return 4000.0

    def device_info(self, i):
        return {"freeMem": self.free, "totalGlobalMem": 288 * 10**9}

    def hbm_memtest(self, device, chunks, seed, max_records, scrub, inject):
        self.memtest_calls.append((device, list(chunks), seed, max_records, scrub, list(inject)))
        return {
            "bytes_tested": sum(chunks),
            "passes": 6,
            "errors": self.errors,
            "bad_bits": 4 if self.errors else 0,
            "records": [],
            "write_gbps": 4000.0,
            "verify_gbps": 4000.0,
            "seconds": 0.1,
        }


@pytest.fixture
def stub(monkeypatch):
    from gpu_docker_api_amd.ops import hipcore

    def install(**kw):
        ext = StubExt(**kw)
        monkeypatch.setattr(hipcore, "_ext", ext)
        return ext

    return install


def test_validate_without_memtest_is_unchanged(stub):
    from gpu_docker_api_amd.ops import hipcore

    ext = stub()
    report = hipcore.validate_gpus(size=2048, iters=3)
    assert report == hipcore.validate_gpus(size=2048, iters=3, memtest_mib=0)
    assert ext.memtest_calls == []
    assert report == {
        "gpus": [
            {
                "index": 0,
                "hbm_gbps": 5000.0,
                "bf16_tflops": 1000.0,
                "fp8_tflops": 1900.0,
                "fp4_tflops": 4000.0,
                "healthy": True,
            }
        ]
    }


def test_validate_memtest_clean_keeps_healthy(stub):
    from gpu_docker_api_amd.ops import hipcore

    ext = stub()
    g = hipcore.validate_gpus(size=2048, iters=3, memtest_mib=2048)["gpus"][0]
    assert g["memtest"]["errors"] == 0 and g["healthy"] is True
    assert len(ext.memtest_calls) == 1
    device, chunks, seed, _, scrub, inject = ext.memtest_calls[0]
    assert device == 0 and chunks == [GIB, GIB] and scrub is False and inject == []
    assert 0 <= seed < 2**64


def test_validate_memtest_errors_mark_unhealthy(stub):
    from gpu_docker_api_amd.ops import hipcore

    stub(errors=3)
    g = hipcore.validate_gpus(size=2048, iters=3, memtest_mib=2048)["gpus"][0]
    assert g["memtest"]["errors"] == 3
    assert g["healthy"] is False


def test_validate_memtest_skipped_leaves_throughput_rule(stub):
    from gpu_docker_api_amd.ops import hipcore

    ext = stub(free=2 * GIB + 4096, errors=3)  # errors never consulted: no run
    g = hipcore.validate_gpus(size=2048, iters=3, memtest_mib=2048)["gpus"][0]
    assert g["memtest"] == {"skipped": "insufficient free HBM"}
    assert ext.memtest_calls == []
    assert g["healthy"] is True


def test_memtest_gpu_forwards_two_element_inject_entries(stub):
    """The binding's optional third inject field and its base_word keyword
    are for the tests: memtest_gpu passes what it always passed."""
    from gpu_docker_api_amd.ops import hipcore

    ext = stub()
    inject = [(12345, 0x8000000000000001), (7, 1)]
    hipcore.memtest_gpu(0, 2048, inject=inject)
    assert len(ext.memtest_calls) == 1  # six positional arguments, no keyword
    assert ext.memtest_calls[0][5] == inject
    assert all(type(e) is tuple and len(e) == 2 for e in ext.memtest_calls[0][5])


# ---------------------------------------------------------------------------
# route
# ---------------------------------------------------------------------------

@pytest.fixture
def client(tmp_path):
    from fastapi.testclient import TestClient

    from gpu_docker_api_amd.routers.app import build_app
    from helpers import make_config

    app = build_app(make_config(tmp_path))
    with TestClient(app) as c:
        yield c


@pytest.fixture
def validate_calls(monkeypatch):
    from gpu_docker_api_amd.ops import hipcore

    calls = []

    async def fake(indices=None, size=4096, iters=5, memtest_mib=0):
        calls.append({"size": size, "iters": iters, "memtest_mib": memtest_mib})
        return {"gpus": []}

    monkeypatch.setattr(hipcore, "validate_gpus_async", fake)
    return calls


URL = "/api/v1/resources/gpus/validate"


def test_route_memtest_non_int_is_invalid_params(client, validate_calls):
    from gpu_docker_api_amd.routers.codes import Code

    bad_size = client.post(URL, json={"size": "x"}).json()["code"]
    assert bad_size == int(Code.INVALID_PARAMS)
    for value in ("x", "2048", 1.5, None, [1], True):
        r = client.post(URL, json={"memtestMiB": value})
        assert r.json()["code"] == bad_size, value
    assert validate_calls == []


def test_route_memtest_clamped_and_default_off(client, validate_calls):
    assert client.post(URL, json={}).json()["code"] == 200
    assert client.post(URL, json={"memtestMiB": 0}).json()["code"] == 200
    assert client.post(URL, json={"memtestMiB": 5}).json()["code"] == 200
    assert client.post(URL, json={"memtestMiB": 4096}).json()["code"] == 200
    assert client.post(URL, json={"memtestMiB": 10**9}).json()["code"] == 200
    assert [c["memtest_mib"] for c in validate_calls] == [0, 0, 1024, 4096, 294912]
    assert all(c["size"] == 4096 and c["iters"] == 5 for c in validate_calls)


# ---------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------

@pytest.fixture
def recording_daemon():
    """A socket that answers every POST with an empty success envelope and
    keeps the JSON bodies it was sent."""
    bodies = []

    class Handler(http.server.BaseHTTPRequestHandler):
        def do_POST(self):
            n = int(self.headers.get("Content-Length", 0))
            bodies.append((self.path, json.loads(self.rfile.read(n) or b"{}")))
            out = json.dumps({"code": 200, "msg": "Success", "data": {"gpus": []}}).encode()
            self.send_response(200)
            self.send_header("Content-Type", "application/json")
            self.send_header("Content-Length", str(len(out)))
            self.end_headers()
            self.wfile.write(out)

        def log_message(self, *a):
            pass

    server = http.server.HTTPServer(("127.0.0.1", 0), Handler)
    t = threading.Thread(target=server.serve_forever, daemon=True)
    t.start()
    yield server.server_address[1], bodies
    server.shutdown()
    server.server_close()
    t.join(timeout=10)


def _cli(port, *args):
    env = dict(os.environ, GDA_ADDR=f"http://127.0.0.1:{port}")
    return subprocess.run(
        [sys.executable, "-m", "gpu_docker_api_amd.cli", *args],
        capture_output=True,
        text=True,
        timeout=60,
        cwd=ROOT,
        env=env,
    )


def test_cli_memtest_flag_only_when_given(recording_daemon):
    port, bodies = recording_daemon
    out = _cli(port, "resources", "validate")
    assert out.returncode == 0, out.stderr
    out = _cli(port, "resources", "validate", "--memtest-mib", "4096", "--size", "2048")
    assert out.returncode == 0, out.stderr
    out = _cli(port, "resources", "validate", "--memtest-mib", "0")
    assert out.returncode == 0, out.stderr
    assert bodies == [
        (URL, {"size": 4096, "iters": 5}),
        (URL, {"size": 2048, "iters": 5, "memtestMiB": 4096}),
        (URL, {"size": 4096, "iters": 5}),
    ]
