"""bench.py single-rank contract: one JSON line with the driver's schema."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_json_contract():
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "4", "--warmup", "1"],
        capture_output=True,
        text=True,
        timeout=300,
        cwd=ROOT,
    )
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, f"expected exactly one JSON line, got {len(lines)}"
    r = json.loads(lines[0])
    for key in (
        "metric",
        "value",
        "unit",
        "n_gpus",
        "steps",
        "warmup",
        "ms_per_step",
        "higher_is_better",
        "scaling",
        "vs_baseline",
        "dtype",
        "data",
        "config",
    ):
        assert key in r, f"missing {key}"
    assert r["n_gpus"] == 1
    assert r["steps"] == 4 and r["warmup"] == 1
    assert r["higher_is_better"] is False
    assert r["scaling"] == "weak"
    assert r["unit"] == "ms"
    assert r["value"] > 0 and r["ms_per_step"] > 0
    assert "global_batch" in r["config"] and "parallelism" in r["config"]


def test_bench_dump_outputs_and_full(tmp_path):
    """--dump-outputs writes the last timed cycle's results as float .npy
    arrays; --full is accepted and still yields the one result line."""
    import numpy as np

    dump = tmp_path / "out"
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2",
         "--warmup", "1", "--full", "--dump-outputs", str(dump)],
        capture_output=True,
        text=True,
        timeout=300,
        cwd=ROOT,
    )
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r["steps"] == 2 and r["ms_per_step"] > 0

    arrays = {p.stem: np.load(p) for p in dump.glob("*.npy")}
    assert set(arrays) == {"codes", "versions", "names_utf8"}
    for a in arrays.values():
        assert a.dtype in (np.float32, np.float64)
    assert arrays["codes"].tolist() == [200.0, 200.0, 200.0]
    # create returns version 1, the rolling replace version 2
    assert arrays["versions"].tolist() == [1.0, 2.0]
    names = [bytes(int(b) for b in row if b).decode() for row in arrays["names_utf8"]]
    assert names == ["bench0-1", "bench0-2"]
