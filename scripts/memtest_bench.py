#!/usr/bin/env python3
"""HBM memtest throughput next to the copy kernel, in one process on one
MI355X: the numbers behind profiles/hbm_memtest.md and the floors of
tests/test_memtest_gpu.py.

Per repeat: stream_bandwidth_gbps(0, 1024, 5), then hbm_memtest over
--gib GiB in 1 GiB chunks. Then every kernel alone on one 4 GiB tensor.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SEED = 0x0123456789ABCDEF


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    from gpu_docker_api_amd.ops import hipcore

    ext = hipcore.load_ext()
    out = {"rocm": torch.version.hip, "gib": args.gib, "runs": []}
    for _ in range(args.repeats):
        copy = ext.stream_bandwidth_gbps(0, 1024, 5)
        rep = ext.hbm_memtest(0, [1 << 30] * args.gib, SEED)
        row = {
            "copy_gbps": round(copy, 1),
            "write_gbps": round(rep["write_gbps"], 1),
            "verify_gbps": round(rep["verify_gbps"], 1),
            "seconds": round(rep["seconds"], 4),
            "errors": rep["errors"],
        }
        print(json.dumps(row), flush=True)
        out["runs"].append(row)

    n = (4 << 30) // 8
    t = torch.empty(n, dtype=torch.int64, device="cuda")

    def timed(fn) -> float:
        torch.cuda.synchronize()
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return round(n * 8 / (e0.elapsed_time(e1) * 1e6), 1)

    steps = {}
    for pat in ("addr", "zero", "rand"):
        # the first launch of a kernel loads its code: one untimed call each
        ext.memtest_write(t, pat, SEED)
        ext.memtest_verify(t, pat, SEED)
        steps[f"write {pat}"] = [timed(lambda: ext.memtest_write(t, pat, SEED)) for _ in range(3)]
        steps[f"verify {pat}"] = [timed(lambda: ext.memtest_verify(t, pat, SEED)) for _ in range(3)]
    flips, inv = [], False
    ext.memtest_verify_flip(t, "rand", SEED, 0, inv)
    for _ in range(3):
        inv = not inv
        flips.append(timed(lambda: ext.memtest_verify_flip(t, "rand", SEED, 0, inv)))
    steps["verify_flip rand"] = flips
    for k, v in steps.items():
        print(f"{k}: {v}", flush=True)
    out["steps_4gib"] = steps
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
