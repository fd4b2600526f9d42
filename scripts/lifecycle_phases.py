#!/usr/bin/env python3
"""Where one bench.py cycle spends its time: per-phase p50/p95.

Starts the daemon exactly as bench.py does (same DaemonThread, same config,
same requests), runs N create -> patch -> delete cycles and aggregates

  * the server-side ``phases`` each create/patch response body carries
    (utils/timing.PhaseTimer: schedule, create, start, persist, copy,
    preserve, delete_old, total),
  * the client-side wall time of each request (``request_ms``), so the gap
    between a request and its phase total — HTTP stack, routing, JSON — is
    visible; the delete response carries no phases and is timed as a whole,
  * the whole cycle.

Writes one JSON document (``--out``) and prints it.
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pct(samples, q):
    s = sorted(samples)
    return round(s[min(int(q * len(s)), len(s) - 1)], 3) if s else 0.0


def table(rows):
    """rows: list of {phase: ms} -> {phase: {p50_ms, p95_ms}}"""
    keys = []
    for r in rows:
        for k in r:
            if k not in keys:
                keys.append(k)
    return {
        k: {"p50_ms": pct([r[k] for r in rows if k in r], 0.50),
            "p95_ms": pct([r[k] for r in rows if k in r], 0.95)}
        for k in keys
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cycles", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--port", type=int, default=18741)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import httpx
    import torch

    import bench

    use_gpu = torch.cuda.is_available()
    data_dir = os.path.join("/tmp", f"gda-phases-{args.port}")
    shutil.rmtree(data_dir, ignore_errors=True)
    server = bench.DaemonThread(args.port, 1, use_gpu, data_dir=data_dir, runtime="proc")
    server.start()
    client = httpx.Client(base_url=f"http://127.0.0.1:{args.port}", timeout=120)
    node_gpus = len((client.get("/api/v1/resources/gpus").json().get("data") or {}))
    patch_to = 2 if 2 <= node_gpus else 0

    create_rows, patch_rows, delete_rows, cycle_ms = [], [], [], []
    name = "phase0"
    try:
        for i in range(args.warmup + args.cycles):
            t0 = time.perf_counter()
            c = client.post(
                "/api/v1/replicaSet",
                json={"imageName": "synthetic:bench", "replicaSetName": name,
                      "gpuCount": 1, "cpuCount": 1, "memory": "1GB"},
            ).json()
            t1 = time.perf_counter()
            p = client.patch(
                f"/api/v1/replicaSet/{name}", json={"gpuPatch": {"gpuCount": patch_to}}
            ).json()
            t2 = time.perf_counter()
            d = client.delete(f"/api/v1/replicaSet/{name}").json()
            t3 = time.perf_counter()
            assert c["code"] == 200 and p["code"] == 200 and d["code"] == 200, (c, p, d)
            if i < args.warmup:
                continue
            create_rows.append({**(c["data"].get("phases") or {}), "request_ms": (t1 - t0) * 1e3})
            patch_rows.append({**(p["data"].get("phases") or {}), "request_ms": (t2 - t1) * 1e3})
            delete_rows.append({"request_ms": (t3 - t2) * 1e3})
            cycle_ms.append((t3 - t0) * 1e3)
    finally:
        client.close()
        server.stop()
        shutil.rmtree(data_dir, ignore_errors=True)

    from gpu_docker_api_amd.runtime import proc as proc_rt

    out = {
        "label": args.label,
        "cycles": args.cycles,
        "warmup": args.warmup,
        "gpu": use_gpu,
        "patch_step": f"gpuCount 1->{patch_to}",
        "native_lifecycle": bool(getattr(proc_rt, "NATIVE_LIFECYCLE", False)),
        "cycle": {"p50_ms": pct(cycle_ms, 0.50), "p95_ms": pct(cycle_ms, 0.95)},
        "create": table(create_rows),
        "patch": table(patch_rows),
        "delete": table(delete_rows),
    }
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
