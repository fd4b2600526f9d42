#!/usr/bin/env python3
"""Interleaved timing of the checked GEMM loop (csrc/gemm_check.hip).

Per format and size, round-robin in one process (run-to-run noise is a few
percent, so the variants must share a process and alternate):

  unchecked  the GEMM alone, back to back, on the exact operands
  serial     GEMM, verify, GEMM, verify ... on one stream and one C
  serial-atomic, verify-atomic
             as serial and verify, the column sums combined with 64-bit atomics
             instead of the slab
  overlap    C double-buffered, verify on a second stream
  verify     the verify kernels alone on an idle device, one C read again and
             again (the 256 MiB Infinity Cache serves much of it)
  verify-cold  the same, cycling over 768 MiB of results: reads from HBM
  probe      the throughput tier's hash-fill probe (*_tflops), for the
             operand-activity comparison

Prints microseconds per iteration (median, min..max over the rounds) and one
JSON document; `--out` also writes it to a file.

    python scripts/gemm_check_ab.py --sizes 4096 8192 --iters 2000 --rounds 5
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gpu_docker_api_amd.ops import hipcore  # noqa: E402

LOOPS = ("unchecked", "serial", "serial-atomic", "overlap", "verify", "verify-atomic",
         "verify-cold")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 8192])
    ap.add_argument("--formats", nargs="+", default=list(hipcore.GEMM_CHECK_KINDS))
    ap.add_argument("--iters", type=int, default=2000,
                    help="iterations per timed window at size 4096; other sizes scale "
                         "with 1/size^3 so every window holds the same work")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    ext = hipcore.load_ext()
    probes = {"bf16": ext.gemm_bf16_8ph_tflops, "fp8": ext.gemm_fp8_mx_tflops,
              "fp4": ext.gemm_fp4_mx_tflops}
    doc = {"rounds": args.rounds, "series": []}
    doc["stream_gbps"] = [round(ext.stream_bandwidth_gbps(args.device, 1024, 10), 1)
                          for _ in range(3)]
    print(f"stream_bandwidth_gbps (read + write): {doc['stream_gbps']}")
    for size in args.sizes:
        for kind in args.formats:
            rng = hipcore.gemm_check_range(kind, size)
            iters = max(20, int(args.iters * (4096.0 / size) ** 3))
            flop = 2.0 * size**3
            us = {name: [] for name in LOOPS + ("probe",)}
            errors = 0
            for _ in range(args.rounds):
                for loop in LOOPS:
                    raw = ext.gemm_check(args.device, kind, size, iters,
                                         hipcore.GEMM_CHECK_SEED, rng, -1, 8, [], loop)
                    errors += sum(raw["errors"].values()) + raw["operand_errors"]
                    us[loop].append(raw["seconds"] / iters * 1e6)
                tf = probes[kind](args.device, size, iters)
                us["probe"].append(flop / (tf * 1e12) * 1e6)
            row = {"size": size, "kind": kind, "range": rng, "iters": iters, "errors": errors}
            for name, vals in us.items():
                row[name] = {"us": [round(v, 2) for v in vals],
                             "median_us": round(statistics.median(vals), 2)}
            base = row["unchecked"]["median_us"]
            row["unchecked_tflops"] = round(flop / base / 1e6, 1)
            row["probe_tflops"] = round(flop / row["probe"]["median_us"] / 1e6, 1)
            row["serial_over_unchecked"] = round(row["serial"]["median_us"] / base, 4)
            row["overlap_over_unchecked"] = round(row["overlap"]["median_us"] / base, 4)
            row["verify_read_gbps"] = round(4.0 * size * size / row["verify"]["median_us"] / 1e3, 1)
            row["verify_cold_read_gbps"] = round(
                4.0 * size * size / row["verify-cold"]["median_us"] / 1e3, 1)
            doc["series"].append(row)
            print(f"{kind:5s} {size:6d} range {rng:3d} errors {errors}: " + "  ".join(
                f"{n} {row[n]['median_us']:.1f} ({min(us[n]):.1f}..{max(us[n]):.1f})" for n in us)
                + f"  serial x{row['serial_over_unchecked']:.3f} overlap x"
                f"{row['overlap_over_unchecked']:.3f}  verify {row['verify_read_gbps']:.0f} / cold {row['verify_cold_read_gbps']:.0f} GB/s"
                f"  TF exact {row['unchecked_tflops']:.0f} probe {row['probe_tflops']:.0f}",
                flush=True)
    text = json.dumps(doc)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
