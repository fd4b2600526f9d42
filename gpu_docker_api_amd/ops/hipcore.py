"""Python facade over the _hipcore extension + the rccl_smoke binary.

Fails loudly when a GPU is present but the native extension is missing
(NativeOpUnavailable) — GPU paths must never silently fall back.
"""
from __future__ import annotations

import asyncio
import json
import os
import subprocess
from typing import Optional

from ..xerrors import NativeOpUnavailable

_ext = None
_ext_err: Optional[str] = None


def load_ext():
    """Load the _hipcore torch extension (torch must be imported first so
    libtorch*.so are resolvable)."""
    global _ext, _ext_err
    if _ext is not None:
        return _ext
    if _ext_err is not None:
        raise NativeOpUnavailable(_ext_err)
    try:
        import importlib.util
        import torch  # noqa: F401  (loads libtorch into the process)

        so = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_hipcore.so")
        if not os.path.exists(so):
            raise FileNotFoundError(f"{so} not built (run ops.build)")
        spec = importlib.util.spec_from_file_location("_hipcore", so)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _ext = mod
        return _ext
    except Exception as exc:
        _ext_err = f"native _hipcore unavailable: {exc}"
        raise NativeOpUnavailable(_ext_err) from exc


def gpu_available() -> bool:
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:
        return False


def run_probe(mib: int = 256, iters: int = 5) -> dict:
    """Measure HBM stream + pairwise p2p bandwidth across visible GPUs.

    Returns {"gpus": [uuid...], "hbm_gbps": [...], "p2p_gbps": [[...]]} —
    the shape parallel.topology.Topology.overlay_measured consumes. GPU
    identity comes from torch (HIP enumeration order); UUIDs are taken from
    the amdsmi inventory at matching indices when available.
    """
    ext = load_ext()
    n = ext.device_count()
    if n == 0:
        raise NativeOpUnavailable("no HIP devices visible")
    uuids = [f"GPU-{i}" for i in range(n)]
    try:
        from ..parallel.inventory import AmdSmiInventory

        infos = AmdSmiInventory().enumerate()
        if len(infos) == n:
            uuids = [g.uuid for g in infos]
    except Exception:
        pass
    # one-shot matrix: per-device buffers allocated once (on an 8-GPU node
    # per-pair re-allocation would cost minutes of daemon startup)
    mat = ext.p2p_matrix(mib, iters)
    hbm = [round(mat[i][i], 1) for i in range(n)]
    p2p = [
        [0.0 if i == j else round(mat[i][j], 1) for j in range(n)] for i in range(n)
    ]
    return {"gpus": uuids, "hbm_gbps": hbm, "p2p_gbps": p2p}


async def run_probe_async(mib: int = 256, iters: int = 5) -> dict:
    return await asyncio.get_running_loop().run_in_executor(
        None, lambda: run_probe(mib, iters)
    )


MEMTEST_SEED = 0x0123456789ABCDEF
_GIB = 1 << 30


def memtest_plan(
    free_bytes: int, want_bytes: int, chunk_bytes: int = 1 << 30, reserve_bytes: int = 2 << 30
) -> list:
    """Chunk sizes for an HBM pattern test: min(want, free - reserve) rounded
    down to a multiple of 16, cut into chunk_bytes pieces with one short last
    chunk. Empty when less than 1 GiB would remain: every step covers all
    chunks before the next one starts, and below that the read-back could be
    served from the 256 MiB Infinity Cache instead of HBM."""
    total = (min(int(want_bytes), int(free_bytes) - int(reserve_bytes)) // 16) * 16
    if total < _GIB:
        return []
    chunk = max(16, (int(chunk_bytes) // 16) * 16)
    plan = [chunk] * (total // chunk)
    if total % chunk:
        plan.append(total % chunk)
    return plan


def memtest_gpu(
    index: int,
    mib: int = 4096,
    seed: int = MEMTEST_SEED,
    scrub: bool = False,
    inject: Optional[list] = None,
) -> dict:
    """HBM data-integrity pass over `mib` MiB of GPU `index` (address and
    pseudorandom patterns, written, read back, complemented and read back
    again; csrc/hbm_memtest.hip). The plan comes from the free HBM hipMemGetInfo
    reports, less a reserve for the runtime."""
    ext = load_ext()
    free = int(ext.device_info(index)["freeMem"])
    plan = memtest_plan(free, int(mib) << 20)
    if not plan:
        return {"skipped": "insufficient free HBM"}
    report = ext.hbm_memtest(index, plan, seed, 32, scrub, list(inject or []))
    for key, digits in (("write_gbps", 1), ("verify_gbps", 1), ("seconds", 4)):
        if key in report:
            report[key] = round(report[key], digits)
    return report


CU_CHECK_SEED = 0x5EEDC0DEC0FFEE11
CU_CHECK_ROUNDS = 8
CU_CHECK_TESTS = ("bf16", "fp8", "fp4", "lds")


def hw_id_fields(hw_id: int) -> dict:
    """HW_REG_HW_ID as the CDNA ISA documents it: wave 3:0, simd 5:4, pipe
    7:6, cu 11:8, sh 12, se 15:13. The layout is a presentation of the raw
    word; a CU's identity never rests on it (cu_check_key)."""
    hw_id = int(hw_id)
    return {
        "wave": hw_id & 0xF,
        "simd": (hw_id >> 4) & 0x3,
        "pipe": (hw_id >> 6) & 0x3,
        "cu": (hw_id >> 8) & 0xF,
        "sh": (hw_id >> 12) & 0x1,
        "se": (hw_id >> 13) & 0x7,
    }


def cu_check_key(record: dict) -> int:
    """The CU a workgroup ran on: xcc << 8 | HW_ID bits 15:8 (SE, SH and CU
    together) of its first wave, raw."""
    return (int(record["xcc"]) & 0xF) << 8 | (int(record["hw_id"][0]) >> 8) & 0xFF


def cu_check_fold(records: list, cus_expected: int) -> dict:
    """Fold the per-workgroup records of cu_check by the CU they ran on.
    Pure Python. `bad_cus` lists every CU with a mismatch, with its counts per
    test and the first mismatch one of its workgroups reported. Coverage
    (`cus_seen` against `cus_expected`) is reported, never judged: a busy GPU
    places workgroups unevenly."""
    cus: dict = {}
    simds = set()
    split = 0
    errors = {t: 0 for t in CU_CHECK_TESTS}
    for rec in records:
        key = cu_check_key(rec)
        if len({(int(h) >> 8) & 0xFF for h in rec["hw_id"]}) > 1:
            split += 1  # waves of one workgroup on different "CUs": layout is off
        simds.update(hw_id_fields(h)["simd"] for h in rec["hw_id"])
        cu = cus.setdefault(
            key, {"workgroups": 0, "tests": {t: 0 for t in CU_CHECK_TESTS}, "first": None}
        )
        cu["workgroups"] += 1
        for t in CU_CHECK_TESTS:
            n = int(rec["counts"].get(t, 0))
            cu["tests"][t] += n
            errors[t] += n
        if cu["first"] is None and rec.get("first") is not None:
            cu["first"] = dict(rec["first"])
            wave = int(cu["first"].get("wave", 0))
            if 0 <= wave < len(rec["hw_id"]):  # the SIMD that wave ran on
                cu["first"]["simd"] = hw_id_fields(rec["hw_id"][wave])["simd"]
    per_xcc: dict = {}
    for key in cus:
        per_xcc[key >> 8] = per_xcc.get(key >> 8, 0) + 1
    bad = []
    for key in sorted(cus):
        cu = cus[key]
        if sum(cu["tests"].values()) == 0:
            continue
        f = hw_id_fields(key << 8)
        bad.append(
            {
                "xcc": key >> 8,
                "se": f["se"],
                "sh": f["sh"],
                "cu": f["cu"],
                "key": key,
                "tests": dict(cu["tests"]),
                "first": cu["first"],
            }
        )
    return {
        "cus_expected": int(cus_expected),
        "cus_seen": len(cus),
        "xccs": [{"xcc": x, "cus": per_xcc[x]} for x in sorted(per_xcc)],
        "simds_seen": sorted(simds),
        "workgroups": len(records),
        "split_workgroups": split,
        "errors": {"total": sum(errors.values()), **errors},
        "bad_cus": bad,
    }


def cu_check_gpu(
    index: int,
    rounds: int = CU_CHECK_ROUNDS,
    seed: int = CU_CHECK_SEED,
    inject: Optional[list] = None,
) -> dict:
    """Per-CU compute check of GPU `index` (csrc/cu_check.hip): every CU
    computes `rounds` x 4 exact tiles in bf16, MX-fp8 and MX-fp4, compares
    them with integer arithmetic on the spot and pattern-tests its whole LDS.
    Returns the fold by CU plus how the pass ran."""
    ext = load_ext()
    cus = int(ext.device_info(index)["multiProcessorCount"])
    raw = ext.cu_check(index, int(rounds), seed, 2, list(inject or []))
    report = cu_check_fold(raw["records"], cus)
    report["rounds"] = int(rounds)
    report["launches"] = raw["launches"]
    report["lds_bytes"] = raw["lds_bytes"]
    report["seconds"] = round(raw["seconds"], 4)
    return report


def validate_gpus(
    indices: Optional[list] = None,
    size: int = 4096,
    iters: int = 5,
    fp8: bool = True,
    memtest_mib: int = 0,
    cu_rounds: int = 0,
) -> dict:
    """Per-GPU health burn-in: HBM stream bandwidth + dense bf16 MFMA GEMM
    (the 8-phase 256^2 structure, ~1.1 PF) + the MX-fp8 path (block-scaled
    mfma_scale 16x16x128, ~1.9 PF — exercised because fp8 training is what
    tenants run on MI355X and its datapath can fail independently of bf16).
    Run on FREE GPUs before scheduling; a GPU far below its siblings is
    flagged. With memtest_mib > 0 each GPU also gets the HBM pattern test
    (memtest_gpu) and is unhealthy if a single word read back wrong. With
    cu_rounds > 0 each GPU also gets the per-CU MFMA and LDS check
    (cu_check_gpu) and is unhealthy if a single result or LDS word was wrong;
    CUs the pass did not reach are reported, not judged."""
    ext = load_ext()
    n = ext.device_count()
    idx = list(indices) if indices else list(range(n))
    size = max(256, (size // 256) * 256)  # kernel tile constraints
    report = {"gpus": []}
    for i in idx:
        if i < 0 or i >= n:
            continue
        hbm = ext.stream_bandwidth_gbps(i, 1024, 5)
        # the 8-phase 256^2 pipelined structure (~1000 TF); size always fits it
        tflops = ext.gemm_bf16_8ph_tflops(i, size, iters)
        entry = {
            "index": i,
            "hbm_gbps": round(hbm, 1),
            "bf16_tflops": round(tflops, 1),
        }
        if fp8:
            entry["fp8_tflops"] = round(ext.gemm_fp8_mx_tflops(i, size, iters), 1)
        if fp8 and size >= 512:  # the fp4 kernel needs K >= 512
            entry["fp4_tflops"] = round(ext.gemm_fp4_mx_tflops(i, size, iters), 1)
        if memtest_mib > 0:
            entry["memtest"] = memtest_gpu(i, memtest_mib)
        if cu_rounds > 0:
            entry["cu_check"] = cu_check_gpu(i, cu_rounds)
        report["gpus"].append(entry)
    vals = [g["bf16_tflops"] for g in report["gpus"]]
    if vals:
        top = max(vals)
        for g in report["gpus"]:
            g["healthy"] = bool(g["bf16_tflops"] > 0.7 * top and g["hbm_gbps"] > 2000)
            if "memtest" in g and "errors" in g["memtest"]:
                g["healthy"] = bool(g["healthy"] and g["memtest"]["errors"] == 0)
            if "cu_check" in g:
                g["healthy"] = bool(g["healthy"] and g["cu_check"]["errors"]["total"] == 0)
    return report


async def validate_gpus_async(
    indices: Optional[list] = None,
    size: int = 4096,
    iters: int = 5,
    memtest_mib: int = 0,
    cu_rounds: int = 0,
) -> dict:
    return await asyncio.get_running_loop().run_in_executor(
        None,
        lambda: validate_gpus(
            indices, size, iters, memtest_mib=memtest_mib, cu_rounds=cu_rounds
        ),
    )


def rccl_smoke_path() -> str:
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    return os.path.join(root, "csrc", "bin", "rccl_smoke")


def run_rccl_smoke(ndev: int = 0, mib: int = 64, timeout: float = 120.0) -> dict:
    """Run the native RCCL all-reduce smoke binary; returns its JSON verdict."""
    binary = rccl_smoke_path()
    if not os.path.exists(binary):
        raise NativeOpUnavailable(f"{binary} not built (run ops.build)")
    cmd = [binary]
    if ndev > 0:
        cmd.append(str(ndev))
        cmd.append(str(mib))
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    line = (out.stdout.strip().splitlines() or ["{}"])[-1]
    try:
        result = json.loads(line)
    except json.JSONDecodeError:
        result = {"ok": False, "error": f"unparseable output: {line!r}", "rc": out.returncode}
    result.setdefault("ok", False)
    return result


async def run_rccl_smoke_async(ndev: int = 0, mib: int = 64) -> dict:
    return await asyncio.get_running_loop().run_in_executor(
        None, lambda: run_rccl_smoke(ndev, mib)
    )
