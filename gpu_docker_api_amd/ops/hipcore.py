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


VALU_CHECK_SEED = 0x7A1C0DE5EED5A1D5
VALU_CHECK_ROUNDS = 8
VALU_CHECK_TESTS = ("int", "f32", "f64", "pk16", "trans")


def valu_check_fold(records: list, cus_expected: int) -> dict:
    """Fold the per-workgroup records of valu_check by the SIMD each wave ran
    on: (cu_check_key, SIMD field of that wave's HW_ID). Pure Python.
    `bad_simds` lists every SIMD with a mismatch, with its counts per test and
    the first mismatch one of its waves reported. Coverage (`cus_seen`,
    `simds_seen`) is reported, never judged. `trans_reference_suspect` is true
    when more than half of the SIMDs seen report trans mismatches while their
    exact tests are clean: the one workgroup the trans table came from is then
    the likelier culprit than half the card."""
    simds: dict = {}
    cus = set()
    split = 0
    errors = {t: 0 for t in VALU_CHECK_TESTS}
    for rec in records:
        key = cu_check_key(rec)
        cus.add(key)
        if len({(int(h) >> 8) & 0xFF for h in rec["hw_id"]}) > 1:
            split += 1  # waves of one workgroup on different "CUs": layout is off
        for hw, wave in zip(rec["hw_id"], rec["waves"]):
            simd = simds.setdefault(
                (key, hw_id_fields(hw)["simd"]),
                {"tests": {t: 0 for t in VALU_CHECK_TESTS}, "first": None},
            )
            for t in VALU_CHECK_TESTS:
                n = int(wave["counts"].get(t, 0))
                simd["tests"][t] += n
                errors[t] += n
            if simd["first"] is None and wave.get("first") is not None:
                simd["first"] = dict(wave["first"])
    bad = []
    trans_only = 0
    for (key, s) in sorted(simds):
        simd = simds[(key, s)]
        total = sum(simd["tests"].values())
        if total == 0:
            continue
        if simd["tests"]["trans"] == total:
            trans_only += 1
        f = hw_id_fields(key << 8)
        bad.append(
            {
                "xcc": key >> 8,
                "se": f["se"],
                "sh": f["sh"],
                "cu": f["cu"],
                "simd": s,
                "key": key,
                "tests": dict(simd["tests"]),
                "first": simd["first"],
            }
        )
    return {
        "cus_expected": int(cus_expected),
        "cus_seen": len(cus),
        "simds_seen": len(simds),
        "workgroups": len(records),
        "split_workgroups": split,
        "errors": {"total": sum(errors.values()), **errors},
        "bad_simds": bad,
        "trans_reference_suspect": 2 * trans_only > len(simds),
    }


def valu_check_gpu(
    index: int,
    rounds: int = VALU_CHECK_ROUNDS,
    seed: int = VALU_CHECK_SEED,
    inject: Optional[list] = None,
) -> dict:
    """Per-SIMD vector ALU check of GPU `index` (csrc/valu_check.hip): every
    SIMD of every CU runs `rounds` rounds of integer, fp32, fp64, packed-fp16
    and transcendental chains and compares each lane's digest with a table
    (computed on the host for the exact tests, taken from a reference launch
    for trans). Returns the fold by SIMD plus how the pass ran."""
    ext = load_ext()
    cus = int(ext.device_info(index)["multiProcessorCount"])
    raw = ext.valu_check(index, int(rounds), seed, 2, list(inject or []))
    report = valu_check_fold(raw["records"], cus)
    report["rounds"] = int(rounds)
    report["launches"] = raw["launches"]
    report["seconds"] = round(raw["seconds"], 4)
    report["table_seconds"] = round(raw["table_seconds"], 4)
    report["trans_reference"] = dict(raw["trans_reference"])
    return report


GEMM_CHECK_SEED = 0x6E44C4EC5EED0001
GEMM_CHECK_KINDS = ("bf16", "fp8", "fp4")
GEMM_CHECK_TILE = 256
GEMM_CHECK_MIN_SIZE = {"bf16": 256, "fp8": 256, "fp4": 512}
GEMM_CHECK_CODE = {"bf16": 0, "fp8": 16, "fp4": 16}  # the kernels validate_gpus times
GEMM_CHECK_RECORDS = 64
_NXCD = 8  # gemm_8ph::NXCD


def gemm_check_range(kind: str, K: int) -> int:
    """The operand range of the checked GEMM loop at inner extent K, the
    largest for which every partial sum stays an integer below 2^24 product
    granules (csrc/gemm_check.hip): bf16 numerators m/16 in [-r, r] with
    r = min(127, floor(sqrt(2^24 / K))); e4m3 exponent fields 6..6+w-1 with w
    the largest of 1..4 with (15 * 2^(w-1))^2 * K <= 2^24; e2m1 all 16 codes."""
    import math

    K = int(K)
    if K < 1:
        raise ValueError("K must be positive")
    if kind == "bf16":
        r = min(127, math.isqrt((1 << 24) // K))
        if r < 1:
            raise ValueError(f"no exact bf16 operand range at K = {K}")
        return r
    if kind == "fp8":
        for w in (4, 3, 2, 1):
            if (15 << (w - 1)) ** 2 * K <= 1 << 24:
                return w
        raise ValueError(f"no exact fp8 operand range at K = {K}")
    if kind == "fp4":
        if 144 * K > 1 << 24:
            raise ValueError(f"no exact fp4 operand range at K = {K}")
        return 16
    raise ValueError(f"unknown kind {kind!r} (bf16, fp8, fp4)")


def _xcd_start(x: int, nwg: int) -> int:
    q, r = divmod(nwg, _NXCD)
    return x * (q + 1) if x < r else r * (q + 1) + (x - r) * q


def gemm_check_owner(tile_row: int, tile_col: int, tiles_n: int, nwg: int, xcd_remap: bool):
    """(blockIdx.x, blockIdx.x % 8) of the workgroup of an `nwg`-workgroup
    256^2 GEMM launch that computes tile (tile_row, tile_col): the inverse of
    tile_coord in csrc/gemm_8phase_common.h. With xcd_remap (the odd bf16
    codes) workgroup b takes tile start(b % 8) + b // 8, where XCD x owns a
    contiguous range of tiles; the second value is the XCD a workgroup runs
    on under round-robin dispatch."""
    t = tile_row * tiles_n + tile_col
    if not (0 <= tile_col < tiles_n and 0 <= t < nwg):
        raise ValueError(f"tile ({tile_row}, {tile_col}) is outside the launch")
    bid = t
    if xcd_remap:
        q, r = divmod(nwg, _NXCD)
        # the first r XCDs own q + 1 tiles each, the others q
        xcd = t // (q + 1) if t < r * (q + 1) else r + (t - r * (q + 1)) // q
        bid = (t - _xcd_start(xcd, nwg)) * _NXCD + xcd
    return bid, bid % _NXCD


def gemm_check_fold(raw: dict, tiles_n: int, nwg: int, xcd_remap: bool) -> dict:
    """Group the records of a checked GEMM run by (iteration, tile). Pure
    Python. Each bad tile names the workgroup that computed it and lists its
    mismatching rows and columns in product granules; `element` appears only
    where it can be pinned: exactly one row and one column of the tile
    mismatch, by the same delta, and nothing in it is malformed. A whole line
    of bad tiles (what a flipped operand word gives) is listed in `bands`.
    Records are capped on the device, counts are not: `records_truncated`
    says that findings exist beyond the ones folded here."""
    tiles: dict = {}
    for rec in raw["records"]:
        key = (int(rec["iter"]), int(rec["tile_row"]), int(rec["tile_col"]))
        t = tiles.setdefault(key, {"rows": [], "cols": [], "malformed": []})
        if rec["type"] == "malformed":
            t["malformed"].append(
                {"row": int(rec["row"]), "col": int(rec["col"]), "bits": int(rec["bits"])}
            )
        else:
            name = "row" if rec["type"] == "row" else "col"
            t[name + "s"].append(
                {name: int(rec["index"]), "got": int(rec["got"]), "want": int(rec["want"])}
            )
    tiles_m = max(1, nwg // tiles_n)
    bad_tiles = []
    by_mod8 = [0] * _NXCD
    lines: dict = {}
    for key in sorted(tiles):
        it, tr, tc = key
        t = tiles[key]
        block, mod8 = gemm_check_owner(tr, tc, tiles_n, nwg, xcd_remap)
        entry = {
            "iter": it,
            "tile": [tr, tc],
            "block": block,
            "block_mod8": mod8,
            "rows": sorted(t["rows"], key=lambda e: e["row"]),
            "cols": sorted(t["cols"], key=lambda e: e["col"]),
            "malformed": sorted(t["malformed"], key=lambda e: (e["row"], e["col"])),
        }
        if len(t["rows"]) == 1 and len(t["cols"]) == 1 and not t["malformed"]:
            dr = t["rows"][0]["got"] - t["rows"][0]["want"]
            dc = t["cols"][0]["got"] - t["cols"][0]["want"]
            if dr == dc:
                entry["element"] = {
                    "row": tr * GEMM_CHECK_TILE + t["rows"][0]["row"],
                    "col": tc * GEMM_CHECK_TILE + t["cols"][0]["col"],
                    "delta": dr,
                }
        bad_tiles.append(entry)
        by_mod8[mod8] += 1
        lines.setdefault((it, "row", tr), set()).add(tc)
        lines.setdefault((it, "col", tc), set()).add(tr)
    bands = [
        {"iter": it, "axis": axis, "index": index, "tiles": len(members)}
        for (it, axis, index), members in sorted(lines.items())
        if len(members) > 1 and len(members) == (tiles_n if axis == "row" else tiles_m)
    ]
    errors = {k: int(raw["errors"][k]) for k in ("rows", "cols", "malformed")}
    return {
        "errors": errors,
        "bad_tiles": bad_tiles,
        "bands": bands,
        "by_block_mod8": by_mod8,
        "records_truncated": sum(errors.values()) > len(raw["records"]),
    }


def gemm_check_gpu(
    index: int,
    size: int = 4096,
    iters: int = 10,
    formats=GEMM_CHECK_KINDS,
    seed: int = GEMM_CHECK_SEED,
    inject: Optional[list] = None,
) -> dict:
    """Checked GEMM loop on GPU `index` (csrc/gemm_check.hip): per format,
    `iters` full-size launches of the kernel validate_gpus times, on operands
    whose sums are exact, each result verified on the device with integer row
    and column checksums per 256^2 tile. fp4 is skipped below size 512, as in
    the throughput tier. `tflops` is information, not a health criterion: the
    exact operand sets toggle fewer bits than the probes' hash fills."""
    ext = load_ext()
    size = max(GEMM_CHECK_TILE, (int(size) // GEMM_CHECK_TILE) * GEMM_CHECK_TILE)
    tiles = size // GEMM_CHECK_TILE
    report = {"size": size, "iters": int(iters), "formats": {}}
    total = 0
    for kind in formats:
        if size < GEMM_CHECK_MIN_SIZE[kind]:
            continue
        code = GEMM_CHECK_CODE[kind]
        raw = ext.gemm_check(
            index, kind, size, int(iters), seed, gemm_check_range(kind, size), code,
            GEMM_CHECK_RECORDS, list(inject or []),
        )
        entry = gemm_check_fold(raw, tiles, tiles * tiles, kind == "bf16" and code % 2 == 1)
        entry["operand_errors"] = int(raw["operand_errors"])
        entry["seconds"] = round(raw["seconds"], 4)
        entry["tflops"] = round(raw["tflops"], 1)
        entry["checked_bytes"] = int(raw["checked_bytes"])
        total += sum(entry["errors"].values()) + entry["operand_errors"]
        report["formats"][kind] = entry
    report["errors_total"] = total
    return report


def validate_gpus(
    indices: Optional[list] = None,
    size: int = 4096,
    iters: int = 5,
    fp8: bool = True,
    memtest_mib: int = 0,
    cu_rounds: int = 0,
    gemm_check_iters: int = 0,
    valu_rounds: int = 0,
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
    CUs the pass did not reach are reported, not judged. With
    gemm_check_iters > 0 each GPU also gets the checked GEMM loop
    (gemm_check_gpu) at `size` and is unhealthy if a single checksum, element
    or stored operand was wrong in any format. With valu_rounds > 0 each GPU
    also gets the per-SIMD vector ALU check (valu_check_gpu) and is unhealthy
    if a single lane's digest was wrong."""
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
        if gemm_check_iters > 0:
            entry["gemm_check"] = gemm_check_gpu(i, size, gemm_check_iters)
        if valu_rounds > 0:
            entry["valu_check"] = valu_check_gpu(i, valu_rounds)
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
            if "gemm_check" in g:
                g["healthy"] = bool(g["healthy"] and g["gemm_check"]["errors_total"] == 0)
            if "valu_check" in g:
                g["healthy"] = bool(g["healthy"] and g["valu_check"]["errors"]["total"] == 0)
    return report


async def validate_gpus_async(
    indices: Optional[list] = None,
    size: int = 4096,
    iters: int = 5,
    memtest_mib: int = 0,
    cu_rounds: int = 0,
    gemm_check_iters: int = 0,
    valu_rounds: int = 0,
) -> dict:
    return await asyncio.get_running_loop().run_in_executor(
        None,
        lambda: validate_gpus(
            indices,
            size,
            iters,
            memtest_mib=memtest_mib,
            cu_rounds=cu_rounds,
            gemm_check_iters=gemm_check_iters,
            valu_rounds=valu_rounds,
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
