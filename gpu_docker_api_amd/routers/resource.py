"""Resource routes (reference: internal/routers/resource.go:11-38), extended
with what an MI355X operator actually needs: per-GPU HBM free/used bytes and
the xGMI adjacency matrix (SURVEY.md §2.4 last row)."""
from __future__ import annotations

from fastapi import APIRouter, Request

from ..parallel import CpuScheduler, GpuScheduler, PortScheduler
from .response import success


def make_router(gpu: GpuScheduler, cpu: CpuScheduler, ports: PortScheduler) -> APIRouter:
    r = APIRouter(prefix="/api/v1/resources")

    @r.get("/gpus")
    async def gpus():
        # reference shape: the uuid -> 0|1 map verbatim
        return success(gpu.get_gpu_status())

    @r.get("/gpus/detail")
    async def gpus_detail():
        # MI355X extension: HBM bytes + xGMI adjacency for job sizing
        return success(gpu.get_detail())

    @r.post("/gpus/validate")
    async def gpus_validate(request: Request):
        """MI355X extension: burn-in the node's FREE GPUs (HBM bandwidth +
        dense bf16 MFMA GEMM, with `memtestMiB` an HBM pattern memory test
        with `cuCheck` a per-CU MFMA and LDS check, with `gemmCheck` a
        checked loop of the full-size GEMMs, with `valuCheck` a per-SIMD
        vector ALU check) before trusting them
        with placements. Busy GPUs are skipped unless explicitly listed."""
        try:
            body = await request.json()
        except Exception:
            body = {}
        if not isinstance(body, dict):
            from .codes import Code
            from .response import error

            return error(Code.INVALID_PARAMS)
        requested = body.get("gpus")
        status = gpu.get_gpu_status()
        if requested:
            idx = [
                g.index
                for u in requested
                if (g := gpu.info_by_uuid(u)) is not None
            ]
        else:
            idx = [
                g.index for g in gpu.gpus if status.get(g.uuid, 1) == 0
            ]
        try:
            size = int(body.get("size", 4096))
            iters = int(body.get("iters", 5))
            memtest = body.get("memtestMiB", 0)
            if isinstance(memtest, bool) or not isinstance(memtest, int):
                raise TypeError("memtestMiB must be an int")
            cu_rounds = body.get("cuCheck", 0)
            if isinstance(cu_rounds, bool) or not isinstance(cu_rounds, int):
                raise TypeError("cuCheck must be an int")
            gemm_check = body.get("gemmCheck", 0)
            if isinstance(gemm_check, bool) or not isinstance(gemm_check, int):
                raise TypeError("gemmCheck must be an int")
            valu_rounds = body.get("valuCheck", 0)
            if isinstance(valu_rounds, bool) or not isinstance(valu_rounds, int):
                raise TypeError("valuCheck must be an int")
        except (TypeError, ValueError):
            from .codes import Code
            from .response import error

            return error(Code.INVALID_PARAMS)
        try:
            from ..ops import hipcore

            # HBM pattern test: off at 0, else 1 GiB .. the whole 288 GB card
            if memtest != 0:
                memtest = max(1024, min(memtest, 294912))
            # per-CU compute check: off at 0, else 1 .. 4096 rounds
            extra = {}
            if cu_rounds != 0:
                extra["cu_rounds"] = max(1, min(cu_rounds, 4096))
            # checked GEMM loop: off at 0, else 1 .. 100000 iterations a format
            if gemm_check != 0:
                extra["gemm_check_iters"] = max(1, min(gemm_check, 100000))
            # per-SIMD vector ALU check: off at 0, else 1 .. 4096 rounds
            if valu_rounds != 0:
                extra["valu_rounds"] = max(1, min(valu_rounds, 4096))
            report = await hipcore.validate_gpus_async(
                idx,
                max(256, min(size, 16384)),
                max(1, min(iters, 50)),
                memtest_mib=memtest,
                **extra,
            )
        except Exception as exc:  # noqa: BLE001 — no GPU / extension absent
            from .codes import Code
            from .response import error

            return error(Code.SERVER_BUSY, detail=f"validation unavailable: {exc}")
        return success(report)

    @r.get("/cpus")
    async def cpus():
        return success(cpu.get_cpu_status())

    @r.get("/ports")
    async def port_status():
        return success(ports.get_port_status())

    return r
