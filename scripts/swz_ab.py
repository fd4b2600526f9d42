#!/usr/bin/env python3
"""fp8/fp4 swizzle-variant A/B (shape 16 = g(row)=row&7, 17 = +row bit 3)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import _screen
    from gpu_docker_api_amd.ops import hipcore

    ext = hipcore.load_ext()
    out = {}
    # numerics first (scripts/_screen.py): poisoned output, per-element bound
    out["fp8_swz1_err_over_bound"] = _screen.screen_fp8_mx(ext, 17)  # worst err/bound
    out["fp4_swz1_exact"] = _screen.screen_fp4_mx(ext, 17)

    for size, iters in ((4096, 6), (8192, 3)):
        for key in ("fp8_16", "fp8_17", "fp4_16", "fp4_17"):
            out.setdefault(f"{key}_{size}", [])
        for _ in range(3):
            out[f"fp8_16_{size}"].append(round(ext.gemm_fp8_mx_tflops(0, size, iters, shape=16), 1))
            out[f"fp8_17_{size}"].append(round(ext.gemm_fp8_mx_tflops(0, size, iters, shape=17), 1))
            out[f"fp4_16_{size}"].append(round(ext.gemm_fp4_mx_tflops(0, size, iters, shape=16), 1))
            out[f"fp4_17_{size}"].append(round(ext.gemm_fp4_mx_tflops(0, size, iters, shape=17), 1))
    print(json.dumps(out))
    os.makedirs("gpurun_out", exist_ok=True)
    open("gpurun_out/swz_ab.json", "w").write(json.dumps(out))


if __name__ == "__main__":
    main()
