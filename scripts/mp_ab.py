#!/usr/bin/env python3
"""Merged-phase MX variant A/B (shape 16 default vs 19/20 merged)."""
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
    out["fp8_mp_err_over_bound"] = _screen.screen_fp8_mx(ext, 20)  # worst err/bound
    out["fp4_mp_exact"] = _screen.screen_fp4_mx(ext, 19)

    for size, iters in ((4096, 6), (8192, 3)):
        for key in ("fp4_16", "fp4_19", "fp8_16", "fp8_20"):
            out.setdefault(f"{key}_{size}", [])
        for _ in range(3):
            # merged FIRST this run (position/clock-ramp bias control)
            out[f"fp4_19_{size}"].append(round(ext.gemm_fp4_mx_tflops(0, size, iters, shape=19), 1))
            out[f"fp4_16_{size}"].append(round(ext.gemm_fp4_mx_tflops(0, size, iters, shape=16), 1))
            out[f"fp8_20_{size}"].append(round(ext.gemm_fp8_mx_tflops(0, size, iters, shape=20), 1))
            out[f"fp8_16_{size}"].append(round(ext.gemm_fp8_mx_tflops(0, size, iters, shape=16), 1))
    print(json.dumps(out))
    os.makedirs("gpurun_out", exist_ok=True)
    open("gpurun_out/mp_ab.json", "w").write(json.dumps(out))


if __name__ == "__main__":
    main()
