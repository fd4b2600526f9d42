"""Numerics race screens shared by the A/B scripts.

A variant must not win an A/B because it is wrong: every screen here writes
into a NaN-poisoned `out` with a guard zone, re-poisoned before each run, and
judges each element against a float64 reference with the derived bound of
tests/kernel_refs.py (the same comparators the GPU test suite uses; the full
variant x shape matrix lives in tests/test_gpu_kernels.py).
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

import kernel_refs as kr  # noqa: E402


def _run(call, M, N, compare, reps, label):
    import torch

    buf = kr.PoisonedOut(M * N, "cuda", shape=(M, N))
    worst = 0.0
    for rep in range(reps):
        buf.poison()
        call(buf.out)
        torch.cuda.synchronize()
        worst = max(worst, compare(buf.out) or 0.0)
        buf.check(f"{label} run {rep}")
    return worst


def screen_bf16_8ph(ext, variant, size, reps=4, seed=11, operands=None):
    """Real-valued bf16 operands, per-element K*2^-23*(|A|@|B|^T) bound.
    Returns (worst err/bound, operands) so one problem serves all variants."""
    import torch

    if operands is None:
        g = torch.Generator(device="cuda").manual_seed(seed + size)
        A = (torch.randn(size, size, device="cuda", generator=g) * 0.5).bfloat16()
        Bt = (torch.randn(size, size, device="cuda", generator=g) * 0.5).bfloat16()
        a64, b64 = A.double(), Bt.double()  # float64 on the device: 4096^3 is slow on a CPU
        operands = (A, Bt, (a64 @ b64.T).cpu(),
                    kr.sum_bound(a64.abs(), b64.abs(), size).cpu())
    A, Bt, ref, bound = operands
    worst = _run(
        lambda out: ext.gemm_bf16_8ph(A, Bt, variant=variant, out=out), size, size,
        lambda C: kr.assert_within_sum_bound(C, ref, None, None, size, bound=bound),
        reps, f"gemm_bf16_8ph v{variant} {size}^3")
    return worst, operands


def screen_fp8_mx(ext, code, reps=4, M=512, N=256, K=512, seed=9):
    """randn*0.5 e4m3 operands at the plain bound against the float64 model of
    the MX instruction's product truncation (docs/testing.md)."""
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    A = (torch.randn(M, K, device="cuda", generator=g) * 0.5).to(torch.float8_e4m3fn).view(torch.uint8)
    Bt = (torch.randn(N, K, device="cuda", generator=g) * 0.5).to(torch.float8_e4m3fn).view(torch.uint8)
    a64 = torch.from_numpy(kr.E4M3_LUT[A.cpu().numpy()])
    b64 = torch.from_numpy(kr.E4M3_LUT[Bt.cpu().numpy()])
    model = kr.mx_fp8_truncated_reference(A, Bt)
    bound = kr.sum_bound(a64.abs(), b64.abs(), K)
    ref = kr.reference(a64, b64)
    scale = ref.abs().max().item() + 1e-6

    def compare(C):
        # the scripts' earlier max-norm check stays, next to the per-element one
        rel = (C.cpu().double() - ref).abs().max().item() / scale
        assert rel < 1e-3, f"gemm_fp8_mx shape={code}: rel err {rel}"
        return kr.assert_within_sum_bound(C, model, None, None, K, bound=bound)

    return _run(lambda out: ext.gemm_fp8_mx(A, Bt, shape=code, out=out), M, N,
                compare, reps, f"gemm_fp8_mx shape={code}")


def screen_fp4_mx(ext, code, reps=4, M=512, N=256, K=1024, seed=13):
    """All 16 e2m1 codes: sums are exact in fp32, so bit-equality."""
    packA, a64 = kr.all_e2m1(M, K, seed)
    packB, b64 = kr.all_e2m1(N, K, seed + 1)
    ref = kr.reference(a64, b64)
    A, Bt = packA.cuda(), packB.cuda()
    _run(lambda out: ext.gemm_fp4_mx(A, Bt, K, shape=code, out=out), M, N,
         lambda C: kr.assert_exact(C, ref), reps, f"gemm_fp4_mx shape={code}")
    return True
