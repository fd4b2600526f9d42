"""The 256^2 GEMM family at the scale the burn-in launches it, and the fills
that feed the burn-in's throughput probes (hardware-gated: `pytest -m gpu`).

tests/test_gpu_kernels.py checks layout: at most 16 workgroups, operands that
sit in L2, an idle device. The skeleton's counted vmcnt waits and its LDS slot
reuse are wrong only when a load lands late, so here every distinct
instantiation runs

  one-per-cu     one workgroup on every CU (remap quotient 32, remainder 0);
  second-round   more workgroups than CUs, so some start on a CU whose LDS
                 still holds another tile's operands (remainder 2);
  contended      second-round again while a side stream streams 1 GiB copies
                 through HBM, asserted to have overlapped the GEMM,

with exact operand sets larger than one XCD's L2. Run 0 must equal the
float64 reference bit for bit; runs 1 and 2 (re-poisoned) must equal run 0
bit for bit, compared on the device. A mismatch names the owning workgroup
and its blockIdx % 8 next to the tile, quadrant, wave and fragment.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import kernel_refs as kr
import test_gpu_kernels as tgk
from test_gpu_kernels import ext  # noqa: F401  (module-scoped fixture)

pytestmark = pytest.mark.gpu

TILE = kr.TILE
# distinct instantiations only: bf16 10, 11 and fp4 19 are table aliases
CODES = {
    "bf16": [0, 1, 2, 3, 4, 5, 6, 7, 12],
    "e4m3": [16, 17, 18, 20, 32],
    "e2m1": [16, 17, 18, 21, 32],
}
# the largest round K at which the exact sets still guarantee fp32-exact sums
K_FULL = {"bf16": 1024, "e4m3": 1152, "e2m1": 2048}
MODES = [("one-per-cu", False), ("second-round", False), ("second-round", True)]


def full_shapes(cus):
    """Tile grids (tiles_m, tiles_n) for a device with `cus` CUs.

    one-per-cu: the most nearly square grid of exactly `cus` tiles.
    second-round: the fewest tiles above `cus`, rows and columns each at most
    three more than one-per-cu's, with nwg % 8 >= 2 so the XCD remap runs
    with a remainder that gives two XCDs the longer range. 256 CUs give
    16 x 16 (nwg 256 = 8 * 32) and 17 x 18 (nwg 306 = 8 * 38 + 2)."""
    tm = max(d for d in range(1, math.isqrt(cus) + 1) if cus % d == 0)
    tn = cus // tm
    second = min(((m, n) for m in range(tm, tm + 4) for n in range(tn, tn + 4)
                  if m * n > cus and (m * n) % kr.NXCD >= 2),
                 key=lambda s: (s[0] * s[1], s))
    return {"one-per-cu": (tm, tn), "second-round": second}


def launch(ext, kind, code, p, out):
    if kind == "bf16":
        return ext.gemm_bf16_8ph(p["A"], p["Bt"], variant=code, out=out)
    if kind == "e4m3":
        return ext.gemm_fp8_mx(p["A"], p["Bt"], shape=code, out=out)
    return ext.gemm_fp4_mx(p["A"], p["Bt"], p["K"], shape=code, out=out)


@functools.lru_cache(maxsize=1)
def full_problem(kind, M, N):
    """tgk.problem (exactness condition checked, A and Bt from different
    seeds), but only the latest is kept: a reference here is 150 MB. The
    cases below are ordered so that each is built once."""
    return tgk.problem.__wrapped__(kind, M, N, K_FULL[kind])


@pytest.fixture(scope="module")
def shapes(ext):
    cus = int(ext.device_info(0)["multiProcessorCount"])
    s = full_shapes(cus)
    if cus != 256:
        print(f"FULL SHAPES for {cus} CUs: {s}")
    assert s["one-per-cu"][0] * s["one-per-cu"][1] == cus
    assert s["second-round"][0] * s["second-round"][1] > cus
    return s


COPY_FLOATS = (1 << 30) // 4
# at least ten idle GEMM durations of copies, and never fewer than 8: behind
# the copies a GEMM was measured to take 10 to 17 times its idle time, about
# two copies (docs/testing.md), and the queue must still outlast it
MIN_COPIES, MAX_COPIES = 8, 64


def _timed(stream, fn):
    """Milliseconds of `fn()` on `stream`, between two events."""
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        t0.record(stream)
        fn()
        t1.record(stream)
    t1.synchronize()
    return t0.elapsed_time(t1)


@pytest.fixture(scope="module")
def contention(ext):
    """Two streams of their own (the null stream would serialise them), a
    1 GiB copy for the side stream and the measured duration of one copy."""
    torch.cuda.synchronize()
    c = SimpleNamespace(
        src=torch.zeros(COPY_FLOATS, device="cuda"),
        dst=torch.empty(COPY_FLOATS, device="cuda"),
        side=torch.cuda.Stream(), main=torch.cuda.Stream())
    torch.cuda.synchronize()
    c.copy = lambda: ext.copy_f32(c.dst, c.src)
    _timed(c.side, c.copy)  # first touch
    c.copy_ms = _timed(c.side, c.copy)
    print(f"CONTENTION one 1 GiB copy_f32: {c.copy_ms:.3f} ms")
    yield c
    torch.cuda.synchronize()


def _with_owners(e, what, p, xcd_remap):
    tiles_n = p["N"] // TILE
    nwg = (p["M"] // TILE) * tiles_n
    e.args = (f"{what}: {e.args[0]}; "
              f"{kr.describe_owners(e, tiles_n, nwg, xcd_remap)}",)
    return e


def run_full(ext, kind, code, p, label, contention=None):
    """The protocol of tgk.run_protocol at full size: poisoned `out` with its
    guard, tgk.REPS runs re-poisoned each time. Run 0 is compared with the
    float64 reference on the CPU, later runs with run 0 on the device through
    int32 views (the kernels are deterministic: one wave owns each output and
    adds in a fixed order). With `contention`, every run is launched behind a
    queue of 1 GiB copies on a second stream and must have ended before
    them."""
    M, N = p["M"], p["N"]
    xcd_remap = kind == "bf16" and bool(code & 1)
    buf = kr.PoisonedOut(M * N, "cuda", shape=(M, N))
    n_copies = 0
    if contention is not None:
        c = contention
        torch.cuda.synchronize()  # the poison fill ran on the null stream
        gemm_ms = _timed(c.main, lambda: launch(ext, kind, code, p, buf.out))
        n_copies = min(MAX_COPIES, max(MIN_COPIES, math.ceil(10 * gemm_ms / c.copy_ms)))
        print(f"CONTENTION {label}: idle GEMM {gemm_ms:.3f} ms, copy "
              f"{c.copy_ms:.3f} ms, {n_copies} copies queued")
        assert n_copies * c.copy_ms >= 10 * gemm_ms, (n_copies, c.copy_ms, gemm_ms)
    first = None
    for rep in range(tgk.REPS):
        what = f"{label} run {rep}"
        buf.poison()
        torch.cuda.synchronize()
        if contention is None:
            ret = launch(ext, kind, code, p, buf.out)
            torch.cuda.synchronize()
        else:
            copies_done = torch.cuda.Event()
            with torch.cuda.stream(c.side):
                for _ in range(n_copies):
                    c.copy()
                copies_done.record(c.side)
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(c.main):
                t0.record(c.main)
                ret = launch(ext, kind, code, p, buf.out)
                t1.record(c.main)
            c.main.synchronize()
            copies_running = not copies_done.query()
            c.side.synchronize()
            torch.cuda.synchronize()
            print(f"CONTENTION {what}: GEMM behind the copies {t0.elapsed_time(t1):.3f} ms")
            assert copies_running, (
                f"{what}: the {n_copies} queued copies had ended before the "
                f"GEMM did, so the GEMM was not shown to run under contention")
        assert ret.data_ptr() == buf.out.data_ptr(), f"{what}: out not returned"
        assert buf.guard_intact(), f"{what}: guard behind out was overwritten"
        try:
            if first is None:
                kr.assert_exact(buf.out, p["ref"])
                first = buf.out.clone()
            else:
                bad = buf.out.view(torch.int32) != first.view(torch.int32)
                if bool(bad.any()):
                    raise kr.KernelMismatch(
                        "differs from run 0 (which equals the reference)",
                        bad.cpu(), buf.out.cpu(), first.cpu())
        except kr.KernelMismatch as e:
            raise _with_owners(e, what, p, xcd_remap) from None
    # bit-equal to a finite reference: nothing was left unwritten
    buf.check(label)


CASES = [(kind, name, contended, code)
         for kind in CODES for name, contended in MODES for code in CODES[kind]]


def _case_id(case):
    kind, name, contended, code = case
    return (f"{kind}-{'v' if kind == 'bf16' else 'c'}{code}-{name}-"
            f"{'contended' if contended else 'idle'}")


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_gemm_256_full_machine_exact(ext, shapes, request, case):  # noqa: F811
    kind, name, contended, code = case
    tm, tn = shapes[name]
    p = full_problem(kind, tm * TILE, tn * TILE)
    run_full(ext, kind, code, p, f"{_case_id(case)} {tm}x{tn} tiles K={p['K']}",
             request.getfixturevalue("contention") if contended else None)


# ---------------------------------------------------------------------------
# the probe operand fills
# ---------------------------------------------------------------------------

PROBE_N = 4096 * 4096
FILL_SIZES = [0, 1, 255, 4096 * 256 + 3, PROBE_N]  # grid is 4096 x 256 threads


@functools.lru_cache(maxsize=None)
def port_fill(kind, seed):
    """The port is position-wise, so every size is a prefix of the largest."""
    return kr.FILL_PORTS[kind](PROBE_N, seed)


def kernel_fill(ext, kind, n, seed):
    t = ext.probe_fill(kind, n, seed)
    torch.cuda.synchronize()
    assert t.shape == (n,) and t.is_cuda
    if kind == "bf16":
        assert t.dtype == torch.bfloat16
        return t.cpu().view(torch.int16).numpy().view(np.uint16)
    assert t.dtype == torch.uint8
    return t.cpu().numpy()


@pytest.mark.parametrize("seed", kr.PROBE_SEEDS)
@pytest.mark.parametrize("n", FILL_SIZES)
@pytest.mark.parametrize("kind", sorted(kr.FILL_PORTS))
def test_probe_fill_equals_port(ext, kind, n, seed):  # noqa: F811
    got = kernel_fill(ext, kind, n, seed)
    want = port_fill(kind, seed)[:n]
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        i = int(bad[0])
        raise AssertionError(
            f"probe_fill({kind!r}, {n}, {seed}): {bad.size} of {n} elements differ "
            f"from the port, first at {i}: got {int(got[i]):#x}, want {int(want[i]):#x}")


@pytest.mark.parametrize("kind", sorted(kr.FILL_PORTS))
def test_probe_fill_properties(ext, kind):  # noqa: F811
    a, b = kr.PROBE_SEEDS
    kr.check_fill_properties(kind, port_fill(kind, a), port_fill(kind, b))
    kr.check_fill_properties(kind, kernel_fill(ext, kind, PROBE_N, a),
                             kernel_fill(ext, kind, PROBE_N, b))


@pytest.mark.parametrize("kind", ["bf16", "e4m3", "e2m1"])
def test_gemm_on_probe_operands(ext, kind):  # noqa: F811
    """The default kernel of each family on the operands its probe times:
    the seed-1 and seed-7 fills, 4096 x 4096 with K = 1024 (2048 for fp4)."""
    M = N = 4096
    K = 2048 if kind == "e2m1" else 1024
    stored = K // 2 if kind == "e2m1" else K
    seed_a, seed_b = kr.PROBE_SEEDS
    A = ext.probe_fill(kind, M * stored, seed_a).view(M, stored)
    Bt = ext.probe_fill(kind, N * stored, seed_b).view(N, stored)
    torch.cuda.synchronize()
    if kind == "bf16":
        a64, b64 = A.cpu().double(), Bt.cpu().double()
    elif kind == "e4m3":
        a64, b64 = (torch.from_numpy(kr.E4M3_LUT[t.cpu().numpy()]) for t in (A, Bt))
    else:
        kr.require_exact("e2m1", K)
        a64, b64 = (torch.from_numpy(kr.E2M1_LUT[kr.unpack_e2m1(t.cpu().numpy())])
                    for t in (A, Bt))
    assert a64.shape == (M, K) and b64.shape == (N, K)
    p = {"A": A, "Bt": Bt, "M": M, "N": N, "K": K, "ref": kr.reference(a64, b64)}
    label = f"probe operands {kind} {M}x{N}x{K}"
    call = functools.partial(launch, ext, kind, 0 if kind == "bf16" else 16, p)
    if kind == "e2m1":
        tgk.run_protocol(call, p, tgk.exact(p), label)
        print(f"ERR/BOUND {label}: exact")
        return
    bound = kr.sum_bound(a64.abs(), b64.abs(), K)
    extra = kr.MX_FP8_TRUNCATION if kind == "e4m3" else 0.0
    worst = tgk.run_protocol(
        call, p,
        lambda C: kr.assert_within_sum_bound(C, p["ref"], None, None, K,
                                             extra_factor=extra, bound=bound),
        label)
    tgk.report(label, worst)
