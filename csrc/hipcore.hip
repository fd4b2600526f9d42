// MI355X (gfx950 / CDNA4) native core for the control plane.
//
// This is the native layer the reference lacks entirely (the
// reference's only GPU interaction is forking nvidia-smi and delegating
// device wiring to nvidia-docker). Components:
//
//   * xGMI / HBM bandwidth probe kernels: vectorized float4 grid-stride
//     copy, local (HBM stream) and peer-to-peer (pull over xGMI). Feeds the
//     scheduler's adjacency matrix (parallel/topology.py).
//   * HBM pattern memory test (hbm_memtest.hip): write / verify / verify_flip
//     over seeded 64-bit words — the burn-in's data-integrity pass.
//   * Per-CU MFMA and LDS check (cu_check.hip): exact tiles in bf16, MX-fp8
//     and MX-fp4 checked on the CU that computed them, its whole LDS
//     pattern-tested, every result tagged with the XCC and CU id.
//   * Per-SIMD vector ALU check (valu_check.hip): integer, fp32, fp64, packed
//     fp16 and transcendental chains with known digests on every SIMD of
//     every CU, every result tagged with the XCC, CU and SIMD id.
//   * Checked GEMM loop (gemm_check.hip): the 256^2 kernels at full size on
//     exactly-summable operands, every result verified on the device with
//     integer row and column checksums per tile.
//   * MFMA warm-up / validation tiles: the exact-f32 16x16x4 MFMA (operand
//     maps documented in the CDNA4 guide) and the bf16 16x16x32 MFMA —
//     clock ramp before measuring, numerics check against torch fp32.
//
// Wave width is 64 on CDNA4; tiles and launch shapes below are sized for
// 64-lane wavefronts and a 256-CU / 8-XCD chip (grids ≫ 256 workgroups).
//
// Build: hipcc --offload-arch=gfx950 (driven by gpu_docker_api_amd/ops/build.py).
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <algorithm>
#include <chrono>
#include <functional>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "hip_host.h"

using hip_host::DeviceBuf;
using hip_host::DeviceScope;
using hip_host::Event;
using hip_host::Stream;

namespace {

// ---------------------------------------------------------------------------
// Copy kernels (bandwidth probe + numerics-testable copy)
// ---------------------------------------------------------------------------

// Grid-stride float4 copy: 16 B per lane per iteration — one coalesced
// 1 KiB transaction per wave64 (CDNA4 guide §2, "Global memory coalescing").
__global__ void copy_f32x4_kernel(const float4* __restrict__ src,
                                  float4* __restrict__ dst, size_t n4) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n4; i += stride) dst[i] = src[i];
}

// 4x-unrolled variant: four independent dwordx4 loads in flight per thread
// before any store — deeper MLP to hide HBM latency on large streams.
__global__ void copy_f32x4_x4_kernel(const float4* __restrict__ src,
                                     float4* __restrict__ dst, size_t n4) {
  size_t stride = (size_t)gridDim.x * blockDim.x;
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  for (; i + 3 * stride < n4; i += 4 * stride) {
    float4 a = src[i];
    float4 b = src[i + stride];
    float4 c = src[i + 2 * stride];
    float4 d = src[i + 3 * stride];
    dst[i] = a;
    dst[i + stride] = b;
    dst[i + 2 * stride] = c;
    dst[i + 3 * stride] = d;
  }
  for (; i < n4; i += stride) dst[i] = src[i];
}

// Tail-safe scalar copy for non-multiple-of-4 sizes.
__global__ void copy_f32_tail_kernel(const float* __restrict__ src,
                                     float* __restrict__ dst, size_t n,
                                     size_t offset) {
  size_t i = offset + blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

void launch_copy_f32(const float* src, float* dst, size_t n, hipStream_t stream) {
  size_t n4 = n / 4;
  constexpr int kBlock = 256;
  if (n4 > 0) {
    // ≫ 256 workgroups to fill 256 CUs across 8 XCDs; cap to keep launch sane
    int grid = (int)std::min<size_t>((n4 + kBlock - 1) / kBlock, 32768);
    if (n4 >= (size_t)4 * grid * kBlock) {
      hipLaunchKernelGGL(copy_f32x4_x4_kernel, dim3(grid), dim3(kBlock), 0,
                         stream, reinterpret_cast<const float4*>(src),
                         reinterpret_cast<float4*>(dst), n4);
    } else {
      hipLaunchKernelGGL(copy_f32x4_kernel, dim3(grid), dim3(kBlock), 0, stream,
                         reinterpret_cast<const float4*>(src),
                         reinterpret_cast<float4*>(dst), n4);
    }
  }
  size_t tail = n - n4 * 4;
  if (tail > 0) {
    hipLaunchKernelGGL(copy_f32_tail_kernel, dim3(1), dim3(kBlock), 0, stream,
                       src, dst, n, n4 * 4);
  }
}

// ---------------------------------------------------------------------------
// MFMA tiles
// ---------------------------------------------------------------------------

using f32x4 = __attribute__((ext_vector_type(4))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;

// Exact-f32 MFMA 16x16x4 (v_mfma_f32_16x16x4_f32). Operand map is documented
// in the CDNA4 guide §3: lane l supplies A[l&15][l>>4] and B[l>>4][l&15]
// (one f32 each); C/D: col = lane&15, row = (lane>>4)*4 + reg.
// K is tiled in steps of 4, accumulating in the same f32x4 (guide §3,
// "K-loop accumulator recipe"). One wave per 16x16 C tile.
__global__ void mfma_f32_16x16_kernel(const float* __restrict__ A,
                                      const float* __restrict__ B,
                                      float* __restrict__ C, int M, int N,
                                      int K) {
  int lane = threadIdx.x & 63;
  int wave = (blockIdx.x * (blockDim.x >> 6)) + (threadIdx.x >> 6);
  int tiles_n = N / 16;
  int tm = (wave / tiles_n) * 16;
  int tn = (wave % tiles_n) * 16;
  if (tm >= M) return;

  int row = lane & 15;
  int kk = lane >> 4;  // 0..3
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < K; k0 += 4) {
    float a = A[(tm + row) * K + (k0 + kk)];
    float b = B[(k0 + kk) * N + (tn + row)];
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
  int crow = (lane >> 4) * 4;
  int ccol = lane & 15;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    C[(tm + crow + r) * N + (tn + ccol)] = acc[r];
  }
}

// bf16 MFMA 16x16x32 (gfx950 2xK form). Each lane holds 8 bf16 of A and B.
// Operand map: A[l&15][(l>>4)*8 + j], B[(l>>4)*8 + j][l&15]; C/D map as
// above (dtype-independent on gfx950, guide §3).
__global__ void mfma_bf16_16x16_kernel(const __hip_bfloat16* __restrict__ A,
                                       const __hip_bfloat16* __restrict__ B,
                                       float* __restrict__ C, int M, int N,
                                       int K) {
  int lane = threadIdx.x & 63;
  int wave = (blockIdx.x * (blockDim.x >> 6)) + (threadIdx.x >> 6);
  int tiles_n = N / 16;
  int tm = (wave / tiles_n) * 16;
  int tn = (wave % tiles_n) * 16;
  if (tm >= M) return;

  int row = lane & 15;
  int kbase = (lane >> 4) * 8;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < K; k0 += 32) {
    bf16x8 a_frag, b_frag;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      a_frag[j] = *reinterpret_cast<const __bf16*>(&A[(tm + row) * K + k0 + kbase + j]);
      b_frag[j] = *reinterpret_cast<const __bf16*>(&B[(k0 + kbase + j) * N + tn + row]);
    }
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_frag, b_frag, acc, 0, 0, 0);
  }
  int crow = (lane >> 4) * 4;
  int ccol = lane & 15;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    C[(tm + crow + r) * N + (tn + ccol)] = acc[r];
  }
}

// MFMA clock-ramp warm-up: dependent-chain f32 MFMA spin, one wave per block.
__global__ void mfma_warmup_kernel(float* __restrict__ sink, int iters) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  float a = (threadIdx.x & 15) * 0.001f + 1.0f;
  float b = (threadIdx.x >> 4) * 0.002f + 1.0f;
  for (int i = 0; i < iters; ++i) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
  if (sink != nullptr && threadIdx.x == 0 && blockIdx.x == 0) sink[0] = acc[0];
}

}  // namespace  (reopened below — gemm lives in its own TU-style include)

#include "gemm_bf16.hip"
#include "gemm_bf16_8phase.hip"
#include "gemm_fp8_mx.hip"
#include "hbm_memtest.hip"
#include "cu_check.hip"
#include "valu_check.hip"

namespace {

// LCG-hash fill: pseudorandom bf16 in [-1, 1) — zero-filled operands
// overstate GEMM throughput on this chip (guide §5.4 rule 25).
__global__ void fill_bf16_hash_kernel(__hip_bfloat16* p, size_t n, unsigned seed) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    unsigned h = (unsigned)i * 2654435761u + seed;
    h ^= h >> 15;
    h *= 2246822519u;
    h ^= h >> 13;
    float v = ((h & 0xFFFFFF) / 8388608.0f) - 1.0f;  // [-1, 1)
    // the bf16 rounding takes v >= 1 - 2^-9 up to 1.0 (one value in 1024):
    // hold those at the largest bf16 below 1 so the fill stays in [-1, 1)
    p[i] = __hip_bfloat16(fminf(v, 0.99609375f));
  }
}

// ---------------------------------------------------------------------------
// Host-side probe machinery
// ---------------------------------------------------------------------------

// Every probe below makes its device current through a DeviceScope, so the
// calling thread leaves on the device it came in on.

double time_kernel_ms(int device, std::function<void(hipStream_t)> body,
                      int iters) {
  DeviceScope scope(device);
  Stream stream;
  Event t0, t1;
  body(stream.s);  // one warm launch
  stream.synchronize();
  t0.record(stream);
  for (int i = 0; i < iters; ++i) body(stream.s);
  t1.record(stream);
  t1.synchronize();
  return Event::elapsed_ms(t0, t1) / iters;
}

void mfma_warmup(int device, int spins) {
  DeviceScope scope(device);
  hipLaunchKernelGGL(mfma_warmup_kernel, dim3(2048), dim3(256), 0, 0, nullptr,
                     spins);
  HIP_CHECK(hipDeviceSynchronize());
}

// The `mib` MiB of floats a bandwidth probe moves.
size_t probe_floats(int mib) { return (size_t)mib * 1024 * 1024 / sizeof(float); }

// A probe's source buffer: `n` floats on `device`, every byte set to 1.
DeviceBuf<float> probe_source(int device, size_t n) {
  DeviceBuf<float> src(device, n);
  DeviceScope scope(device);
  HIP_CHECK(hipMemset(src.ptr, 1, n * sizeof(float)));
  return src;
}

// Enables peer access from `dst` to `src` and says whether a kernel on `dst`
// may read `src`'s memory: false when the devices are not peers or when
// enabling fails, and then the pair is timed on the copy engine.
bool enable_peer_read(int dst, int src) {
  if (dst == src) return true;
  int can = 0;
  HIP_CHECK(hipDeviceCanAccessPeer(&can, dst, src));
  if (!can) return false;
  DeviceScope scope(dst);
  hipError_t e = hipDeviceEnablePeerAccess(src, 0);
  (void)hipGetLastError();  // "already enabled" is sticky otherwise
  return e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled;
}

// GB/s of `n` floats from `src` on src_dev to `dst` on dst_dev, timed on
// dst_dev. kernel_path: the float4 copy kernel; on one device that is the HBM
// stream and read + write bytes count, across devices it pulls over xGMI
// (per-link peak ≈153 GB/s, 7 links/GPU on an 8-GPU node) and the bytes count
// once. Otherwise hipMemcpyPeerAsync, the SDMA/blit path (on one device that
// is the plain device-to-device hipMemcpyAsync).
double time_pair_gbps(int src_dev, const float* src, int dst_dev, float* dst,
                      size_t n, bool kernel_path, int iters) {
  const size_t bytes = n * sizeof(float);
  std::function<void(hipStream_t)> body;
  if (kernel_path) {
    body = [=](hipStream_t s) { launch_copy_f32(src, dst, n, s); };
  } else {
    body = [=](hipStream_t s) {
      HIP_CHECK(hipMemcpyPeerAsync(dst, dst_dev, src, src_dev, bytes, s));
    };
  }
  double ms = time_kernel_ms(dst_dev, body, iters);
  return (src_dev == dst_dev ? 2.0 : 1.0) * bytes / (ms * 1e6);
}

// One pair with buffers of its own. warm: MFMA clock ramp on dst_dev first.
double pair_bandwidth_gbps(int src_dev, int dst_dev, int mib, int iters,
                           bool kernel_path, bool warm) {
  const size_t n = probe_floats(mib);
  if (warm) mfma_warmup(dst_dev, 2000);
  DeviceBuf<float> src = probe_source(src_dev, n), dst(dst_dev, n);
  return time_pair_gbps(src_dev, src.ptr, dst_dev, dst.ptr, n, kernel_path, iters);
}

// Local HBM stream bandwidth: copy of `mib` MiB on one device; GB/s counts
// read + write bytes (achievable ceiling ≈6.3 TB/s on MI355X).
double stream_bandwidth_gbps(int device, int mib, int iters) {
  return pair_bandwidth_gbps(device, device, mib, iters, true, true);
}

// Reference point: the SDMA/blit path on one device.
double memcpy_bandwidth_gbps(int device, int mib, int iters) {
  return pair_bandwidth_gbps(device, device, mib, iters, false, false);
}

// Peer bandwidth: dst-device kernel pulls from src-device memory, or the copy
// engine where kernel p2p access is not available.
double p2p_bandwidth_gbps(int src_dev, int dst_dev, int mib, int iters) {
  return pair_bandwidth_gbps(src_dev, dst_dev, mib, iters,
                             enable_peer_read(dst_dev, src_dev), true);
}

// Full pairwise matrix in one call: per-device src/dst buffers allocated
// ONCE, peer access enabled once, then every ordered pair timed. On an
// 8-GPU node this is ~56 measurements; per-pair re-allocation would push
// daemon startup to minutes.
std::vector<std::vector<double>> p2p_matrix(int mib, int iters) {
  int n = 0;
  HIP_CHECK(hipGetDeviceCount(&n));
  std::vector<std::vector<double>> out(n, std::vector<double>(n, 0.0));
  const size_t count = probe_floats(mib);

  std::vector<DeviceBuf<float>> src, dst;
  // readable[d][s]: a kernel on d may read s's memory
  std::vector<std::vector<bool>> readable(n, std::vector<bool>(n, false));
  for (int i = 0; i < n; ++i) {
    src.push_back(probe_source(i, count));
    dst.emplace_back(i, count);
    mfma_warmup(i, 2000);
    for (int j = 0; j < n; ++j) readable[i][j] = enable_peer_read(i, j);
  }
  for (int d = 0; d < n; ++d)
    for (int s = 0; s < n; ++s)
      out[s][d] = time_pair_gbps(s, src[s].ptr, d, dst[d].ptr, count,
                                 readable[d][s], iters);
  return out;
}

// ---------------------------------------------------------------------------
// Torch bindings
// ---------------------------------------------------------------------------

// The GEMM kernels stage with 16-byte global_load_lds (and the dwordx4
// epilogue stores 16 bytes), the copy kernels reinterpret as float4: a
// contiguous view with a storage offset that is not a multiple of 16 bytes
// must be rejected before any launch.
void check_aligned16(const torch::Tensor& t, const char* name) {
  TORCH_CHECK((reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0, name,
              ": data pointer must be 16-byte aligned");
}

// Resolve the optional `out` argument of the GEMM bindings: allocate when
// absent, otherwise require an fp32 contiguous [M, N] tensor on A's device.
torch::Tensor resolve_out(const c10::optional<torch::Tensor>& out, int64_t M,
                          int64_t N, const torch::Tensor& A) {
  if (!out.has_value())
    return torch::empty({M, N}, A.options().dtype(torch::kFloat32));
  const torch::Tensor& C = *out;
  TORCH_CHECK(C.is_cuda() && C.device() == A.device(),
              "out: must be on the same device as A");
  TORCH_CHECK(C.scalar_type() == torch::kFloat32, "out: must be float32");
  TORCH_CHECK(C.dim() == 2 && C.size(0) == M && C.size(1) == N,
              "out: must have shape [M, N] = [", M, ", ", N, "]");
  TORCH_CHECK(C.is_contiguous(), "out: must be contiguous");
  return C;
}

// What one GEMM / MFMA binding accepts.
struct GemmSpec {
  torch::ScalarType dtype;
  const char* dtype_msg;
  bool b_is_nk;            // second operand is Bt [N][K]; otherwise B [K][N]
  int tile;                // M and N: multiples of it, at least it
  int k_mult, k_min;
  const char* extent_msg;  // names tile, k_mult and k_min
  bool packed_fp4 = false;  // two elements per stored byte; K is an argument
};

// The validated operands of one call: extents, contiguous A and B, the
// resolved C, and torch's current stream.
struct GemmOperands {
  int M, N, K;
  torch::Tensor A, B, C;
  hipStream_t stream;
  template <typename T>
  const T* a() const { return static_cast<const T*>(A.data_ptr()); }
  template <typename T>
  const T* b() const { return static_cast<const T*>(B.data_ptr()); }
  float* c() const { return C.data_ptr<float>(); }
};

// The one operand check of the six GEMM / MFMA bindings, in this order:
// placement and rank, dtype, inner extent, tile extents, `select(K)` (the
// binding's variant lookup, may be empty), 16-byte alignment, `out`.
// packed_k: the K argument of a packed_fp4 binding, not read otherwise.
GemmOperands gemm_operands(torch::Tensor A, torch::Tensor B,
                           const c10::optional<torch::Tensor>& out,
                           const GemmSpec& spec,
                           const std::function<void(int)>& select = nullptr,
                           int packed_k = 0) {
  const char* bname = spec.b_is_nk ? "Bt" : "B";
  TORCH_CHECK(A.is_cuda() && B.is_cuda(), "GPU tensors required");
  TORCH_CHECK(A.device() == B.device(), "operands must share a device");
  TORCH_CHECK(A.dim() == 2 && B.dim() == 2, "A and ", bname, " must be 2-D");
  TORCH_CHECK(A.scalar_type() == spec.dtype && B.scalar_type() == spec.dtype,
              spec.dtype_msg);
  GemmOperands g;
  g.A = A.contiguous();
  g.B = B.contiguous();
  g.M = g.A.size(0);
  g.N = g.B.size(spec.b_is_nk ? 0 : 1);
  const int64_t a_cols = g.A.size(1), b_k = g.B.size(spec.b_is_nk ? 1 : 0);
  if (spec.packed_fp4) {
    g.K = packed_k;
    TORCH_CHECK(a_cols * 2 == g.K && b_k * 2 == g.K,
                "K must equal 2 x packed byte columns");
  } else {
    g.K = a_cols;
    TORCH_CHECK(b_k == g.K, spec.b_is_nk ? "Bt must be [N][K]" : "shape mismatch");
  }
  TORCH_CHECK(g.M >= spec.tile && g.N >= spec.tile && g.M % spec.tile == 0 &&
                  g.N % spec.tile == 0 && g.K % spec.k_mult == 0 &&
                  g.K >= spec.k_min,
              spec.extent_msg);
  if (select) select(g.K);
  check_aligned16(g.A, "A");
  check_aligned16(g.B, bname);
  g.C = resolve_out(out, g.M, g.N, g.A);
  check_aligned16(g.C, "out");
  g.stream = at::hip::getCurrentHIPStream().stream();
  return g;
}

// One wave per 16x16 tile of C, four waves per block.
template <typename T>
torch::Tensor launch_mfma_16x16(void (*kernel)(const T*, const T*, float*, int,
                                               int, int),
                                const GemmOperands& g) {
  constexpr int kWavesPerBlock = 4;  // 256 threads
  int waves = (g.M / 16) * (g.N / 16);
  int grid = (waves + kWavesPerBlock - 1) / kWavesPerBlock;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kWavesPerBlock * 64), 0, g.stream,
                     g.a<T>(), g.b<T>(), g.c(), g.M, g.N, g.K);
  return g.C;
}

void copy_f32(torch::Tensor dst, torch::Tensor src) {
  TORCH_CHECK(src.is_cuda() && dst.is_cuda(), "tensors must be on GPU");
  TORCH_CHECK(src.scalar_type() == torch::kFloat32 &&
                  dst.scalar_type() == torch::kFloat32,
              "f32 only");
  TORCH_CHECK(src.is_contiguous() && dst.is_contiguous(), "contiguous only");
  TORCH_CHECK(src.numel() == dst.numel(), "size mismatch");
  check_aligned16(src, "src");
  check_aligned16(dst, "dst");
  auto stream = at::hip::getCurrentHIPStream();
  launch_copy_f32(src.data_ptr<float>(), dst.data_ptr<float>(), src.numel(),
                  stream.stream());
}

torch::Tensor mfma_f32_matmul(torch::Tensor A, torch::Tensor B,
                              c10::optional<torch::Tensor> out) {
  return launch_mfma_16x16<float>(
      mfma_f32_16x16_kernel,
      gemm_operands(A, B, out,
                    {torch::kFloat32, "f32 only", false, 16, 4, 4,
                     "M,N multiples of 16; K multiple of 4, >= 4"}));
}

torch::Tensor mfma_bf16_matmul(torch::Tensor A, torch::Tensor B,
                               c10::optional<torch::Tensor> out) {
  return launch_mfma_16x16<__hip_bfloat16>(
      mfma_bf16_16x16_kernel,
      gemm_operands(A, B, out,
                    {torch::kBFloat16, "bf16 only", false, 16, 32, 32,
                     "M,N multiples of 16; K multiple of 32, >= 32"}));
}

// BK of the 128^2 kernel: 32 or 64; 0 picks the widest K-step that divides K
// (the binding's default). Validated once, before any launch.
int resolve_bf16_bk(int bk, int K) {
  if (bk == 0) bk = (K % 64 == 0) ? 64 : 32;
  TORCH_CHECK(bk == 32 || bk == 64, "bk must be 0 (auto), 32 or 64");
  TORCH_CHECK(K % bk == 0, "K must be a multiple of bk");
  return bk;
}

// The one BK -> instantiation table of the 128^2 kernel, shared by the
// tensor binding and gemm_bf16_tflops. bk comes from resolve_bf16_bk.
void launch_bf16_tile(int bk, int swizzle, dim3 grid, hipStream_t s,
                      const __hip_bfloat16* A, const __hip_bfloat16* Bt,
                      float* C, int M, int N, int K) {
  if (bk == 32) {
    hipLaunchKernelGGL(gemm_bf16::gemm_bf16_tile_kernel<32>, grid, dim3(256),
                       0, s, A, Bt, C, M, N, K, swizzle);
  } else {
    hipLaunchKernelGGL(gemm_bf16::gemm_bf16_tile_kernel<64>, grid, dim3(256),
                       0, s, A, Bt, C, M, N, K, swizzle);
  }
}

torch::Tensor gemm_bf16_bt(torch::Tensor A, torch::Tensor Bt, int swizzle,
                           int bk, c10::optional<torch::Tensor> out) {
  auto g = gemm_operands(
      A, Bt, out,
      {torch::kBFloat16, "bf16 only", true, 128, 32, 32,
       "M,N multiples of 128; K multiple of 32, >= 32"},
      [&](int K) {
        TORCH_CHECK(swizzle == 0 || swizzle == 1, "swizzle must be 0 or 1");
        bk = resolve_bf16_bk(bk, K);
      });
  launch_bf16_tile(bk, swizzle, dim3((g.M / 128) * (g.N / 128)), g.stream,
                   g.a<__hip_bfloat16>(), g.b<__hip_bfloat16>(), g.c(), g.M, g.N,
                   g.K);
  return g.C;
}

// Enqueues one size^3 GEMM on a stream: (stream, A, Bt, C).
template <typename T>
using GemmLaunch = std::function<void(hipStream_t, const T*, const T*, float*)>;

// The one launch of a probe operand fill, shared by time_gemm_tflops and the
// probe_fill binding so the fills that are tested are the fills that are timed.
constexpr unsigned kProbeSeedA = 1u, kProbeSeedBt = 7u;

template <typename T>
void launch_probe_fill(void (*fill)(T*, size_t, unsigned), T* p, size_t n,
                       unsigned seed, hipStream_t s) {
  hipLaunchKernelGGL(fill, dim3(4096), dim3(256), 0, s, p, n, seed);
}

// One size^3 throughput measurement, shared by every *_tflops / _ab driver:
// MFMA warm-up, three owned device buffers (released on any exit), hash-filled
// operands, then each of `launches` timed once per round, round-robin.
// operand_elems: stored elements per operand (size^2; halved for packed fp4).
// Returns TF (2*size^3 flop) as [round][launch].
template <typename T>
std::vector<std::vector<double>> time_gemm_tflops(
    int device, int size, int iters, int rounds, size_t operand_elems,
    void (*fill)(T*, size_t, unsigned), const std::vector<GemmLaunch<T>>& launches) {
  DeviceScope scope(device);
  mfma_warmup(device, 20000);
  DeviceBuf<T> A(device, operand_elems), Bt(device, operand_elems);
  DeviceBuf<float> C(device, (size_t)size * size);
  launch_probe_fill(fill, A.ptr, operand_elems, kProbeSeedA, 0);
  launch_probe_fill(fill, Bt.ptr, operand_elems, kProbeSeedBt, 0);
  HIP_CHECK(hipDeviceSynchronize());
  std::vector<std::vector<double>> tf(rounds);
  for (auto& round : tf) {
    for (const auto& launch : launches) {
      double ms = time_kernel_ms(
          device, [&](hipStream_t s) { launch(s, A.ptr, Bt.ptr, C.ptr); }, iters);
      round.push_back(2.0 * size * (double)size * size / (ms * 1e9));
    }
  }
  return tf;
}

// Dense bf16 throughput on one device (the health-check burn-in number).
double gemm_bf16_tflops(int device, int size, int iters, int swizzle, int bk) {
  if (bk != 32) bk = 64;  // historical: anything but 32 times the BK=64 kernel
  TORCH_CHECK(size >= 128 && size % 128 == 0, "size must be a multiple of 128");
  bk = resolve_bf16_bk(bk, size);
  int grid = (size / 128) * (size / 128);
  return time_gemm_tflops<__hip_bfloat16>(
      device, size, iters, 1, (size_t)size * size, fill_bf16_hash_kernel,
      {[=](hipStream_t s, const __hip_bfloat16* A, const __hip_bfloat16* Bt,
           float* C) {
        launch_bf16_tile(bk, swizzle, dim3(grid), s, A, Bt, C, size, size, size);
      }})[0][0];
}

// ---------------------------------------------------------------------------
// 256^2 8-phase family: one {code, kernel} table per operand format, shared by
// the tensor bindings and the timing drivers so the numerics tests cover
// exactly the kernels that are timed. Tables are in ascending code order; the
// "known codes" text of the errors is generated from them.
// ---------------------------------------------------------------------------

template <typename T>
using Gemm256Kernel = void (*)(const T*, const T*, float*, int, int, int);

template <typename T>
struct Gemm256Variant {
  int code;
  Gemm256Kernel<T> kernel;
};

// bit0 = XCD remap; schedules are described in gemm_bf16_8phase.hip.
// Template axes: <XCD, SCHED, SWZV>.
constexpr Gemm256Variant<__hip_bfloat16> kBf16Variants8ph[] = {
    {0, gemm_bf16_8ph::gemm_bf16_8phase_kernel<0, gemm_bf16_8ph::ROLLED>},
    {1, gemm_bf16_8ph::gemm_bf16_8phase_kernel<1, gemm_bf16_8ph::ROLLED>},
    {2, gemm_bf16_8ph::gemm_bf16_8phase_kernel<0, gemm_bf16_8ph::PHASE_AHEAD>},
    {3, gemm_bf16_8ph::gemm_bf16_8phase_kernel<1, gemm_bf16_8ph::PHASE_AHEAD>},
    {4, gemm_bf16_8ph::gemm_bf16_8phase_kernel<0, gemm_bf16_8ph::UNROLLED_FENCED>},
    {5, gemm_bf16_8ph::gemm_bf16_8phase_kernel<1, gemm_bf16_8ph::UNROLLED_FENCED>},
    {6, gemm_bf16_8ph::gemm_bf16_8phase_kernel<0, gemm_bf16_8ph::UNROLLED>},
    {7, gemm_bf16_8ph::gemm_bf16_8phase_kernel<1, gemm_bf16_8ph::UNROLLED>},
    // 10, 11: aliases of 6, 7, the kernels these codes always ran (8 and 9,
    // the other two such codes, are rejected; gemm_bf16_8phase.hip)
    {10, gemm_bf16_8ph::gemm_bf16_8phase_kernel<0, gemm_bf16_8ph::UNROLLED>},
    {11, gemm_bf16_8ph::gemm_bf16_8phase_kernel<1, gemm_bf16_8ph::UNROLLED>},
    {12, gemm_bf16_8ph::gemm_bf16_8phase_kernel<0, gemm_bf16_8ph::ROLLED, 1>},
};

// Template axes: <FMT, SWZV, EPI, MP23>.
constexpr Gemm256Variant<unsigned char> kFp8MxShapes[] = {
    // default: row-bit-3 swizzle (conflict-free 2-chunk reads, +11%)
    {16, gemm_fp8_mx::gemm_fp8_mx_kernel<0, 1, 0, 0>},
    // legacy row&7-only swizzle (A/B reference)
    {17, gemm_fp8_mx::gemm_fp8_mx_kernel<0, 0, 0, 0>},
    // + quad-transpose dwordx4 epilogue
    {18, gemm_fp8_mx::gemm_fp8_mx_kernel<0, 1, 1, 0>},
    // merged phases 2+3
    {20, gemm_fp8_mx::gemm_fp8_mx_kernel<0, 1, 0, 1>},
    // 32x32x64 instruction
    {32, gemm_fp8_mx::gemm_mx32_kernel<0, 0>},
};

// Code 16 (the default) and 19 are the same instantiation.
constexpr Gemm256Variant<unsigned char> kFp4MxShapes[] = {
    // default: merged phases 2+3 (+1-2% measured both orders)
    {16, gemm_fp8_mx::gemm_fp8_mx_kernel<4, 0, 0, 1>},
    // 16x16 with the row-bit-3 swizzle
    {17, gemm_fp8_mx::gemm_fp8_mx_kernel<4, 1, 0, 0>},
    // + quad-transpose dwordx4 epilogue
    {18, gemm_fp8_mx::gemm_fp8_mx_kernel<4, 0, 1, 0>},
    {19, gemm_fp8_mx::gemm_fp8_mx_kernel<4, 0, 0, 1>},
    // unmerged legacy (A/B reference)
    {21, gemm_fp8_mx::gemm_fp8_mx_kernel<4, 0, 0, 0>},
    // 32x32x64 instruction
    {32, gemm_fp8_mx::gemm_mx32_kernel<4, 0>},
};

// The kernel for `code`, or an error naming `what`, the code and the known ones.
template <typename T, size_t N>
Gemm256Kernel<T> find_variant(const Gemm256Variant<T> (&table)[N], int code,
                              const char* what) {
  for (const auto& v : table)
    if (v.code == code) return v.kernel;
  std::string known;
  for (const auto& v : table)
    known += (known.empty() ? "" : ", ") + std::to_string(v.code);
  TORCH_CHECK(false, "unknown ", what, " ", code, " (", known, ")");
  return nullptr;  // not reached
}

template <typename T>
void launch_256(Gemm256Kernel<T> kernel, hipStream_t s, const T* A, const T* Bt,
                float* C, int M, int N, int K) {
  hipLaunchKernelGGL(kernel, dim3((M / 256) * (N / 256)), dim3(512), 0, s, A, Bt,
                     C, M, N, K);
}

// size^3 throughput of each of `kernels`, [round][kernel].
template <typename T>
std::vector<std::vector<double>> time_256_tflops(
    int device, int size, int iters, int rounds, size_t operand_elems,
    void (*fill)(T*, size_t, unsigned),
    const std::vector<Gemm256Kernel<T>>& kernels) {
  std::vector<GemmLaunch<T>> launches;
  for (auto kernel : kernels)
    launches.push_back([=](hipStream_t s, const T* A, const T* Bt, float* C) {
      launch_256(kernel, s, A, Bt, C, size, size, size);
    });
  return time_gemm_tflops<T>(device, size, iters, rounds, operand_elems, fill,
                             launches);
}

// The tensor binding of one 256^2 format: operands checked against `spec`,
// `code` looked up in `table`, one launch on the current stream.
template <typename T, size_t NV>
torch::Tensor gemm_256_bt(torch::Tensor A, torch::Tensor Bt,
                          const c10::optional<torch::Tensor>& out,
                          const GemmSpec& spec,
                          const Gemm256Variant<T> (&table)[NV], int code,
                          const char* what, int packed_k = 0) {
  Gemm256Kernel<T> kernel = nullptr;
  const GemmOperands g = gemm_operands(
      A, Bt, out, spec, [&](int) { kernel = find_variant(table, code, what); },
      packed_k);
  launch_256(kernel, g.stream, g.a<T>(), g.b<T>(), g.c(), g.M, g.N, g.K);
  return g.C;
}

torch::Tensor gemm_bf16_8ph_bt(torch::Tensor A, torch::Tensor Bt, int variant,
                               c10::optional<torch::Tensor> out) {
  return gemm_256_bt(A, Bt, out,
                     {torch::kBFloat16, "bf16 only", true, 256, 64, 192,
                      "M,N multiples of 256; K multiple of 64, >= 192"},
                     kBf16Variants8ph, variant, "8-phase variant");
}

double gemm_bf16_8ph_tflops(int device, int size, int iters, int variant) {
  auto kernel = find_variant(kBf16Variants8ph, variant, "8-phase variant");
  TORCH_CHECK(size >= 256 && size % 256 == 0, "size must be a multiple of 256");
  return time_256_tflops<__hip_bfloat16>(device, size, iters, 1,
                                         (size_t)size * size,
                                         fill_bf16_hash_kernel, {kernel})[0][0];
}

// Within-probe interleaved A/B over the template variants (guide §5.4
// rules 9/24: run-to-run noise ~±3%, so variants must be interleaved in one
// process). Returns {variant: [tflops per round]}.
py::dict gemm_bf16_8ph_ab(int device, int size, int iters, int rounds,
                          std::vector<int> variants) {
  std::vector<Gemm256Kernel<__hip_bfloat16>> kernels;
  for (int v : variants)
    kernels.push_back(find_variant(kBf16Variants8ph, v, "8-phase variant"));
  TORCH_CHECK(size >= 256 && size % 256 == 0, "size must be a multiple of 256");
  auto tf = time_256_tflops<__hip_bfloat16>(device, size, iters, rounds,
                                            (size_t)size * size,
                                            fill_bf16_hash_kernel, kernels);
  std::map<int, std::vector<double>> out;
  for (const auto& round : tf)
    for (size_t i = 0; i < variants.size(); ++i)
      out[variants[i]].push_back(round[i]);
  py::dict d;
  for (auto& kv : out) d[py::int_(kv.first)] = kv.second;
  return d;
}

torch::Tensor gemm_fp8_mx_bt(torch::Tensor A, torch::Tensor Bt, int shape,
                             c10::optional<torch::Tensor> out) {
  return gemm_256_bt(
      A, Bt, out,
      {torch::kUInt8, "raw e4m3 bytes expected (uint8 view of float8_e4m3fn)",
       true, 256, 128, 256, "M,N multiples of 256; K multiple of 128, >= 256"},
      kFp8MxShapes, shape, "fp8 MX shape code");
}

torch::Tensor gemm_fp4_mx_bt(torch::Tensor A, torch::Tensor Bt, int K, int shape,
                             c10::optional<torch::Tensor> out) {
  // A [M][K/2], Bt [N][K/2]: e2m1 nibble-packed (low nibble = even k)
  return gemm_256_bt(
      A, Bt, out,
      {torch::kUInt8, "packed e2m1 bytes expected", true, 256, 256, 512,
       "M,N multiples of 256; K multiple of 256, >= 512", true},
      kFp4MxShapes, shape, "fp4 MX shape code", K);
}

double gemm_fp8_mx_tflops(int device, int size, int iters, int shape) {
  auto kernel = find_variant(kFp8MxShapes, shape, "fp8 MX shape code");
  TORCH_CHECK(size >= 256 && size % 256 == 0, "size must be a multiple of 256");
  return time_256_tflops<unsigned char>(device, size, iters, 1,
                                        (size_t)size * size,
                                        gemm_fp8_mx::fill_e4m3_hash_kernel,
                                        {kernel})[0][0];
}

double gemm_fp4_mx_tflops(int device, int size, int iters, int shape) {
  auto kernel = find_variant(kFp4MxShapes, shape, "fp4 MX shape code");
  TORCH_CHECK(size >= 512 && size % 256 == 0,
              "size must be a multiple of 256, >= 512");
  return time_256_tflops<unsigned char>(device, size, iters, 1,
                                        (size_t)size * size / 2,  // nibble-packed
                                        gemm_fp8_mx::fill_e2m1_hash_kernel,
                                        {kernel})[0][0];
}

// The operand fill of the *_tflops probes as a tensor of `n` stored elements
// on the current device: "bf16" -> bfloat16, "e4m3" -> uint8 codes, "e2m1" ->
// uint8 nibble pairs. Seeds 1 and 7 give the probes' A and Bt.
torch::Tensor probe_fill(const std::string& kind, int64_t n, unsigned seed) {
  TORCH_CHECK(n >= 0, "n must not be negative");
  auto opts = torch::TensorOptions().device(torch::kCUDA);
  auto stream = at::hip::getCurrentHIPStream();
  if (kind == "bf16") {
    auto t = torch::empty({n}, opts.dtype(torch::kBFloat16));
    launch_probe_fill(fill_bf16_hash_kernel,
                      reinterpret_cast<__hip_bfloat16*>(t.data_ptr()), (size_t)n,
                      seed, stream.stream());
    return t;
  }
  TORCH_CHECK(kind == "e4m3" || kind == "e2m1", "unknown fill kind ", kind,
              " (bf16, e4m3, e2m1)");
  auto t = torch::empty({n}, opts.dtype(torch::kUInt8));
  launch_probe_fill(kind == "e4m3" ? gemm_fp8_mx::fill_e4m3_hash_kernel
                                   : gemm_fp8_mx::fill_e2m1_hash_kernel,
                    reinterpret_cast<unsigned char*>(t.data_ptr()), (size_t)n, seed,
                    stream.stream());
  return t;
}

int device_count() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

py::dict device_info(int device) {
  hipDeviceProp_t prop;
  HIP_CHECK(hipGetDeviceProperties(&prop, device));
  py::dict d;
  d["name"] = std::string(prop.name);
  d["gcnArchName"] = std::string(prop.gcnArchName);
  d["totalGlobalMem"] = (long long)prop.totalGlobalMem;
  d["multiProcessorCount"] = prop.multiProcessorCount;
  d["sharedMemPerBlockOptin"] = (long long)prop.sharedMemPerBlockOptin;
  d["pciBusID"] = prop.pciBusID;
  d["pciDomainID"] = prop.pciDomainID;
  d["pciDeviceID"] = prop.pciDeviceID;
  size_t free_b = 0, total_b = 0;
  DeviceScope scope(device);
  HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
  d["freeMem"] = (long long)free_b;
  return d;
}

}  // namespace

#include "gemm_check.hip"

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "MI355X native core: bandwidth probes + MFMA tiles";
  m.def("probe_fill", &probe_fill, py::arg("kind"), py::arg("n"), py::arg("seed"));
  m.def("device_count", &device_count);
  m.def("device_info", &device_info, py::arg("device"));
  m.def("copy_f32", &copy_f32, py::arg("dst"), py::arg("src"));
  m.def("mfma_f32_matmul", &mfma_f32_matmul, py::arg("A"), py::arg("B"),
        py::arg("out") = py::none());
  m.def("mfma_bf16_matmul", &mfma_bf16_matmul, py::arg("A"), py::arg("B"),
        py::arg("out") = py::none());
  m.def("mfma_warmup", &mfma_warmup, py::arg("device") = 0,
        py::arg("spins") = 20000);
  m.def("gemm_bf16_bt", &gemm_bf16_bt, py::arg("A"), py::arg("Bt"),
        py::arg("swizzle") = 0, py::arg("bk") = 0, py::arg("out") = py::none());
  m.def("gemm_bf16_8ph", &gemm_bf16_8ph_bt, py::arg("A"), py::arg("Bt"),
        py::arg("variant") = 0, py::arg("out") = py::none());
  m.def("gemm_fp8_mx", &gemm_fp8_mx_bt, py::arg("A"), py::arg("Bt"),
        py::arg("shape") = 16, py::arg("out") = py::none());
  m.def("gemm_fp4_mx", &gemm_fp4_mx_bt, py::arg("A"), py::arg("Bt"), py::arg("K"),
        py::arg("shape") = 16, py::arg("out") = py::none());
  m.def("gemm_fp4_mx_tflops", &gemm_fp4_mx_tflops, py::arg("device") = 0,
        py::arg("size") = 4096, py::arg("iters") = 10, py::arg("shape") = 16,
        py::call_guard<py::gil_scoped_release>());
  m.def("gemm_fp8_mx_tflops", &gemm_fp8_mx_tflops, py::arg("device") = 0,
        py::arg("size") = 4096, py::arg("iters") = 10, py::arg("shape") = 16,
        py::call_guard<py::gil_scoped_release>());
  m.def("gemm_bf16_8ph_ab", &gemm_bf16_8ph_ab, py::arg("device") = 0,
        py::arg("size") = 4096, py::arg("iters") = 4, py::arg("rounds") = 3,
        py::arg("variants") = std::vector<int>{0, 1, 2, 3});
  m.def("gemm_bf16_8ph_tflops", &gemm_bf16_8ph_tflops, py::arg("device") = 0,
        py::arg("size") = 4096, py::arg("iters") = 10, py::arg("variant") = 0,
        py::call_guard<py::gil_scoped_release>());
  m.def("gemm_bf16_tflops", &gemm_bf16_tflops, py::arg("device") = 0,
        py::arg("size") = 4096, py::arg("iters") = 10, py::arg("swizzle") = 0,
        py::arg("bk") = 64, py::call_guard<py::gil_scoped_release>());
  m.def("stream_bandwidth_gbps", &stream_bandwidth_gbps, py::arg("device") = 0,
        py::arg("mib") = 1024, py::arg("iters") = 10,
        py::call_guard<py::gil_scoped_release>());
  m.def("memcpy_bandwidth_gbps", &memcpy_bandwidth_gbps, py::arg("device") = 0,
        py::arg("mib") = 1024, py::arg("iters") = 10,
        py::call_guard<py::gil_scoped_release>());
  m.def("p2p_bandwidth_gbps", &p2p_bandwidth_gbps, py::arg("src_dev"),
        py::arg("dst_dev"), py::arg("mib") = 512, py::arg("iters") = 10,
        py::call_guard<py::gil_scoped_release>());
  m.def("p2p_matrix", &p2p_matrix, py::arg("mib") = 256, py::arg("iters") = 5,
        py::call_guard<py::gil_scoped_release>());
  m.def("memtest_write", &hbm_memtest::memtest_write, py::arg("t"),
        py::arg("pattern"), py::arg("seed"), py::arg("base_word") = 0,
        py::arg("invert") = false);
  m.def("memtest_verify", &hbm_memtest::memtest_verify, py::arg("t"),
        py::arg("pattern"), py::arg("seed"), py::arg("base_word") = 0,
        py::arg("invert") = false, py::arg("max_records") = 32);
  m.def("memtest_verify_flip", &hbm_memtest::memtest_verify_flip, py::arg("t"),
        py::arg("pattern"), py::arg("seed"), py::arg("base_word") = 0,
        py::arg("invert") = false, py::arg("max_records") = 32);
  m.def("memtest_geometry", &hbm_memtest::memtest_geometry);
  m.def("hbm_memtest", &hbm_memtest::hbm_memtest, py::arg("device"),
        py::arg("chunk_bytes"), py::arg("seed"), py::arg("max_records") = 32,
        py::arg("scrub") = false, py::arg("inject") = py::list(),
        py::arg("base_word") = 0);
  m.def("cu_check", &cu_check::cu_check, py::arg("device"), py::arg("rounds"),
        py::arg("seed"), py::arg("grid_mult") = 2,
        py::arg("inject") = std::vector<std::vector<long long>>{});
  m.def("cu_check_tile", &cu_check::cu_check_tile, py::arg("fmt"),
        py::arg("tile"), py::arg("seed"));
  m.def("cu_check_geometry", &cu_check::cu_check_geometry);
  m.def("valu_check", &valu_check::valu_check, py::arg("device"), py::arg("rounds"),
        py::arg("seed"), py::arg("grid_mult") = 2,
        py::arg("inject") = std::vector<std::vector<long long>>{});
  m.def("valu_check_values", &valu_check::valu_check_values, py::arg("test"),
        py::arg("round"), py::arg("seed"));
  m.def("valu_check_table", &valu_check::valu_check_table, py::arg("rounds"),
        py::arg("seed"));
  m.def("valu_check_geometry", &valu_check::valu_check_geometry);
  m.def("gemm_check", &gemm_check::gemm_check, py::arg("device"), py::arg("kind"),
        py::arg("size"), py::arg("iters"), py::arg("seed"), py::arg("range"),
        py::arg("code") = -1, py::arg("max_records") = 32,
        py::arg("inject") = std::vector<std::vector<long long>>{},
        py::arg("loop") = gemm_check::kLoopNames[gemm_check::kDefaultLoop]);
  m.def("gemm_check_fill", &gemm_check::gemm_check_fill, py::arg("kind"),
        py::arg("operand"), py::arg("rows"), py::arg("K"), py::arg("seed"),
        py::arg("range"));
  m.def("gemm_check_expected", &gemm_check::gemm_check_expected, py::arg("kind"),
        py::arg("M"), py::arg("N"), py::arg("K"), py::arg("seed"), py::arg("range"));
  m.def("gemm_check_verify", &gemm_check::gemm_check_verify, py::arg("kind"),
        py::arg("C"), py::arg("K"), py::arg("seed"), py::arg("range"),
        py::arg("max_records") = 32, py::arg("atomic") = false);
  m.def("gemm_check_operand", &gemm_check::gemm_check_operand, py::arg("kind"),
        py::arg("operand"), py::arg("t"), py::arg("K"), py::arg("seed"),
        py::arg("range"));
  m.def("gemm_check_geometry", &gemm_check::gemm_check_geometry);
}
