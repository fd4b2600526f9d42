// Argument checks the burn-in bindings of hbm_memtest.hip, cu_check.hip,
// gemm_check.hip and valu_check.hip share. Host only; unlike hip_host.h this one speaks
// TORCH_CHECK, so it is not for the torch-free files.
#pragma once
#include <c10/util/Exception.h>

#include "burnin_core.h"
#include "hip_host.h"

namespace burnin {

constexpr u64 kMaxRecordsLimit = 65536;

inline u64 check_max_records(long long max_records) {
  TORCH_CHECK(max_records >= 0 && (u64)max_records <= kMaxRecordsLimit,
              "max_records must be in [0, ", kMaxRecordsLimit, "]");
  return (u64)max_records;
}

inline void check_device(int device) {
  int ndev = 0;
  HIP_CHECK(hipGetDeviceCount(&ndev));
  TORCH_CHECK(device >= 0 && device < ndev, "no such device ", device);
}

// One element of an inject entry that the kernel takes as a u32.
inline u32 check_inject_word(long long x) {
  TORCH_CHECK(x >= 0 && x <= 0xFFFFFFFFll, "inject: ", x,
              " is not an unsigned 32-bit value");
  return (u32)x;
}

}  // namespace burnin
