// Host-side launch helpers shared by the entry points: 1-D grid sizing, the device's CU count, a launch with raised
// dynamic LDS, and the runtime dtype code turned into a template argument.  Host only; nothing here is device code.
#pragma once
#include "common.h"

// Blocks of 256 threads for a grid-stride loop over `total` items, at most `cap`: min(cap, ceil(total / 256)).  0 for
// total == 0: a site that needs at least one block says so at the call.
constexpr unsigned grid1d(unsigned long long total, unsigned cap) {
  return (unsigned)((total + 255) / 256 > cap ? cap : (total + 255) / 256);
}
static_assert(grid1d(0, 4096) == 0 && grid1d(1, 4096) == 1 && grid1d(256, 8192) == 1 && grid1d(257, 8192) == 2, "grid1d");
static_assert(grid1d(16384ull * 256, 16384) == 16384 && grid1d(16384ull * 256 + 1, 16384) == 16384, "grid1d at its cap");
static_assert(grid1d(16384ull * 256 - 256, 16384) == 16383 && grid1d(4096ull * 256 + 1, 32768) == 4097, "grid1d below its cap");
static_assert(grid1d(131072ull * 256 + 1, 131072) == 131072 && grid1d(2048ull * 256, 2048) == 2048, "grid1d at its cap");
static_assert(grid1d((1ull << 32) + 1, 32768) == 32768 && grid1d((1ull << 32) + 1, 0xFFFFFFFFu) == (1u << 24) + 1,
              "grid1d above 2^32 items");

// Compute units of the current device, asked once per device id (a multi-GPU process may hold devices with different
// CU counts); 256 where the runtime does not say.
static inline int mega_cu_count() {
  static int cached[64] = {0};
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  if (!cached[dev]) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) cached[dev] = n;
    else cached[dev] = 256;
  }
  return cached[dev];
}

// Launch with lds_bytes of dynamic LDS, which may exceed the 64 KiB default: the limit is raised on every call (it is a
// per-device property of the kernel, so a per-process flag would miss a second device).  MEGA_ERR_LAUNCH if the runtime
// refuses the limit, else what mega_check_launch() says after the launch.
template <typename... KArgs, typename... Args>
static inline int launch_lds(void (*kernel)(KArgs...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, Args... args) {
  const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    g_mega_last_hip_error = (int)e;
    return MEGA_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(kernel, grid, block, lds_bytes, st, args...);
  return mega_check_launch();
}

// The runtime dtype code as a type: f is a generic lambda, `[&](auto tag) { using T = decltype(tag); ...; return rc; }`.
// MEGA_ERR_ARG for a code outside the set.
template <typename F> static inline int dispatch_half(int dtype, F&& f) {
  if (dtype == MEGA_BF16) return f(bf16_t{});
  if (dtype == MEGA_F16) return f(f16_t{});
  return MEGA_ERR_ARG;
}
template <typename F> static inline int dispatch_elem(int dtype, F&& f) {
  if (dtype == MEGA_F32) return f(float{});
  return dispatch_half(dtype, f);
}
