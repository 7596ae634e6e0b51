// os2r_host.hpp — the host plumbing the C-ABI units share (os2r_capi.hip, os2r_control_capi.hip, os2r_search_capi.hip): the
// finite and symmetric tests of host matrices, the device guard and, for a unit that names its entry point in
// OS2R_HOST_ERROR_PREFIX before it includes this file, the calling thread's error text, the gfx950 check, the layout checks and
// the verdict on a launch.
// Host only, and never part of a kernel header: the JIT units compile those.  Everything has internal linkage, so every library
// keeps an error text and a device cache of its own.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/os2r.h"

namespace {

// The libraries are built with -fno-honor-nans -fno-honor-infinities: a comparison written to fail on a NaN, `!(x > 0.0)`, is
// compiled as if there were none, and a NaN passes it (so does std::isfinite, and a test of the bits of a double passed by value:
// the argument itself is declared free of NaNs).  A double of the caller's is therefore tested on its bit pattern first, read
// from memory as an integer.
__attribute__((noinline)) bool is_finite(const double* x) {
  uint64_t b;
  std::memcpy(&b, x, sizeof(b));
  return ((b >> 52) & 0x7ffu) != 0x7ffu;
}

bool all_finite(const double* x, int count) {
  for (int i = 0; i < count; ++i)
    if (!is_finite(&x[i])) return false;
  return true;
}

// x [n][n] row-major, compared exactly
bool symmetric(const double* x, int n) {
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j)
      if (x[i * n + j] != x[j * n + i]) return false;
  return true;
}

// Every entry point works on the device of its handle or layout and leaves the caller's current device as it found it
// (a process may hold handles on several GPUs; torch keeps its own idea of the current device).
struct DeviceGuard {
  int prev = -1, dev = -1;
  explicit DeviceGuard(int device) : dev(device) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    if (prev >= 0 && prev != dev) (void)hipSetDevice(prev);
  }
};

}  // namespace

#ifdef OS2R_HOST_ERROR_PREFIX
#include "../../include/os2r_control.h"

namespace {

thread_local std::string g_error;

int fail(int code, const std::string& why) {
  g_error = OS2R_HOST_ERROR_PREFIX + why;
  return code;
}

// is `device` a visible gfx950?  Asked of the runtime once per ordinal (0: not asked yet, 1: yes).
constexpr int kKnownDevices = 64;
std::atomic<int> g_is_gfx950[kKnownDevices];

int check_device(int device) {
  if (device >= 0 && device < kKnownDevices && g_is_gfx950[device].load(std::memory_order_relaxed) == 1) return OS2R_OK;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(OS2R_ERR_NO_DEVICE, "no HIP device visible");
  if (device < 0 || device >= ndev) return fail(OS2R_ERR_NO_DEVICE, "layout->device is no visible device");
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return fail(OS2R_ERR_HIP, "hipGetDeviceProperties failed");
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(OS2R_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
  if (device < kKnownDevices) g_is_gfx950[device].store(1, std::memory_order_relaxed);
  return OS2R_OK;
}

// What follows a launch: 1 from the dispatcher says that there is no kernel, then the runtime's verdict on the launch
int launched(int no_kernel) {
  if (no_kernel != 0) return fail(OS2R_ERR_INVALID, "no kernel for this chain length");
  const hipError_t rc = hipGetLastError();
  if (rc != hipSuccess) return fail(OS2R_ERR_HIP, std::string("launch failed: ") + hipGetErrorString(rc));
  return OS2R_OK;
}

// What an entry point refuses about its layout, as the refusal's text (null: nothing): the layout itself, which every call
// reads, and its observation slots, which a call reads that forms errors or a weight table from observations.
const char* layout_refusal(const Os2rControlLayout* layout) {
  if (!layout) return "null layout";
  if (layout->dtype != OS2R_F32 && layout->dtype != OS2R_F64) return "layout->dtype must be OS2R_F32 or OS2R_F64";
  if (layout->nq < 2 || layout->nq > OS2R_MAX_DOF) return "layout->nq must be 2..5";
  return nullptr;
}

const char* slots_refusal(const Os2rControlLayout* layout) {
  if (layout->obs_dim < 1 || layout->obs_dim > OS2R_MAX_OBS) return "layout->obs_dim must be 1..12";
  for (int d = 0; d < layout->obs_dim; ++d)
    if (layout->slot_col[d] < -1 || layout->slot_col[d] >= 2 * layout->nq) return "layout->slot_col entries must be -1..n-1";
  return nullptr;
}

}  // namespace
#endif
