// os2r_control_capi.hip — the C-ABI of libos2r_control.so (include/os2r_control.h): argument checks, a device guard, the
// calling thread's error text and the launch.  Every argument check runs before the first HIP call.
#include "os2r_ilqr.hpp"

#include <atomic>
#include <cstring>
#include <string>

namespace {

using namespace os2r;

thread_local std::string g_error;

int fail(int code, const std::string& why) {
  g_error = "os2rc_ilqr_backward: " + why;
  return code;
}

// The library is built with -fno-honor-nans -fno-honor-infinities: a double is tested on its bit pattern, read from memory as
// an integer (os2r_capi.hip, is_finite, says why).
__attribute__((noinline)) bool is_finite(const double* x) {
  uint64_t b;
  std::memcpy(&b, x, sizeof(b));
  return ((b >> 52) & 0x7ffu) != 0x7ffu;
}

// the call works on the layout's device and leaves the caller's current device as it found it
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

struct Call {
  const Os2rControlLayout* layout;
  int nknots; long long ntraj;
  const void *a, *b, *lx, *lu;
  const double *q, *r; double mu;
  const void *pmat_final, *pvec_final;
  void *gain, *ff, *pmat_out, *pvec_out; uint8_t* flag; void* dv;
  const void *actions, *obs; const double* alpha; int nalpha; void* weights;
  hipStream_t stream;
};

template <typename T>
int launch(const Call& c) {
  IlqrArgs<T> p;
  std::memset(&p, 0, sizeof(p));
  const int nq = c.layout->nq, n = 2 * nq;
  p.a = (const T*)c.a; p.b = (const T*)c.b; p.lx = (const T*)c.lx; p.lu = (const T*)c.lu;
  p.pmat_final = (const T*)c.pmat_final; p.pvec_final = (const T*)c.pvec_final; p.pmat_out = (T*)c.pmat_out; p.pvec_out = (T*)c.pvec_out;
  p.gain = (T*)c.gain; p.ff = (T*)c.ff; p.flag = c.flag; p.dv = (T*)c.dv;
  p.M = c.ntraj; p.K = c.nknots;
  for (int d = 0; d < OS2R_MAX_OBS; ++d) p.slot_col[d] = -1;
  if (c.weights) {
    p.actions = (const T*)c.actions; p.obs = (const T*)c.obs; p.weights = (T*)c.weights;
    p.D = c.layout->obs_dim; p.nalpha = c.nalpha;
    for (int d = 0; d < p.D; ++d) p.slot_col[d] = c.layout->slot_col[d];
    for (int i = 0; i < c.nalpha; ++i) p.alpha[i] = (T)c.alpha[i];
  }
  p.r00 = (T)c.r[0]; p.r01 = (T)c.r[1]; p.r11 = (T)c.r[3]; p.mu = (T)c.mu;
  for (int i = 0; i < n * n; ++i) p.q[i] = (T)c.q[i];
  if (launch_ilqr_backward<T>(nq, p, c.stream) != 0) return fail(OS2R_ERR_INVALID, "no kernel for this chain length");
  const hipError_t rc = hipGetLastError();
  if (rc != hipSuccess) return fail(OS2R_ERR_HIP, std::string("launch failed: ") + hipGetErrorString(rc));
  return OS2R_OK;
}

}  // namespace

extern "C" {

int os2rc_abi_version(void) { return OS2R_CONTROL_ABI_VERSION; }

const char* os2rc_last_error(void) { return g_error.c_str(); }

int os2rc_ilqr_backward(const Os2rControlLayout* layout, int32_t nknots, int64_t ntraj, const void* a_dev, const void* b_dev,
                        const void* lx_dev, const void* lu_dev, const double* q_host, const double* r_host, double mu,
                        const void* pmat_final_dev, const void* pvec_final_dev, void* gain_dev, void* ff_dev, void* pmat_out_dev,
                        void* pvec_out_dev, uint8_t* flag_dev, void* dv_dev, const void* actions_dev, const void* obs_dev,
                        const double* alpha_host, int32_t nalpha, void* weights_dev, void* stream) {
  if (!layout) return fail(OS2R_ERR_INVALID, "null layout");
  if (layout->dtype != OS2R_F32 && layout->dtype != OS2R_F64) return fail(OS2R_ERR_INVALID, "layout->dtype must be OS2R_F32 or OS2R_F64");
  if (layout->nq < 2 || layout->nq > OS2R_MAX_DOF) return fail(OS2R_ERR_INVALID, "layout->nq must be 2..5");
  if (nknots < 1) return fail(OS2R_ERR_INVALID, "nknots must be >= 1");
  if (ntraj < 1) return fail(OS2R_ERR_INVALID, "ntraj must be >= 1");
  if (ntraj > (int64_t)kLqrEnvs * 0x7fffffffll) return fail(OS2R_ERR_INVALID, "ntraj exceeds what one launch covers");
  if (!a_dev) return fail(OS2R_ERR_INVALID, "null a_dev");
  if (!b_dev) return fail(OS2R_ERR_INVALID, "null b_dev");
  if (!q_host) return fail(OS2R_ERR_INVALID, "null q_host");
  if (!r_host) return fail(OS2R_ERR_INVALID, "null r_host");
  const int n = 2 * layout->nq;
  for (int i = 0; i < n * n; ++i)
    if (!is_finite(&q_host[i])) return fail(OS2R_ERR_INVALID, "Q must be finite");
  for (int i = 0; i < 4; ++i)
    if (!is_finite(&r_host[i])) return fail(OS2R_ERR_INVALID, "R must be finite");
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j)
      if (q_host[i * n + j] != q_host[j * n + i]) return fail(OS2R_ERR_INVALID, "Q must be exactly symmetric");
  if (r_host[1] != r_host[2]) return fail(OS2R_ERR_INVALID, "R must be exactly symmetric");
  {
    volatile double mu_mem = mu;   // (the argument itself is declared free of NaNs: its bits are read back from memory)
    const double mu_read = mu_mem;
    if (!is_finite(&mu_read)) return fail(OS2R_ERR_INVALID, "mu must be finite");
    if (mu_read < 0.0) return fail(OS2R_ERR_INVALID, "mu must be >= 0");
  }
  if (!gain_dev && !ff_dev && !pmat_out_dev && !pvec_out_dev && !dv_dev && !weights_dev)
    return fail(OS2R_ERR_INVALID, "all outputs are null (gain, ff, pmat_out, pvec_out, dv, weights)");
  if (weights_dev) {
    if (!actions_dev || !obs_dev || !alpha_host) return fail(OS2R_ERR_INVALID, "weights need actions_dev, obs_dev and alpha_host");
    if (nalpha < 1 || nalpha > OS2RC_MAX_ALPHAS) return fail(OS2R_ERR_INVALID, "nalpha must be 1..16");
    for (int i = 0; i < nalpha; ++i)
      if (!is_finite(&alpha_host[i])) return fail(OS2R_ERR_INVALID, "alpha must be finite");
    if (layout->obs_dim < 1 || layout->obs_dim > OS2R_MAX_OBS) return fail(OS2R_ERR_INVALID, "layout->obs_dim must be 1..12");
    for (int d = 0; d < layout->obs_dim; ++d)
      if (layout->slot_col[d] < -1 || layout->slot_col[d] >= n) return fail(OS2R_ERR_INVALID, "layout->slot_col entries must be -1..n-1");
  }
  // the device, from here on
  if (const int rc = check_device(layout->device)) return rc;
  DeviceGuard guard(layout->device);
  const Call c{layout, nknots, ntraj, a_dev, b_dev, lx_dev, lu_dev, q_host, r_host, mu, pmat_final_dev, pvec_final_dev, gain_dev, ff_dev,
               pmat_out_dev, pvec_out_dev, flag_dev, dv_dev, actions_dev, obs_dev, alpha_host, nalpha, weights_dev, (hipStream_t)stream};
  return layout->dtype == OS2R_F64 ? launch<double>(c) : launch<float>(c);
}

}  // extern "C"
