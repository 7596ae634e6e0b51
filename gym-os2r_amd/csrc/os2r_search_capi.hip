// os2r_search_capi.hip — the C-ABI of libos2r_search.so (include/os2r_search.h): argument checks, a device guard, the calling
// thread's error text and the launch.  Every argument check runs before the first HIP call.
#include "os2r_search.hpp"

#include <atomic>
#include <cstring>
#include <string>

namespace {

using namespace os2r;

thread_local std::string g_error;

int fail(int code, const std::string& why) {
  g_error = "os2rs_ilqr_line_search: " + why;
  return code;
}

// The library is built with -fno-honor-nans -fno-honor-infinities: a double is tested on its bit pattern, read from memory as
// an integer (os2r_capi.hip, is_finite, says why).
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

bool symmetric(const double* x, int n) {
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j)
      if (x[i * n + j] != x[j * n + i]) return false;
  return true;
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
  int nknots; long long ntraj; int nalpha; unsigned flags;
  const void *knot_obs, *end_obs, *act; const uint8_t* done; const void* target;
  const double *q, *r, *qf;
  void *cost, *act_nom, *obs_nom, *end_nom, *lx, *lu, *pvec_final;
  int32_t *choice, *index; void* cand_cost;
  hipStream_t stream;
};

template <typename T>
int launch(const Call& c) {
  SearchArgs<T> p;
  std::memset(&p, 0, sizeof(p));
  const int nq = c.layout->nq, n = 2 * nq;
  p.knot_obs = (const T*)c.knot_obs; p.end_obs = (const T*)c.end_obs; p.act = (const T*)c.act; p.done = c.done;
  p.target = (const T*)c.target;
  p.cost = (T*)c.cost; p.act_nom = (T*)c.act_nom; p.obs_nom = (T*)c.obs_nom; p.end_nom = (T*)c.end_nom;
  p.lx = (T*)c.lx; p.lu = (T*)c.lu; p.pvec_final = (T*)c.pvec_final;
  p.choice = c.choice; p.index = c.index; p.cand_cost = (T*)c.cand_cost;
  p.M = c.ntraj; p.K = c.nknots; p.D = c.layout->obs_dim; p.nalpha = c.nalpha;
  p.accept_always = (c.flags & OS2RS_ACCEPT_ALWAYS) ? 1 : 0;
  // the lowest raw slot that shows each state column
  for (int col = 0; col < kLqrMaxN; ++col) p.col_slot[col] = -1;
  for (int d = c.layout->obs_dim - 1; d >= 0; --d)
    if (c.layout->slot_col[d] >= 0) p.col_slot[c.layout->slot_col[d]] = d;
  p.r00 = (T)c.r[0]; p.r01 = (T)c.r[1]; p.r11 = (T)c.r[3];
  const double* qf = c.qf ? c.qf : c.q;
  for (int i = 0; i < n * n; ++i) {
    p.q[i] = (T)c.q[i];
    p.qf[i] = (T)qf[i];
  }
  if (launch_ilqr_line_search<T>(nq, p, c.stream) != 0) return fail(OS2R_ERR_INVALID, "no kernel for this chain length");
  const hipError_t rc = hipGetLastError();
  if (rc != hipSuccess) return fail(OS2R_ERR_HIP, std::string("launch failed: ") + hipGetErrorString(rc));
  return OS2R_OK;
}

}  // namespace

extern "C" {

int os2rs_abi_version(void) { return OS2R_SEARCH_ABI_VERSION; }

const char* os2rs_last_error(void) { return g_error.c_str(); }

int os2rs_ilqr_line_search(const Os2rControlLayout* layout, int32_t nknots, int64_t ntraj, int32_t nalpha, uint32_t flags,
                           const void* knot_obs_dev, const void* end_obs_dev, const void* act_dev, const uint8_t* done_dev,
                           const void* target_dev, const double* q_host, const double* r_host, const double* qf_host, void* cost_dev,
                           void* act_nom_dev, void* obs_nom_dev, void* end_nom_dev, void* lx_dev, void* lu_dev, void* pvec_final_dev,
                           int32_t* choice_dev, int32_t* index_dev, void* cand_cost_dev, void* stream) {
  if (!layout) return fail(OS2R_ERR_INVALID, "null layout");
  if (layout->dtype != OS2R_F32 && layout->dtype != OS2R_F64) return fail(OS2R_ERR_INVALID, "layout->dtype must be OS2R_F32 or OS2R_F64");
  if (layout->nq < 2 || layout->nq > OS2R_MAX_DOF) return fail(OS2R_ERR_INVALID, "layout->nq must be 2..5");
  const int n = 2 * layout->nq;
  if (layout->obs_dim < 1 || layout->obs_dim > OS2R_MAX_OBS) return fail(OS2R_ERR_INVALID, "layout->obs_dim must be 1..12");
  for (int d = 0; d < layout->obs_dim; ++d)
    if (layout->slot_col[d] < -1 || layout->slot_col[d] >= n) return fail(OS2R_ERR_INVALID, "layout->slot_col entries must be -1..n-1");
  if (nknots < 1) return fail(OS2R_ERR_INVALID, "nknots must be >= 1");
  if (ntraj < 1) return fail(OS2R_ERR_INVALID, "ntraj must be >= 1");
  if (nalpha < 1 || nalpha > OS2RC_MAX_ALPHAS) return fail(OS2R_ERR_INVALID, "nalpha must be 1..16");
  if (ntraj > 0x7fffffffll / ((int64_t)nknots * nalpha))
    return fail(OS2R_ERR_INVALID, "nknots * nalpha * ntraj exceeds 2^31 - 1 (index_dev is int32)");
  if (flags & ~(uint32_t)OS2RS_ACCEPT_ALWAYS) return fail(OS2R_ERR_INVALID, "unknown flag bits");
  if (!knot_obs_dev) return fail(OS2R_ERR_INVALID, "null knot_obs_dev");
  if (!end_obs_dev) return fail(OS2R_ERR_INVALID, "null end_obs_dev");
  if (!act_dev) return fail(OS2R_ERR_INVALID, "null act_dev");
  if (!target_dev) return fail(OS2R_ERR_INVALID, "null target_dev");
  if (!q_host) return fail(OS2R_ERR_INVALID, "null q_host");
  if (!r_host) return fail(OS2R_ERR_INVALID, "null r_host");
  if (!cost_dev) return fail(OS2R_ERR_INVALID, "null cost_dev");
  if (!choice_dev) return fail(OS2R_ERR_INVALID, "null choice_dev");
  if (!all_finite(q_host, n * n)) return fail(OS2R_ERR_INVALID, "Q must be finite");
  if (!all_finite(r_host, 4)) return fail(OS2R_ERR_INVALID, "R must be finite");
  if (qf_host && !all_finite(qf_host, n * n)) return fail(OS2R_ERR_INVALID, "Qf must be finite");
  if (!symmetric(q_host, n)) return fail(OS2R_ERR_INVALID, "Q must be exactly symmetric");
  if (!symmetric(r_host, 2)) return fail(OS2R_ERR_INVALID, "R must be exactly symmetric");
  if (qf_host && !symmetric(qf_host, n)) return fail(OS2R_ERR_INVALID, "Qf must be exactly symmetric");
  // the device, from here on
  if (const int rc = check_device(layout->device)) return rc;
  DeviceGuard guard(layout->device);
  const Call c{layout, nknots, ntraj, nalpha, flags, knot_obs_dev, end_obs_dev, act_dev, done_dev, target_dev, q_host, r_host, qf_host,
               cost_dev, act_nom_dev, obs_nom_dev, end_nom_dev, lx_dev, lu_dev, pvec_final_dev, choice_dev, index_dev, cand_cost_dev,
               (hipStream_t)stream};
  return layout->dtype == OS2R_F64 ? launch<double>(c) : launch<float>(c);
}

}  // extern "C"
