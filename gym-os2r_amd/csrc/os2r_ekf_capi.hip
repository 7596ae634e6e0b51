// os2r_ekf_capi.hip — the C-ABI of libos2r_ekf.so (include/os2r_ekf.h): the entry point's own argument checks and the launch; the
// checks of the layout and its slots, the device guard, the gfx950 check and the calling thread's error text are os2r_host.hpp's.
// Every argument check runs before the first HIP call.
#include "os2r_ekf.hpp"

#define OS2R_HOST_ERROR_PREFIX "os2re_ekf_update: "
#include "os2r_host.hpp"

#include <cfloat>

using namespace os2r;

extern "C" {

int os2re_abi_version(void) { return OS2R_EKF_ABI_VERSION; }

const char* os2re_last_error(void) { return g_error.c_str(); }

int os2re_ekf_update(const Os2rControlLayout* layout, int64_t nrobots, const void* x_pred_dev, const void* p_in_dev, const void* a_dev,
                     const double* q_host, const void* meas_dev, const void* prec_dev, double gate, void* x_out_dev, void* p_out_dev,
                     void* nis_dev, int32_t* used_dev, int32_t* refused_dev, void* innov_dev, void* stream) {
  if (const char* why = layout_refusal(layout)) return fail(OS2R_ERR_INVALID, why);
  if (const char* why = slots_refusal(layout)) return fail(OS2R_ERR_INVALID, why);   // (slot_col picks rows of P in LDS)
  const int n = 2 * layout->nq;
  if (nrobots < 1) return fail(OS2R_ERR_INVALID, "nrobots must be >= 1");
  if (nrobots > 0x7fffffffll / (n * n)) return fail(OS2R_ERR_INVALID, "n * n * nrobots exceeds 2^31 - 1");
  if (!x_pred_dev) return fail(OS2R_ERR_INVALID, "null x_pred_dev");
  if (!p_in_dev) return fail(OS2R_ERR_INVALID, "null p_in_dev");
  if (!meas_dev) return fail(OS2R_ERR_INVALID, "null meas_dev");
  if (!prec_dev) return fail(OS2R_ERR_INVALID, "null prec_dev");
  if (!x_out_dev) return fail(OS2R_ERR_INVALID, "null x_out_dev");
  if (!p_out_dev) return fail(OS2R_ERR_INVALID, "null p_out_dev");
  if (a_dev) {
    if (!q_host) return fail(OS2R_ERR_INVALID, "a_dev needs q_host");
    if (!all_finite(q_host, n * n)) return fail(OS2R_ERR_INVALID, "Q must be finite");
    if (!symmetric(q_host, n)) return fail(OS2R_ERR_INVALID, "Q must be exactly symmetric");
  }
  double gate_value;
  {
    volatile double gate_mem = gate;   // (the argument itself is declared free of NaNs: its bits are read back from memory)
    gate_value = gate_mem;
    if (!is_finite(&gate_value)) return fail(OS2R_ERR_INVALID, "gate must be finite");
    if (gate_value < 0.0) return fail(OS2R_ERR_INVALID, "gate must be >= 0");
  }
  {
    // an output is its input's very pointer or clear of it
    // (the distance, not the ends: an end can wrap round at the top of the address space)
    const size_t elem = layout->dtype == OS2R_F64 ? sizeof(double) : sizeof(float);
    const uintptr_t rows = (uintptr_t)n * (uintptr_t)nrobots * elem;
    const uintptr_t xi = (uintptr_t)x_pred_dev, xo = (uintptr_t)x_out_dev, pi = (uintptr_t)p_in_dev, po = (uintptr_t)p_out_dev;
    if (xi != xo && (xi < xo ? xo - xi : xi - xo) < rows) return fail(OS2R_ERR_INVALID, "x_out_dev overlaps x_pred_dev without being it");
    if (pi != po && (pi < po ? po - pi : pi - po) < rows * n) return fail(OS2R_ERR_INVALID, "p_out_dev overlaps p_in_dev without being it");
  }
  // the device, from here on
  if (const int rc = check_device(layout->device)) return rc;
  DeviceGuard guard(layout->device);
  auto launch = [&](auto real) {
    using T = decltype(real);
    EkfArgs<T> p;
    std::memset(&p, 0, sizeof(p));
    p.x_pred = (const T*)x_pred_dev; p.p_in = (const T*)p_in_dev; p.a = (const T*)a_dev; p.meas = (const T*)meas_dev;
    p.prec = (const T*)prec_dev; p.x_out = (T*)x_out_dev; p.p_out = (T*)p_out_dev; p.nis = (T*)nis_dev; p.used = used_dev;
    p.refused = refused_dev; p.innov = (T*)innov_dev;
    p.M = nrobots; p.D = layout->obs_dim;
    for (int d = 0; d < OS2R_MAX_OBS; ++d) p.slot_col[d] = d < layout->obs_dim ? layout->slot_col[d] : -1;
    // rounded once to the dtype; above its largest finite number, that number
    p.gate = sizeof(T) == sizeof(float) && gate_value > (double)FLT_MAX ? (T)FLT_MAX : (T)gate_value;
    if (a_dev)
      for (int i = 0; i < n * n; ++i) p.q[i] = (T)q_host[i];
    return launched(launch_ekf_update<T>(layout->nq, p, (hipStream_t)stream));
  };
  return layout->dtype == OS2R_F64 ? launch(double()) : launch(float());
}

}  // extern "C"
