// os2r_pf_capi.hip — the C-ABI of libos2r_pf.so (include/os2r_pf.h): the entry point's own argument checks and the launch; the
// check of the layout, the device guard, the gfx950 check and the calling thread's error text are os2r_host.hpp's.  Every
// argument check runs before the first HIP call.
#include "os2r_pf.hpp"

#define OS2R_HOST_ERROR_PREFIX "os2rp_pf_update: "
#include "os2r_host.hpp"

#include <cfloat>

using namespace os2r;

extern "C" {

int os2rp_abi_version(void) { return OS2R_PF_ABI_VERSION; }

const char* os2rp_last_error(void) { return g_error.c_str(); }

int os2rp_pf_update(const Os2rControlLayout* layout, int64_t nrobots, int32_t nparticles, const void* obs_dev, const void* meas_dev,
                    const void* prec_dev, const void* logw_in_dev, const void* u_dev, double resample_ratio, void* logw_out_dev,
                    int32_t* index_dev, void* est_dev, void* weights_dev, void* ess_dev, int32_t* count_dev, int32_t* resampled_dev,
                    void* stream) {
  if (const char* why = layout_refusal(layout)) return fail(OS2R_ERR_INVALID, why);
  if (layout->obs_dim < 1 || layout->obs_dim > OS2R_MAX_OBS) return fail(OS2R_ERR_INVALID, "layout->obs_dim must be 1..12");
  if (nrobots < 1) return fail(OS2R_ERR_INVALID, "nrobots must be >= 1");
  if (nparticles < 1) return fail(OS2R_ERR_INVALID, "nparticles must be >= 1");
  if (nrobots > 0x7fffffffll / nparticles) return fail(OS2R_ERR_INVALID, "nparticles * nrobots exceeds 2^31 - 1");
  double ratio;
  {
    volatile double ratio_mem = resample_ratio;   // (the argument itself is declared free of NaNs: its bits are read back from memory)
    ratio = ratio_mem;
    if (!is_finite(&ratio)) return fail(OS2R_ERR_INVALID, "resample_ratio must be finite");
    if (ratio < 0.0) return fail(OS2R_ERR_INVALID, "resample_ratio must be >= 0");
  }
  if (!obs_dev) return fail(OS2R_ERR_INVALID, "null obs_dev");
  if (!meas_dev) return fail(OS2R_ERR_INVALID, "null meas_dev");
  if (!prec_dev) return fail(OS2R_ERR_INVALID, "null prec_dev");
  if (!logw_out_dev) return fail(OS2R_ERR_INVALID, "null logw_out_dev");
  if (!index_dev) return fail(OS2R_ERR_INVALID, "null index_dev");
  if (logw_in_dev) {
    const size_t elem = layout->dtype == OS2R_F64 ? sizeof(double) : sizeof(float);
    const uintptr_t in = (uintptr_t)logw_in_dev, out = (uintptr_t)logw_out_dev;
    const uintptr_t bytes = (uintptr_t)nparticles * (uintptr_t)nrobots * elem;
    // (the distance, not the ends: an end can wrap round at the top of the address space)
    if ((in < out ? out - in : in - out) < bytes) return fail(OS2R_ERR_INVALID, "logw_out_dev overlaps logw_in_dev");
  }
  // the device, from here on
  if (const int rc = check_device(layout->device)) return rc;
  DeviceGuard guard(layout->device);
  auto launch = [&](auto real) {
    using T = decltype(real);
    PfArgs<T> p;
    std::memset(&p, 0, sizeof(p));
    p.obs = (const T*)obs_dev; p.meas = (const T*)meas_dev; p.prec = (const T*)prec_dev; p.logw_in = (const T*)logw_in_dev;
    p.u = (const T*)u_dev; p.logw_out = (T*)logw_out_dev; p.index = index_dev; p.est = (T*)est_dev; p.weights = (T*)weights_dev;
    p.ess = (T*)ess_dev; p.count = count_dev; p.resampled = resampled_dev;
    p.M = nrobots; p.S = nparticles; p.D = layout->obs_dim;
    // rounded once to the dtype; above its largest finite number, that number
    p.ratio = sizeof(T) == sizeof(float) && ratio > (double)FLT_MAX ? (T)FLT_MAX : (T)ratio;
    launch_pf_update<T>(p, (hipStream_t)stream);
    return launched(0);
  };
  return layout->dtype == OS2R_F64 ? launch(double()) : launch(float());
}

}  // extern "C"
