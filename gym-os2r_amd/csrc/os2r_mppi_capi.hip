// os2r_mppi_capi.hip — the C-ABI of libos2r_mppi.so (include/os2r_mppi.h): the entry point's own argument checks and the launch; the
// check of the layout, the device guard, the gfx950 check and the calling thread's error text are os2r_host.hpp's.  Every
// argument check runs before the first HIP call.
#include "os2r_mppi.hpp"

#define OS2R_HOST_ERROR_PREFIX "os2rm_mppi_update: "
#include "os2r_host.hpp"

#include <cfloat>

using namespace os2r;

extern "C" {

int os2rm_abi_version(void) { return OS2R_MPPI_ABI_VERSION; }

const char* os2rm_last_error(void) { return g_error.c_str(); }

int os2rm_mppi_update(const Os2rControlLayout* layout, int32_t nknots, int64_t nrobots, int32_t nsamples, const void* returns_dev,
                      const void* actions_dev, const void* nominal_in_dev, double beta, int32_t shift, uint32_t flags,
                      void* nominal_out_dev, void* applied_dev, void* table_dev, void* weights_dev, void* ess_dev, int32_t* count_dev,
                      void* stream) {
  if (const char* why = layout_refusal(layout)) return fail(OS2R_ERR_INVALID, why);
  if (nknots < 1) return fail(OS2R_ERR_INVALID, "nknots must be >= 1");
  if (nknots > 65535) return fail(OS2R_ERR_INVALID, "nknots must be <= 65535 (one grid row per slot)");
  if (nrobots < 1) return fail(OS2R_ERR_INVALID, "nrobots must be >= 1");
  if (nsamples < 1) return fail(OS2R_ERR_INVALID, "nsamples must be >= 1");
  if (nrobots > 0x7fffffffll / nsamples) return fail(OS2R_ERR_INVALID, "nsamples * nrobots exceeds 2^31 - 1");
  if (shift < 0 || shift > nknots) return fail(OS2R_ERR_INVALID, "shift must be 0..nknots");
  if (flags & ~(uint32_t)OS2RM_TAIL_ZERO) return fail(OS2R_ERR_INVALID, "unknown flag bits");
  {
    volatile double beta_mem = beta;   // (the argument itself is declared free of NaNs: its bits are read back from memory)
    const double beta_read = beta_mem;
    if (!is_finite(&beta_read)) return fail(OS2R_ERR_INVALID, "beta must be finite");
    if (beta_read <= 0.0) return fail(OS2R_ERR_INVALID, "beta must be > 0");
    if (layout->dtype == OS2R_F32 && (beta_read < (double)FLT_MIN || beta_read > (double)FLT_MAX))
      return fail(OS2R_ERR_INVALID, "beta is outside the normal range of fp32");
  }
  if (!returns_dev) return fail(OS2R_ERR_INVALID, "null returns_dev");
  if (!actions_dev) return fail(OS2R_ERR_INVALID, "null actions_dev");
  if (!nominal_in_dev) return fail(OS2R_ERR_INVALID, "null nominal_in_dev");
  if (!nominal_out_dev) return fail(OS2R_ERR_INVALID, "null nominal_out_dev");
  const size_t elem = layout->dtype == OS2R_F64 ? sizeof(double) : sizeof(float);
  if ((uintptr_t)actions_dev % (2 * elem)) return fail(OS2R_ERR_INVALID, "actions_dev must be aligned to a pair of its elements");
  {
    const uintptr_t in = (uintptr_t)nominal_in_dev, out = (uintptr_t)nominal_out_dev;
    const uintptr_t bytes = (uintptr_t)nknots * (uintptr_t)nrobots * 2 * elem;
    if (in < out + bytes && out < in + bytes) return fail(OS2R_ERR_INVALID, "nominal_out_dev overlaps nominal_in_dev");
  }
  if (table_dev && (layout->obs_dim < 1 || layout->obs_dim > OS2R_MAX_OBS))
    return fail(OS2R_ERR_INVALID, "layout->obs_dim must be 1..12 when table_dev is given");
  // the device, from here on
  if (const int rc = check_device(layout->device)) return rc;
  DeviceGuard guard(layout->device);
  auto launch = [&](auto real) {
    using T = decltype(real);
    MppiArgs<T> p;
    std::memset(&p, 0, sizeof(p));
    p.returns = (const T*)returns_dev; p.actions = (const T*)actions_dev; p.nominal_in = (const T*)nominal_in_dev;
    p.nominal_out = (T*)nominal_out_dev; p.applied = (T*)applied_dev; p.table = (T*)table_dev; p.weights = (T*)weights_dev;
    p.ess = (T*)ess_dev; p.count = count_dev;
    p.M = nrobots; p.K = nknots; p.S = nsamples; p.D = table_dev ? layout->obs_dim : 0; p.shift = shift;
    p.tail_zero = (flags & OS2RM_TAIL_ZERO) ? 1 : 0;
    p.beta = (T)beta;
    launch_mppi_update<T>(p, (hipStream_t)stream);
    return launched(0);
  };
  return layout->dtype == OS2R_F64 ? launch(double()) : launch(float());
}

}  // extern "C"
