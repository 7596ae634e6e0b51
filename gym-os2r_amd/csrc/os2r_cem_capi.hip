// os2r_cem_capi.hip — the C-ABI of libos2r_cem.so (include/os2r_cem.h): the entry point's own argument checks and the two
// launches; the check of the layout, the device guard, the gfx950 check and the calling thread's error text are os2r_host.hpp's.
// Every argument check runs before the first HIP call.
#include "os2r_cem.hpp"

#define OS2R_HOST_ERROR_PREFIX "os2rx_cem_update: "
#include "os2r_host.hpp"

#include <cfloat>

using namespace os2r;

namespace {

// [a, a + na) and [b, b + nb) share a byte
bool overlap(const void* a, uintptr_t na, const void* b, uintptr_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

// non-zero and outside the normal range of fp32
bool beyond_fp32(double x) { return x != 0.0 && (x < (double)FLT_MIN || x > (double)FLT_MAX); }

}  // namespace

extern "C" {

int os2rx_abi_version(void) { return OS2R_CEM_ABI_VERSION; }

const char* os2rx_last_error(void) { return g_error.c_str(); }

int os2rx_cem_update(const Os2rControlLayout* layout, int32_t nknots, int64_t nrobots, int32_t nsamples, int32_t nelite,
                     const void* returns_dev, const void* actions_dev, const void* nominal_in_dev, const void* sigma_in_dev, double gain,
                     double sigma_gain, double sigma_min, double sigma_max, int32_t shift, uint32_t flags, void* nominal_out_dev,
                     void* var_out_dev, void* sigma_out_dev, void* applied_dev, void* table_dev, void* lane_sigma_dev, int32_t* elite_dev,
                     void* threshold_dev, int32_t* count_dev, void* stream) {
  if (const char* why = layout_refusal(layout)) return fail(OS2R_ERR_INVALID, why);
  if (nknots < 1) return fail(OS2R_ERR_INVALID, "nknots must be >= 1");
  if (nknots > 65535) return fail(OS2R_ERR_INVALID, "nknots must be <= 65535 (one grid row per knot)");
  if (nrobots < 1) return fail(OS2R_ERR_INVALID, "nrobots must be >= 1");
  if (nsamples < 1) return fail(OS2R_ERR_INVALID, "nsamples must be >= 1");
  if (nelite < 1) return fail(OS2R_ERR_INVALID, "nelite must be >= 1");
  if (nelite > nsamples) return fail(OS2R_ERR_INVALID, "nelite must be <= nsamples");
  if (nrobots > 0x7fffffffll / nsamples) return fail(OS2R_ERR_INVALID, "nsamples * nrobots exceeds 2^31 - 1");
  if (shift < 0 || shift > nknots) return fail(OS2R_ERR_INVALID, "shift must be 0..nknots");
  if (flags & ~(uint32_t)OS2RX_TAIL_ZERO) return fail(OS2R_ERR_INVALID, "unknown flag bits");
  {
    // (the arguments themselves are declared free of NaNs: their bits are read back from memory)
    volatile double mem[4] = {gain, sigma_gain, sigma_min, sigma_max};
    const double g = mem[0], sg = mem[1], lo = mem[2], hi = mem[3];
    const bool f32 = layout->dtype == OS2R_F32;
    if (!is_finite(&g)) return fail(OS2R_ERR_INVALID, "gain must be finite");
    if (g <= 0.0 || g > 1.0) return fail(OS2R_ERR_INVALID, "gain must be in (0, 1]");
    if (f32 && beyond_fp32(g)) return fail(OS2R_ERR_INVALID, "gain is outside the normal range of fp32");
    if (!is_finite(&sg)) return fail(OS2R_ERR_INVALID, "sigma_gain must be finite");
    if (sg <= 0.0 || sg > 1.0) return fail(OS2R_ERR_INVALID, "sigma_gain must be in (0, 1]");
    if (f32 && beyond_fp32(sg)) return fail(OS2R_ERR_INVALID, "sigma_gain is outside the normal range of fp32");
    if (!is_finite(&lo)) return fail(OS2R_ERR_INVALID, "sigma_min must be finite");
    if (lo < 0.0) return fail(OS2R_ERR_INVALID, "sigma_min must be >= 0");
    if (f32 && beyond_fp32(lo)) return fail(OS2R_ERR_INVALID, "sigma_min is outside the normal range of fp32");
    if (!is_finite(&hi)) return fail(OS2R_ERR_INVALID, "sigma_max must be finite");
    if (hi < 0.0) return fail(OS2R_ERR_INVALID, "sigma_max must be >= 0");
    if (f32 && beyond_fp32(hi)) return fail(OS2R_ERR_INVALID, "sigma_max is outside the normal range of fp32");
    if (lo > hi) return fail(OS2R_ERR_INVALID, "sigma_min must be <= sigma_max");
  }
  if (!returns_dev) return fail(OS2R_ERR_INVALID, "null returns_dev");
  if (!actions_dev) return fail(OS2R_ERR_INVALID, "null actions_dev");
  if (!nominal_in_dev) return fail(OS2R_ERR_INVALID, "null nominal_in_dev");
  if (!sigma_in_dev) return fail(OS2R_ERR_INVALID, "null sigma_in_dev");
  if (!nominal_out_dev) return fail(OS2R_ERR_INVALID, "null nominal_out_dev");
  if (!var_out_dev) return fail(OS2R_ERR_INVALID, "null var_out_dev");
  if (!sigma_out_dev) return fail(OS2R_ERR_INVALID, "null sigma_out_dev");
  const size_t elem = layout->dtype == OS2R_F64 ? sizeof(double) : sizeof(float);
  if ((uintptr_t)actions_dev % (2 * elem)) return fail(OS2R_ERR_INVALID, "actions_dev must be aligned to a pair of its elements");
  {
    const uintptr_t lanes = (uintptr_t)nsamples * (uintptr_t)nrobots;
    const uintptr_t knots = (uintptr_t)nknots * (uintptr_t)nrobots * 2 * elem;     // a nominal, and var_out
    if (overlap(nominal_in_dev, knots, nominal_out_dev, knots)) return fail(OS2R_ERR_INVALID, "nominal_out_dev overlaps nominal_in_dev");
    if (overlap(var_out_dev, knots, returns_dev, lanes * elem)) return fail(OS2R_ERR_INVALID, "var_out_dev overlaps returns_dev");
    if (overlap(var_out_dev, knots, actions_dev, (uintptr_t)nknots * lanes * 2 * elem))
      return fail(OS2R_ERR_INVALID, "var_out_dev overlaps actions_dev");
    if (overlap(var_out_dev, knots, nominal_in_dev, knots)) return fail(OS2R_ERR_INVALID, "var_out_dev overlaps nominal_in_dev");
    if (overlap(var_out_dev, knots, sigma_in_dev, (uintptr_t)nrobots * 2 * elem))
      return fail(OS2R_ERR_INVALID, "var_out_dev overlaps sigma_in_dev");
  }
  if (table_dev && (layout->obs_dim < 1 || layout->obs_dim > OS2R_MAX_OBS))
    return fail(OS2R_ERR_INVALID, "layout->obs_dim must be 1..12 when table_dev is given");
  // the device, from here on
  if (const int rc = check_device(layout->device)) return rc;
  DeviceGuard guard(layout->device);
  auto launch = [&](auto real) {
    using T = decltype(real);
    CemArgs<T> p;
    std::memset(&p, 0, sizeof(p));
    p.returns = (const T*)returns_dev; p.actions = (const T*)actions_dev; p.nominal_in = (const T*)nominal_in_dev;
    p.sigma_in = (const T*)sigma_in_dev; p.nominal_out = (T*)nominal_out_dev; p.var_out = (T*)var_out_dev; p.sigma_out = (T*)sigma_out_dev;
    p.applied = (T*)applied_dev; p.table = (T*)table_dev; p.lane_sigma = (T*)lane_sigma_dev; p.elite = elite_dev;
    p.threshold = (T*)threshold_dev; p.count = count_dev;
    p.M = nrobots; p.K = nknots; p.S = nsamples; p.E = nelite; p.D = table_dev ? layout->obs_dim : 0; p.shift = shift;
    p.tail_zero = (flags & OS2RX_TAIL_ZERO) ? 1 : 0;
    p.gain = (T)gain; p.sigma_gain = (T)sigma_gain; p.sigma_min = (T)sigma_min; p.sigma_max = (T)sigma_max;
    launch_cem_update<T>(p, (hipStream_t)stream);
    return launched(0);
  };
  return layout->dtype == OS2R_F64 ? launch(double()) : launch(float());
}

}  // extern "C"
