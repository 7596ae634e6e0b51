// os2r_ukf_capi.hip — the C-ABI of libos2r_ukf.so (include/os2r_ukf.h): the entry points' own argument checks and the launches; the
// checks of the layout and its slots, the device guard, the gfx950 check and the calling thread's error text are os2r_host.hpp's.
// Every argument check runs before the first HIP call.
#include "os2r_ukf.hpp"

// two entry points, two prefixes: each names itself here on entry, and os2r_host.hpp's fail() puts that name in front
namespace {
thread_local const char* g_entry_point = "";
}
#define OS2R_HOST_ERROR_PREFIX g_entry_point
#include "os2r_host.hpp"

#include <cfloat>

using namespace os2r;

namespace {

// do [a, a + na) and [b, b + nb) share a byte?  By the distance, not the ends: an end can wrap round at the top of the address space
bool overlap(const void* a, uintptr_t na, const void* b, uintptr_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb ? pb - pa < na : pa - pb < nb;
}

// a double passed by value, its bits read back from memory (the argument itself is declared free of NaNs)
__attribute__((noinline)) void from_memory(const volatile double* in, double* out, int count) {
  for (int i = 0; i < count; ++i) out[i] = in[i];
}

}  // namespace

extern "C" {

int os2ru_abi_version(void) { return OS2R_UKF_ABI_VERSION; }

const char* os2ru_last_error(void) { return g_error.c_str(); }

int os2ru_ukf_points(const Os2rControlLayout* layout, int64_t nrobots, const void* x_dev, const void* p_dev, double gamma, void* points_dev,
                     int32_t* failed_dev, void* stream) {
  g_entry_point = "os2ru_ukf_points: ";
  if (const char* why = layout_refusal(layout)) return fail(OS2R_ERR_INVALID, why);
  const int n = 2 * layout->nq, S = 2 * n + 1;
  if (nrobots < 1) return fail(OS2R_ERR_INVALID, "nrobots must be >= 1");
  if (nrobots > 0x7fffffffll / (n * S)) return fail(OS2R_ERR_INVALID, "n * S * nrobots exceeds 2^31 - 1");
  if (!x_dev) return fail(OS2R_ERR_INVALID, "null x_dev");
  if (!p_dev) return fail(OS2R_ERR_INVALID, "null p_dev");
  if (!points_dev) return fail(OS2R_ERR_INVALID, "null points_dev");
  double gamma_value;
  {
    volatile double mem[1] = {gamma};
    from_memory(mem, &gamma_value, 1);
    if (!is_finite(&gamma_value)) return fail(OS2R_ERR_INVALID, "gamma must be finite");
    if (!(gamma_value > 0.0)) return fail(OS2R_ERR_INVALID, "gamma must be > 0");
  }
  {
    const size_t elem = layout->dtype == OS2R_F64 ? sizeof(double) : sizeof(float);
    const uintptr_t rows = (uintptr_t)n * (uintptr_t)nrobots * elem;
    if (overlap(points_dev, rows * S, x_dev, rows)) return fail(OS2R_ERR_INVALID, "points_dev overlaps x_dev");
    if (overlap(points_dev, rows * S, p_dev, rows * n)) return fail(OS2R_ERR_INVALID, "points_dev overlaps p_dev");
  }
  // the device, from here on
  if (const int rc = check_device(layout->device)) return rc;
  DeviceGuard guard(layout->device);
  auto launch = [&](auto real) {
    using T = decltype(real);
    UkfPointsArgs<T> p;
    std::memset(&p, 0, sizeof(p));
    p.x = (const T*)x_dev; p.p = (const T*)p_dev; p.points = (T*)points_dev; p.failed = failed_dev;
    p.M = nrobots;
    p.gamma = (T)gamma_value;
    return launched(launch_ukf_points<T>(layout->nq, p, (hipStream_t)stream));
  };
  return layout->dtype == OS2R_F64 ? launch(double()) : launch(float());
}

int os2ru_ukf_update(const Os2rControlLayout* layout, int64_t nrobots, const void* q_dev, const void* qd_dev, const uint8_t* done_dev,
                     const void* p_in_dev, const double* q_host, double gamma, double wm0, double wc0, double wi, const void* meas_dev,
                     const void* prec_dev, double gate, void* x_out_dev, void* p_out_dev, void* nis_dev, int32_t* used_dev,
                     int32_t* refused_dev, void* innov_dev, int32_t* lost_dev, void* points_out_dev, int32_t* failed_dev, void* stream) {
  g_entry_point = "os2ru_ukf_update: ";
  if (const char* why = layout_refusal(layout)) return fail(OS2R_ERR_INVALID, why);
  if (const char* why = slots_refusal(layout)) return fail(OS2R_ERR_INVALID, why);   // (slot_col picks rows of P in LDS)
  const int n = 2 * layout->nq, S = 2 * n + 1;
  if (nrobots < 1) return fail(OS2R_ERR_INVALID, "nrobots must be >= 1");
  if (nrobots > 0x7fffffffll / (n * S)) return fail(OS2R_ERR_INVALID, "n * S * nrobots exceeds 2^31 - 1");
  if (!q_dev) return fail(OS2R_ERR_INVALID, "null q_dev");
  if (!qd_dev) return fail(OS2R_ERR_INVALID, "null qd_dev");
  if (!p_in_dev) return fail(OS2R_ERR_INVALID, "null p_in_dev");
  if (!q_host) return fail(OS2R_ERR_INVALID, "null q_host");
  if (!meas_dev) return fail(OS2R_ERR_INVALID, "null meas_dev");
  if (!prec_dev) return fail(OS2R_ERR_INVALID, "null prec_dev");
  if (!x_out_dev) return fail(OS2R_ERR_INVALID, "null x_out_dev");
  if (!p_out_dev) return fail(OS2R_ERR_INVALID, "null p_out_dev");
  if (failed_dev && !points_out_dev) return fail(OS2R_ERR_INVALID, "failed_dev needs points_out_dev");
  if (!all_finite(q_host, n * n)) return fail(OS2R_ERR_INVALID, "Q must be finite");
  if (!symmetric(q_host, n)) return fail(OS2R_ERR_INVALID, "Q must be exactly symmetric");
  double sc[5];   // gamma, wm0, wc0, wi, gate
  {
    volatile double mem[5] = {gamma, wm0, wc0, wi, gate};
    from_memory(mem, sc, 5);
    if (!is_finite(&sc[0])) return fail(OS2R_ERR_INVALID, "gamma must be finite");
    if (!is_finite(&sc[1])) return fail(OS2R_ERR_INVALID, "wm0 must be finite");
    if (!is_finite(&sc[2])) return fail(OS2R_ERR_INVALID, "wc0 must be finite");
    if (!is_finite(&sc[3])) return fail(OS2R_ERR_INVALID, "wi must be finite");
    if (!(sc[0] > 0.0)) return fail(OS2R_ERR_INVALID, "gamma must be > 0");
    if (!(sc[3] > 0.0)) return fail(OS2R_ERR_INVALID, "wi must be > 0");
    if (!is_finite(&sc[4])) return fail(OS2R_ERR_INVALID, "gate must be finite");
    if (sc[4] < 0.0) return fail(OS2R_ERR_INVALID, "gate must be >= 0");
  }
  {
    const size_t elem = layout->dtype == OS2R_F64 ? sizeof(double) : sizeof(float);
    const uintptr_t rows = (uintptr_t)n * (uintptr_t)nrobots * elem, half = rows / 2 * S;
    if (p_in_dev != p_out_dev && overlap(p_out_dev, rows * n, p_in_dev, rows * n))
      return fail(OS2R_ERR_INVALID, "p_out_dev overlaps p_in_dev without being it");
    if (points_out_dev && overlap(points_out_dev, rows * S, q_dev, half)) return fail(OS2R_ERR_INVALID, "points_out_dev overlaps q_dev");
    if (points_out_dev && overlap(points_out_dev, rows * S, qd_dev, half)) return fail(OS2R_ERR_INVALID, "points_out_dev overlaps qd_dev");
  }
  // the device, from here on
  if (const int rc = check_device(layout->device)) return rc;
  DeviceGuard guard(layout->device);
  auto launch = [&](auto real) {
    using T = decltype(real);
    UkfArgs<T> p;
    std::memset(&p, 0, sizeof(p));
    p.q = (const T*)q_dev; p.qd = (const T*)qd_dev; p.done = done_dev; p.p_in = (const T*)p_in_dev; p.meas = (const T*)meas_dev;
    p.prec = (const T*)prec_dev; p.x_out = (T*)x_out_dev; p.p_out = (T*)p_out_dev; p.nis = (T*)nis_dev; p.used = used_dev;
    p.refused = refused_dev; p.innov = (T*)innov_dev; p.lost = lost_dev; p.points = (T*)points_out_dev; p.failed = failed_dev;
    p.M = nrobots; p.D = layout->obs_dim;
    for (int d = 0; d < OS2R_MAX_OBS; ++d) p.slot_col[d] = d < layout->obs_dim ? layout->slot_col[d] : -1;
    // rounded once to the dtype; a gate above its largest finite number is that number
    p.gate = sizeof(T) == sizeof(float) && sc[4] > (double)FLT_MAX ? (T)FLT_MAX : (T)sc[4];
    p.gamma = (T)sc[0]; p.wm0 = (T)sc[1]; p.wc0 = (T)sc[2]; p.wi = (T)sc[3];
    for (int i = 0; i < n * n; ++i) p.qn[i] = (T)q_host[i];
    return launched(launch_ukf_update<T>(layout->nq, p, (hipStream_t)stream));
  };
  return layout->dtype == OS2R_F64 ? launch(double()) : launch(float());
}

}  // extern "C"
