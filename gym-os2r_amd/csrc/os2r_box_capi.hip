// os2r_box_capi.hip — the C-ABI of libos2r_box.so (include/os2r_box.h): the entry point's own argument checks and the launch; the
// checks of the layout, the device guard, the gfx950 check and the calling thread's error text are os2r_host.hpp's.  Every
// argument check runs before the first HIP call.
#include "os2r_ilqr_box.hpp"

#define OS2R_HOST_ERROR_PREFIX "os2rb_ilqr_backward_box: "
#include "os2r_host.hpp"

using namespace os2r;

namespace {

// the bits of a bound of the caller's, read from memory as an integer (os2r_host.hpp: is_finite)
__attribute__((noinline)) uint64_t bits_of(const double* x) {
  uint64_t b;
  std::memcpy(&b, x, sizeof(b));
  return b;
}

constexpr uint64_t kPlusInf = 0x7ff0000000000000ull, kMinusInf = 0xfff0000000000000ull;

}  // namespace

extern "C" {

int os2rb_abi_version(void) { return OS2R_BOX_ABI_VERSION; }

const char* os2rb_last_error(void) { return g_error.c_str(); }

int os2rb_ilqr_backward_box(const Os2rControlLayout* layout, int32_t nknots, int64_t ntraj, const void* a_dev, const void* b_dev,
                            const void* lx_dev, const void* lu_dev, const double* q_host, const double* r_host, double mu, const void* mu_dev,
                            const double* lo_host, const double* hi_host, const void* pmat_final_dev, const void* pvec_final_dev,
                            void* gain_dev, void* ff_dev, void* pmat_out_dev, void* pvec_out_dev, uint8_t* flag_dev, void* dv_dev,
                            uint8_t* clamp_dev, const void* actions_dev, const void* obs_dev, const double* alpha_host, int32_t nalpha,
                            void* weights_dev, void* stream) {
  if (const char* why = layout_refusal(layout)) return fail(OS2R_ERR_INVALID, why);
  if (nknots < 1) return fail(OS2R_ERR_INVALID, "nknots must be >= 1");
  if (ntraj < 1) return fail(OS2R_ERR_INVALID, "ntraj must be >= 1");
  if (ntraj > (int64_t)kLqrEnvs * 0x7fffffffll) return fail(OS2R_ERR_INVALID, "ntraj exceeds what one launch covers");
  if (!a_dev) return fail(OS2R_ERR_INVALID, "null a_dev");
  if (!b_dev) return fail(OS2R_ERR_INVALID, "null b_dev");
  if (!q_host) return fail(OS2R_ERR_INVALID, "null q_host");
  if (!r_host) return fail(OS2R_ERR_INVALID, "null r_host");
  if (!actions_dev) return fail(OS2R_ERR_INVALID, "null actions_dev (the bounds are relative to the nominal actions)");
  if (!lo_host) return fail(OS2R_ERR_INVALID, "null lo_host");
  if (!hi_host) return fail(OS2R_ERR_INVALID, "null hi_host");
  const int n = 2 * layout->nq;
  if (!all_finite(q_host, n * n)) return fail(OS2R_ERR_INVALID, "Q must be finite");
  if (!all_finite(r_host, 4)) return fail(OS2R_ERR_INVALID, "R must be finite");
  if (!symmetric(q_host, n)) return fail(OS2R_ERR_INVALID, "Q must be exactly symmetric");
  if (!symmetric(r_host, 2)) return fail(OS2R_ERR_INVALID, "R must be exactly symmetric");
  {
    volatile double mu_mem = mu;   // (the argument itself is declared free of NaNs: its bits are read back from memory)
    const double mu_read = mu_mem;
    if (!is_finite(&mu_read)) return fail(OS2R_ERR_INVALID, "mu must be finite");
    if (mu_read < 0.0) return fail(OS2R_ERR_INVALID, "mu must be >= 0");
    if (mu_dev && mu_read != 0.0) return fail(OS2R_ERR_INVALID, "mu_dev and a nonzero mu are both given");
  }
  // the box: every class test on the bits, a comparison only between values found finite
  for (int c = 0; c < 2; ++c) {
    const uint64_t lo = bits_of(&lo_host[c]), hi = bits_of(&hi_host[c]);
    const bool lo_finite = is_finite(&lo_host[c]), hi_finite = is_finite(&hi_host[c]);
    if ((!lo_finite && (lo & ~(1ull << 63)) != kPlusInf) || (!hi_finite && (hi & ~(1ull << 63)) != kPlusInf))
      return fail(OS2R_ERR_INVALID, "a bound must not be NaN");
    if ((!lo_finite && lo != kMinusInf) || (!hi_finite && hi != kPlusInf))
      return fail(OS2R_ERR_INVALID, "lo_host must be -infinity or finite, hi_host +infinity or finite");
    if ((lo_finite && (lo_host[c] < -1.0 || lo_host[c] > 1.0)) || (hi_finite && (hi_host[c] < -1.0 || hi_host[c] > 1.0)))
      return fail(OS2R_ERR_INVALID, "a finite bound must lie in [-1, 1]");
    if (lo_finite && hi_finite && !(lo_host[c] < hi_host[c])) return fail(OS2R_ERR_INVALID, "lo must be < hi in both components");
  }
  if (!gain_dev && !ff_dev && !pmat_out_dev && !pvec_out_dev && !dv_dev && !weights_dev)
    return fail(OS2R_ERR_INVALID, "all outputs are null (gain, ff, pmat_out, pvec_out, dv, weights)");
  if (weights_dev) {
    if (!obs_dev || !alpha_host) return fail(OS2R_ERR_INVALID, "weights need actions_dev, obs_dev and alpha_host");
    if (nalpha < 1 || nalpha > OS2RC_MAX_ALPHAS) return fail(OS2R_ERR_INVALID, "nalpha must be 1..16");
    if (!all_finite(alpha_host, nalpha)) return fail(OS2R_ERR_INVALID, "alpha must be finite");
    if (const char* why = slots_refusal(layout)) return fail(OS2R_ERR_INVALID, why);
  }
  // the device, from here on
  if (const int rc = check_device(layout->device)) return rc;
  DeviceGuard guard(layout->device);
  auto launch = [&](auto real) {
    using T = decltype(real);
    IlqrBoxArgs<T> pm;
    std::memset(&pm, 0, sizeof(pm));
    IlqrArgs<T>& p = pm.base;
    p.a = (const T*)a_dev; p.b = (const T*)b_dev; p.lx = (const T*)lx_dev; p.lu = (const T*)lu_dev;
    p.pmat_final = (const T*)pmat_final_dev; p.pvec_final = (const T*)pvec_final_dev; p.pmat_out = (T*)pmat_out_dev; p.pvec_out = (T*)pvec_out_dev;
    p.gain = (T*)gain_dev; p.ff = (T*)ff_dev; p.flag = flag_dev; p.dv = (T*)dv_dev;
    p.actions = (const T*)actions_dev;
    p.M = ntraj; p.K = nknots;
    for (int d = 0; d < OS2R_MAX_OBS; ++d) p.slot_col[d] = -1;
    if (weights_dev) {
      p.obs = (const T*)obs_dev; p.weights = (T*)weights_dev;
      p.D = layout->obs_dim; p.nalpha = nalpha;
      for (int d = 0; d < p.D; ++d) p.slot_col[d] = layout->slot_col[d];
      for (int i = 0; i < nalpha; ++i) p.alpha[i] = (T)alpha_host[i];
    }
    p.r00 = (T)r_host[0]; p.r01 = (T)r_host[1]; p.r11 = (T)r_host[3]; p.mu = (T)mu;
    for (int i = 0; i < n * n; ++i) p.q[i] = (T)q_host[i];
    pm.mu = (const T*)mu_dev; pm.clamp = clamp_dev;
    for (int c = 0; c < 2; ++c) {
      pm.lo[c] = (T)lo_host[c];
      pm.hi[c] = (T)hi_host[c];
    }
    return launched(launch_ilqr_backward_box<T>(layout->nq, pm, (hipStream_t)stream));
  };
  return layout->dtype == OS2R_F64 ? launch(double()) : launch(float());
}

}  // extern "C"
