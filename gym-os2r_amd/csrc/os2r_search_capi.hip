// os2r_search_capi.hip — the C-ABI of libos2r_search.so (include/os2r_search.h): the entry point's own argument checks and the launch; the
// checks of the layout, the device guard, the gfx950 check and the calling thread's error text are os2r_host.hpp's.  Every
// argument check runs before the first HIP call.
#include "os2r_search.hpp"

#define OS2R_HOST_ERROR_PREFIX "os2rs_ilqr_line_search: "
#include "os2r_host.hpp"

using namespace os2r;

extern "C" {

int os2rs_abi_version(void) { return OS2R_SEARCH_ABI_VERSION; }

const char* os2rs_last_error(void) { return g_error.c_str(); }

int os2rs_ilqr_line_search(const Os2rControlLayout* layout, int32_t nknots, int64_t ntraj, int32_t nalpha, uint32_t flags,
                           const void* knot_obs_dev, const void* end_obs_dev, const void* act_dev, const uint8_t* done_dev,
                           const void* target_dev, const double* q_host, const double* r_host, const double* qf_host, void* cost_dev,
                           void* act_nom_dev, void* obs_nom_dev, void* end_nom_dev, void* lx_dev, void* lu_dev, void* pvec_final_dev,
                           int32_t* choice_dev, int32_t* index_dev, void* cand_cost_dev, void* stream) {
  if (const char* why = layout_refusal(layout)) return fail(OS2R_ERR_INVALID, why);
  if (const char* why = slots_refusal(layout)) return fail(OS2R_ERR_INVALID, why);
  const int n = 2 * layout->nq;
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
  auto launch = [&](auto real) {
    using T = decltype(real);
    SearchArgs<T> p;
    std::memset(&p, 0, sizeof(p));
    p.knot_obs = (const T*)knot_obs_dev; p.end_obs = (const T*)end_obs_dev; p.act = (const T*)act_dev; p.done = done_dev;
    p.target = (const T*)target_dev;
    p.cost = (T*)cost_dev; p.act_nom = (T*)act_nom_dev; p.obs_nom = (T*)obs_nom_dev; p.end_nom = (T*)end_nom_dev;
    p.lx = (T*)lx_dev; p.lu = (T*)lu_dev; p.pvec_final = (T*)pvec_final_dev;
    p.choice = choice_dev; p.index = index_dev; p.cand_cost = (T*)cand_cost_dev;
    p.M = ntraj; p.K = nknots; p.D = layout->obs_dim; p.nalpha = nalpha;
    p.accept_always = (flags & OS2RS_ACCEPT_ALWAYS) ? 1 : 0;
    // the lowest raw slot that shows each state column
    for (int col = 0; col < kLqrMaxN; ++col) p.col_slot[col] = -1;
    for (int d = layout->obs_dim - 1; d >= 0; --d)
      if (layout->slot_col[d] >= 0) p.col_slot[layout->slot_col[d]] = d;
    p.r00 = (T)r_host[0]; p.r01 = (T)r_host[1]; p.r11 = (T)r_host[3];
    const double* qf = qf_host ? qf_host : q_host;
    for (int i = 0; i < n * n; ++i) {
      p.q[i] = (T)q_host[i];
      p.qf[i] = (T)qf[i];
    }
    return launched(launch_ilqr_line_search<T>(layout->nq, p, (hipStream_t)stream));
  };
  return layout->dtype == OS2R_F64 ? launch(double()) : launch(float());
}

}  // extern "C"
