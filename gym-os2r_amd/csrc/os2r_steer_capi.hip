// os2r_steer_capi.hip — the C-ABI of libos2r_steer.so (include/os2r_steer.h): the entry points' own argument checks and the launches; the
// checks of the layout, the device guard, the gfx950 check and the calling thread's error text are os2r_host.hpp's.  Every
// argument check runs before the first HIP call.
#include "os2r_ilqr_mu.hpp"
#include "os2r_steer.hpp"

// two entry points, two prefixes: each names itself here on entry, and os2r_host.hpp's fail() puts that name in front
namespace {
thread_local const char* g_entry_point = "";
}
#define OS2R_HOST_ERROR_PREFIX g_entry_point
#include "os2r_host.hpp"

using namespace os2r;

extern "C" {

int os2rt_abi_version(void) { return OS2R_STEER_ABI_VERSION; }

const char* os2rt_last_error(void) { return g_error.c_str(); }

int os2rt_ilqr_backward_mu(const Os2rControlLayout* layout, int32_t nknots, int64_t ntraj, const void* a_dev, const void* b_dev,
                           const void* lx_dev, const void* lu_dev, const double* q_host, const double* r_host, const void* mu_dev,
                           const void* pmat_final_dev, const void* pvec_final_dev, void* gain_dev, void* ff_dev, void* pmat_out_dev,
                           void* pvec_out_dev, uint8_t* flag_dev, void* dv_dev, const void* actions_dev, const void* obs_dev,
                           const double* alpha_host, int32_t nalpha, void* weights_dev, void* stream) {
  g_entry_point = "os2rt_ilqr_backward_mu: ";
  if (const char* why = layout_refusal(layout)) return fail(OS2R_ERR_INVALID, why);
  if (nknots < 1) return fail(OS2R_ERR_INVALID, "nknots must be >= 1");
  if (ntraj < 1) return fail(OS2R_ERR_INVALID, "ntraj must be >= 1");
  if (ntraj > (int64_t)kLqrEnvs * 0x7fffffffll) return fail(OS2R_ERR_INVALID, "ntraj exceeds what one launch covers");
  if (!a_dev) return fail(OS2R_ERR_INVALID, "null a_dev");
  if (!b_dev) return fail(OS2R_ERR_INVALID, "null b_dev");
  if (!q_host) return fail(OS2R_ERR_INVALID, "null q_host");
  if (!r_host) return fail(OS2R_ERR_INVALID, "null r_host");
  if (!mu_dev) return fail(OS2R_ERR_INVALID, "null mu_dev");
  const int n = 2 * layout->nq;
  if (!all_finite(q_host, n * n)) return fail(OS2R_ERR_INVALID, "Q must be finite");
  if (!all_finite(r_host, 4)) return fail(OS2R_ERR_INVALID, "R must be finite");
  if (!symmetric(q_host, n)) return fail(OS2R_ERR_INVALID, "Q must be exactly symmetric");
  if (!symmetric(r_host, 2)) return fail(OS2R_ERR_INVALID, "R must be exactly symmetric");
  if (!gain_dev && !ff_dev && !pmat_out_dev && !pvec_out_dev && !dv_dev && !weights_dev)
    return fail(OS2R_ERR_INVALID, "all outputs are null (gain, ff, pmat_out, pvec_out, dv, weights)");
  if (weights_dev) {
    if (!actions_dev || !obs_dev || !alpha_host) return fail(OS2R_ERR_INVALID, "weights need actions_dev, obs_dev and alpha_host");
    if (nalpha < 1 || nalpha > OS2RC_MAX_ALPHAS) return fail(OS2R_ERR_INVALID, "nalpha must be 1..16");
    if (!all_finite(alpha_host, nalpha)) return fail(OS2R_ERR_INVALID, "alpha must be finite");
    if (const char* why = slots_refusal(layout)) return fail(OS2R_ERR_INVALID, why);
  }
  // the device, from here on
  if (const int rc = check_device(layout->device)) return rc;
  DeviceGuard guard(layout->device);
  auto launch = [&](auto real) {
    using T = decltype(real);
    IlqrMuArgs<T> pm;
    std::memset(&pm, 0, sizeof(pm));
    IlqrArgs<T>& p = pm.base;
    p.a = (const T*)a_dev; p.b = (const T*)b_dev; p.lx = (const T*)lx_dev; p.lu = (const T*)lu_dev;
    p.pmat_final = (const T*)pmat_final_dev; p.pvec_final = (const T*)pvec_final_dev; p.pmat_out = (T*)pmat_out_dev; p.pvec_out = (T*)pvec_out_dev;
    p.gain = (T*)gain_dev; p.ff = (T*)ff_dev; p.flag = flag_dev; p.dv = (T*)dv_dev;
    p.M = ntraj; p.K = nknots;
    for (int d = 0; d < OS2R_MAX_OBS; ++d) p.slot_col[d] = -1;
    if (weights_dev) {
      p.actions = (const T*)actions_dev; p.obs = (const T*)obs_dev; p.weights = (T*)weights_dev;
      p.D = layout->obs_dim; p.nalpha = nalpha;
      for (int d = 0; d < p.D; ++d) p.slot_col[d] = layout->slot_col[d];
      for (int i = 0; i < nalpha; ++i) p.alpha[i] = (T)alpha_host[i];
    }
    p.r00 = (T)r_host[0]; p.r01 = (T)r_host[1]; p.r11 = (T)r_host[3];
    for (int i = 0; i < n * n; ++i) p.q[i] = (T)q_host[i];
    pm.mu = (const T*)mu_dev;
    return launched(launch_ilqr_backward_mu<T>(layout->nq, pm, (hipStream_t)stream));
  };
  return layout->dtype == OS2R_F64 ? launch(double()) : launch(float());
}

int os2rt_ilqr_steer(const Os2rControlLayout* layout, int32_t nknots, int64_t ntraj, int32_t nalpha, const void* knot_obs_dev,
                     const void* end_obs_dev, const void* act_dev, const uint8_t* done_dev, const void* target_dev, const double* q_host,
                     const double* r_host, const double* qf_host, const void* dv_dev, const double* alpha_host,
                     const Os2rSteerRule* rule_host, void* cost_dev, void* act_nom_dev, void* obs_nom_dev, void* end_nom_dev, void* lx_dev,
                     void* lu_dev, void* pvec_final_dev, void* mu_dev, int32_t* status_dev, int32_t* iters_dev, int32_t* choice_dev,
                     int32_t* index_dev, void* cand_cost_dev, void* stream) {
  g_entry_point = "os2rt_ilqr_steer: ";
  if (const char* why = layout_refusal(layout)) return fail(OS2R_ERR_INVALID, why);
  if (const char* why = slots_refusal(layout)) return fail(OS2R_ERR_INVALID, why);
  const int n = 2 * layout->nq;
  if (nknots < 1) return fail(OS2R_ERR_INVALID, "nknots must be >= 1");
  if (ntraj < 1) return fail(OS2R_ERR_INVALID, "ntraj must be >= 1");
  if (nalpha < 1 || nalpha > OS2RC_MAX_ALPHAS) return fail(OS2R_ERR_INVALID, "nalpha must be 1..16");
  if (ntraj > 0x7fffffffll / ((int64_t)nknots * nalpha))
    return fail(OS2R_ERR_INVALID, "nknots * nalpha * ntraj exceeds 2^31 - 1 (index_dev is int32)");
  if (!knot_obs_dev) return fail(OS2R_ERR_INVALID, "null knot_obs_dev");
  if (!end_obs_dev) return fail(OS2R_ERR_INVALID, "null end_obs_dev");
  if (!act_dev) return fail(OS2R_ERR_INVALID, "null act_dev");
  if (!target_dev) return fail(OS2R_ERR_INVALID, "null target_dev");
  if (!q_host) return fail(OS2R_ERR_INVALID, "null q_host");
  if (!r_host) return fail(OS2R_ERR_INVALID, "null r_host");
  if (!dv_dev) return fail(OS2R_ERR_INVALID, "null dv_dev");
  if (!alpha_host) return fail(OS2R_ERR_INVALID, "null alpha_host");
  if (!rule_host) return fail(OS2R_ERR_INVALID, "null rule_host");
  if (!cost_dev) return fail(OS2R_ERR_INVALID, "null cost_dev");
  if (!mu_dev) return fail(OS2R_ERR_INVALID, "null mu_dev");
  if (!status_dev) return fail(OS2R_ERR_INVALID, "null status_dev");
  if (!choice_dev) return fail(OS2R_ERR_INVALID, "null choice_dev");
  if (!all_finite(q_host, n * n)) return fail(OS2R_ERR_INVALID, "Q must be finite");
  if (!all_finite(r_host, 4)) return fail(OS2R_ERR_INVALID, "R must be finite");
  if (qf_host && !all_finite(qf_host, n * n)) return fail(OS2R_ERR_INVALID, "Qf must be finite");
  if (!symmetric(q_host, n)) return fail(OS2R_ERR_INVALID, "Q must be exactly symmetric");
  if (!symmetric(r_host, 2)) return fail(OS2R_ERR_INVALID, "R must be exactly symmetric");
  if (qf_host && !symmetric(qf_host, n)) return fail(OS2R_ERR_INVALID, "Qf must be exactly symmetric");
  if (!all_finite(alpha_host, nalpha)) return fail(OS2R_ERR_INVALID, "alpha must be finite");
  // the rule: seven doubles in the caller's memory
  if (!all_finite(&rule_host->armijo, 7)) return fail(OS2R_ERR_INVALID, "every member of the rule must be finite");
  if (rule_host->armijo < 0.0) return fail(OS2R_ERR_INVALID, "rule armijo must be >= 0");
  if (rule_host->shrink < 0.0 || rule_host->shrink > 1.0) return fail(OS2R_ERR_INVALID, "rule shrink must be 0..1");
  if (rule_host->grow < 1.0) return fail(OS2R_ERR_INVALID, "rule grow must be >= 1");
  if (rule_host->mu_floor < 0.0) return fail(OS2R_ERR_INVALID, "rule mu_floor must be >= 0");
  if (rule_host->mu_start <= 0.0) return fail(OS2R_ERR_INVALID, "rule mu_start must be > 0");
  if (rule_host->mu_max < rule_host->mu_start) return fail(OS2R_ERR_INVALID, "rule mu_max must be >= mu_start");
  if (rule_host->tol < 0.0) return fail(OS2R_ERR_INVALID, "rule tol must be >= 0");
  // the device, from here on
  if (const int rc = check_device(layout->device)) return rc;
  DeviceGuard guard(layout->device);
  auto launch = [&](auto real) {
    using T = decltype(real);
    SteerArgs<T> s;
    std::memset(&s, 0, sizeof(s));
    SearchArgs<T>& p = s.base;
    p.knot_obs = (const T*)knot_obs_dev; p.end_obs = (const T*)end_obs_dev; p.act = (const T*)act_dev; p.done = done_dev;
    p.target = (const T*)target_dev;
    p.cost = (T*)cost_dev; p.act_nom = (T*)act_nom_dev; p.obs_nom = (T*)obs_nom_dev; p.end_nom = (T*)end_nom_dev;
    p.lx = (T*)lx_dev; p.lu = (T*)lu_dev; p.pvec_final = (T*)pvec_final_dev;
    p.choice = choice_dev; p.index = index_dev; p.cand_cost = (T*)cand_cost_dev;
    p.M = ntraj; p.K = nknots; p.D = layout->obs_dim; p.nalpha = nalpha;
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
    s.dv = (const T*)dv_dev; s.mu = (T*)mu_dev; s.status = status_dev; s.iters = iters_dev;
    s.armijo = (T)rule_host->armijo; s.shrink = (T)rule_host->shrink; s.grow = (T)rule_host->grow;
    s.mu_floor = (T)rule_host->mu_floor; s.mu_start = (T)rule_host->mu_start; s.mu_max = (T)rule_host->mu_max; s.tol = (T)rule_host->tol;
    for (int i = 0; i < nalpha; ++i) s.alpha[i] = (T)alpha_host[i];
    return launched(launch_ilqr_steer<T>(layout->nq, s, (hipStream_t)stream));
  };
  return layout->dtype == OS2R_F64 ? launch(double()) : launch(float());
}

}  // extern "C"
