// os2r_capi.hip — implementation of the C-ABI declared in include/os2r.h.
//
// Host-side only: owns the device buffers of one simulator handle, converts the
// host config into the uniform device structs, and launches the kernels of
// os2r_kernels.hpp on the caller's stream.  Nothing here computes physics on the
// CPU; a missing GPU is an error (OS2R_ERR_NO_DEVICE), never a fallback.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <deque>
#include <mutex>
#include <string>
#include <vector>

#include "os2r_host.hpp"
#include "os2r_kernels.hpp"
#include "os2r_lqr.hpp"
#include "../../include/os2r_record.h"

using namespace os2r;

namespace os2r {
int static_model_id(const Os2rModel& m);
bool same_model(const Os2rModel& a, const Os2rModel& b);
}

// model-specialised code objects registered by the host binding (include/os2r.h)
struct JitEntry {
  Os2rModel model;
  int dtype = 0, device = 0;
  hipModule_t module = nullptr;
  hipFunction_t fn[2][2][2] = {};   // [contact][per-env parameters][default sweep counts compiled in]
  // optional: contact + default sweep counts + the observation layout below folded in (os2r_jit_step_c1_d*_l)
  hipFunction_t fn_layout[2] = {};
  unsigned long long layout_kinds = 0, layout_srcs = 0;
  int layout_dim = -1;
  // optional, usually code objects of their own (csrc/os2r_jit_fused_unit.hip), by per-env parameters: the fused rollout and the
  // fused policy rollout (contact, default solver; os2r_jit_rollout_c1_d*, os2r_jit_policy_c1_d*) ...
  hipFunction_t fn_rollout[2] = {}, fn_policy[2] = {};
  // ... built for the observation layout below if the object announces one (fused_dim >= 0), else for any layout
  unsigned long long fused_kinds = 0, fused_srcs = 0;
  int fused_dim = -1;
  // os2r_jit_lin_c*_d* (_s): [contact][per-env parameters][default sweep counts compiled in], as fn
  hipFunction_t fn_lin[2][2][2] = {};
  // os2r_jit_policy_rec_c1_d*: the policy kernels that record the knots (os2rr_rollout_policy_recorded); kept only from an object
  // that announces the sink with the data symbol os2r_jit_policy_knots
  hipFunction_t fn_policy_rec[2] = {};
};
enum JitKind { kJitStep, kJitRollout, kJitPolicy, kJitLin };

static void task_layout(const Os2rTaskSpec& t, unsigned long long& kinds, unsigned long long& srcs, int& dim) {
  kinds = 0; srcs = 0; dim = t.obs_dim;
  for (int d = 0; d < t.obs_dim && d < OS2R_MAX_OBS; ++d) {
    kinds |= (unsigned long long)(t.obs_kind[d] & 15) << (4 * d);
    srcs |= (unsigned long long)(t.obs_src[d] & 15) << (4 * d);
  }
}

static std::mutex g_jit_mutex;
static std::deque<JitEntry> g_jit;   // entries are never removed: handles keep pointers into it

// newest registration of this robot that exports kernels of this kind for the handle's contact flag (a robot may have been
// registered once with and once without ground contact, and every kind is a code object of its own)
static const JitEntry* find_jit(const Os2rModel& m, int dtype, int device, bool contact, const Os2rTaskSpec& task, JitKind kind = kJitStep) {
  unsigned long long kinds, srcs;
  int dim;
  task_layout(task, kinds, srcs, dim);
  std::lock_guard<std::mutex> lock(g_jit_mutex);
  const JitEntry* any = nullptr;
  for (auto it = g_jit.rbegin(); it != g_jit.rend(); ++it) {
    if (it->dtype != dtype || it->device != device) continue;
    bool exports = false, mine = false;   // mine: built for this handle's observation layout
    if (kind == kJitStep) {
      exports = it->fn[contact][0][0] || it->fn[contact][1][0];
      mine = contact && it->layout_dim == dim && it->layout_kinds == kinds && it->layout_srcs == srcs;
    } else if (kind == kJitLin) {
      exports = it->fn_lin[contact][0][0] || it->fn_lin[contact][0][1] || it->fn_lin[contact][1][0] || it->fn_lin[contact][1][1];
      mine = true;   // (no epilogue, no layout)
    } else {
      const hipFunction_t* f = kind == kJitRollout ? it->fn_rollout : it->fn_policy;
      mine = it->fused_dim == dim && it->fused_kinds == kinds && it->fused_srcs == srcs;
      // a fused kernel with another task's layout folded in cannot serve this handle at all
      exports = contact && (f[0] || f[1]) && (it->fused_dim < 0 || mine);
    }
    if (!exports || !os2r::same_model(it->model, m)) continue;
    // a code object built for this handle's observation layout is preferred over a newer one built for another
    if (mine) return &*it;
    if (!any) any = &*it;
  }
  return any;
}

namespace {

thread_local std::string g_create_error;

struct SimBase {
  Os2rConfig cfg;
  std::string err;
  int nq = 0, D = 0;
  unsigned cmask = 0;
  int model_id = -1;  // matching constexpr model table, -1: run-time model kernels
  const JitEntry* jit = nullptr;  // registered model-specialised code object (os2r_register_model_kernels)
  // with it, where registered: the robot's fused rollout, fused policy rollout and linearize kernels (resolved at creation too)
  const JitEntry *jit_rollout = nullptr, *jit_policy = nullptr, *jit_lin = nullptr;
  bool dr = false;
  size_t esz = 8;
  unsigned long long step_count = 0;
  std::vector<void*> allocs;
  // device buffers (typed views below)
  void *model_d = nullptr, *task_d = nullptr;
  void *q = nullptr, *qd = nullptr, *hist = nullptr;
  void *mass_scale = nullptr, *damping = nullptr, *friction = nullptr, *mu = nullptr, *gravity = nullptr;
  int32_t* steps = nullptr;
  uint32_t* episode = nullptr;
  uint8_t* pose = nullptr;
  void* solver_l = nullptr;          // [4*nq][N]: the contact solver's state (os2r_get/set_solver_state)
  uint32_t* solver_flags = nullptr;  // [N]
  unsigned int* violations = nullptr;
  // scratch outputs for os2r_bench_steps
  void *b_obs = nullptr, *b_rew = nullptr, *b_term = nullptr;
  unsigned long long* counters = nullptr;   // caller-owned work-counter buffer (os2r_set_work_counters)
  uint8_t* b_done = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  uint16_t* reason = nullptr;           // caller-owned done-reason buffer (os2r_set_done_reasons)
  uint8_t* done_mask = nullptr;         // caller-owned done-mask buffer (os2r_set_done_mask)
  uint32_t* mirror_host = nullptr;      // two words of mapped, coherent host memory (os2r_get_violation_mirror) ...
  uint32_t* mirror_dev = nullptr;       // ... and the address the kernels write them through
  unsigned long long* debug = nullptr;  // diagnostic stamp builds only
  void* pol_act = nullptr;              // os2r_rollout_policy's launch loop: [N][2] actions, allocated on first use ...
  uint8_t* pol_open = nullptr;          // ... and [N] "still summing" flags
  void* copy_stage = nullptr;           // os2r_copy_envs within one handle: every copied row once, allocated on first use
};

}  // namespace

struct Os2rSim : SimBase {};

namespace {

#define HIP_TRY(sim, expr)                                                                     \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess) {                                                                    \
      (sim)->err = std::string(#expr) + ": " + hipGetErrorString(_e);                          \
      return OS2R_ERR_HIP;                                                                     \
    }                                                                                          \
  } while (0)

// The handle's arithmetic type, handed to `f` as a value of it: by_dtype(sim, [&](auto t) { return do_x<decltype(t)>(sim, ...); })
template <typename F>
int by_dtype(const Os2rSim* s, F&& f) { return s->cfg.dtype == OS2R_F64 ? f(double()) : f(float()); }

template <typename T>
void fill_model(const Os2rModel& m_in, bool contact, DevModel<T>& d) {
  Os2rModel m = m_in;
  if (!contact) m.ncand = 0;  // contact off: no candidates reach the kernels, whichever instantiation runs
  std::memset(&d, 0, sizeof(d));
  d.nq = m.nq;
  for (int i = 0; i < OS2R_MAX_DOF; ++i) {
    d.axis[i] = m.axis[i];
    for (int k = 0; k < 9; ++k) d.rfix[i][k] = (T)m.rfix[i][k];
    for (int k = 0; k < 3; ++k) { d.rpos[i][k] = (T)m.rpos[i][k]; d.com[i][k] = (T)m.com[i][k]; }
    for (int k = 0; k < 6; ++k) d.icom[i][k] = (T)m.icom[i][k];
    d.mass[i] = (T)m.mass[i];
    d.damping[i] = (T)m.damping[i];
    d.friction[i] = (T)m.friction[i];
    d.mu[i] = (T)m.mu[i];
  }
  for (int k = 0; k < 2; ++k) { d.act_dof[k] = m.act_dof[k]; d.max_torque[k] = (T)m.max_torque[k]; }
  d.gravity_z = (T)m.gravity_z;
  int k = 0;
  for (int b = 0; b < OS2R_MAX_DOF; ++b) {
    d.cand_begin[b] = k;
    while (k < m.ncand && m.cand_body[k] == b) ++k;
  }
  d.cand_begin[OS2R_MAX_DOF] = k;
  for (int c = 0; c < m.ncand; ++c)
    for (int j = 0; j < 3; ++j) d.cand_p[c][j] = (T)m.cand_p[c][j];
  for (int b = 0; b < OS2R_MAX_DOF; ++b) {
    for (int j = 0; j < 3; ++j) d.cand_center[b][j] = (T)m.cand_center[b][j];
    // a zero radius (model built without spheres) must never cull: make it cover everything
    d.cand_radius[b] = m.cand_radius[b] > 0.0 ? (T)(m.cand_radius[b] * 1.000001) : (T)1e30;
  }
}

// The done test of observe() is `x < done_lo || x > done_hi` on the pre-map value x.  done_lo / done_hi are exact
// f64 pre-images of the reference's test; in f32 they must decide what they decide in f64 for every float x:
// a bound rounded to nearest may land on the far side of a float the reference flags (the torque slots:
// -/+0.9999999999999998 -> -/+1.0f, and an action of exactly -/+1 no longer ends the episode).  So a bound rounds
// inward: done_lo up to the smallest float >= it, done_hi down to the largest float <= it.  Periodic slots are the
// exception: the f32 wrap_pi returns -pi_f (just below -pi) for x = +/-pi_f, inputs the reference keeps, so their
// bounds round outward instead, to keep the whole range of the f32 wrap [-pi_f, pi_f] inside.
inline float float_at_or_above(double v) {
  float f = (float)v;
  if ((double)f < v) f = std::nextafter(f, FLT_MAX);
  return f;
}
inline float float_at_or_below(double v) {
  float f = (float)v;
  if ((double)f > v) f = std::nextafter(f, -FLT_MAX);
  return f;
}
inline void done_bounds(int kind, double lo, double hi, double& dlo, double& dhi) { dlo = lo; dhi = hi; }
inline void done_bounds(int kind, double lo, double hi, float& dlo, float& dhi) {
  const bool periodic = kind == OS2R_OBS_POS_PERIODIC_NORM || kind == OS2R_OBS_POS_PERIODIC_RAW;
  dlo = periodic ? float_at_or_below(lo) : float_at_or_above(lo);
  dhi = periodic ? float_at_or_above(hi) : float_at_or_below(hi);
}

template <typename T>
void fill_task(const Os2rConfig& cfg, DevTask<T>& d) {
  const Os2rTaskSpec& t = cfg.task;
  std::memset(&d, 0, sizeof(d));
  d.obs_dim = t.obs_dim;
  for (int i = 0; i < OS2R_MAX_OBS; ++i) {
    d.obs_kind[i] = t.obs_kind[i];
    d.obs_src[i] = t.obs_src[i];
    d.obs_low[i] = (T)t.obs_low[i];
    d.obs_high[i] = (T)t.obs_high[i];
    done_bounds(t.obs_kind[i], t.done_lo[i], t.done_hi[i], d.done_lo[i], d.done_hi[i]);
  }
  d.reward_id = t.reward_id; d.normalized = t.normalized;
  d.idx_pitch_pos = t.idx_pitch_pos; d.idx_yaw_vel = t.idx_yaw_vel;
  d.idx_hip_pos = t.idx_hip_pos; d.idx_knee_pos = t.idx_knee_pos;
  d.max_episode_steps = t.max_episode_steps;
  d.reset_mode = t.reset_mode; d.n_reset_poses = t.n_reset_poses;
  for (int i = 0; i < OS2R_MAX_RESET_POSES; ++i) {
    d.reset_pose_id[i] = t.reset_pose_id[i]; d.reset_laying[i] = t.reset_laying[i];
    d.reset_pitch[i] = t.reset_pitch[i]; d.reset_hip[i] = t.reset_hip[i]; d.reset_knee[i] = t.reset_knee[i];
  }
  d.reset_simple = t.reset_simple;
  for (int i = 0; i < 6; ++i) d.leg_def[i] = t.leg_def[i];
  d.dof_yaw = t.dof_yaw; d.dof_pitch = t.dof_pitch; d.dof_bc = t.dof_bc; d.dof_hip = t.dof_hip; d.dof_knee = t.dof_knee;
  d.randomize_params = t.randomize_params;
  d.gravity_rollouts = t.gravity_rollouts;
  d.dr_gravity_mean = t.dr_gravity_mean; d.dr_gravity_std = t.dr_gravity_std;
  d.dr_mass_lo = t.dr_mass_lo; d.dr_mass_hi = t.dr_mass_hi;
  d.dr_friction_lo = t.dr_friction_lo; d.dr_friction_hi = t.dr_friction_hi;
  d.dr_damping_lo = t.dr_damping_lo; d.dr_damping_hi = t.dr_damping_hi;
  d.dr_mu_base = t.dr_mu_base; d.dr_mu_lo = t.dr_mu_lo; d.dr_mu_hi = t.dr_mu_hi;
  for (int i = 0; i < OS2R_MAX_DOF; ++i) d.nominal_damping[i] = cfg.model.damping[i];
}

int validate(const Os2rConfig* c, std::string& why) {
  if (!c) { why = "null config"; return 1; }
  // (ABI 6 added an entry point, not a field: configs stamped 5 are the same struct)
  if (c->abi_version != OS2R_ABI_VERSION && c->abi_version != 5) { why = "abi_version mismatch"; return 1; }
  if (c->dtype != OS2R_F32 && c->dtype != OS2R_F64) { why = "dtype must be OS2R_F32 or OS2R_F64"; return 1; }
  if (c->num_envs <= 0) { why = "num_envs must be positive"; return 1; }
  const Os2rModel& m = c->model;
  if (m.nq < 2 || m.nq > OS2R_MAX_DOF) { why = "model.nq must be 2..5"; return 1; }
  if (m.ncand < 0 || m.ncand > OS2R_MAX_CAND) { why = "model.ncand out of range"; return 1; }
  int last = 0;
  for (int k = 0; k < m.ncand; ++k) {
    if (m.cand_body[k] < last || m.cand_body[k] >= m.nq) { why = "cand_body must be non-decreasing and < nq"; return 1; }
    last = m.cand_body[k];
  }
  for (int i = 0; i < m.nq; ++i) {
    if (m.axis[i] < 0 || m.axis[i] > 2) { why = "joint axis must be 0,1,2"; return 1; }
    if (!is_finite(&m.mass[i]) || !(m.mass[i] > 0.0)) { why = "body mass must be positive and finite"; return 1; }
  }
  for (int k = 0; k < 2; ++k)
    if (m.act_dof[k] < 0 || m.act_dof[k] >= m.nq) { why = "act_dof out of range"; return 1; }
  const Os2rTaskSpec& t = c->task;
  if (t.obs_dim < 1 || t.obs_dim > OS2R_MAX_OBS) { why = "task.obs_dim out of range"; return 1; }
  for (int d = 0; d < t.obs_dim; ++d) {
    const int kind = t.obs_kind[d];
    if (kind < OS2R_OBS_POS_NORM || kind > OS2R_OBS_TORQUE_RAW) { why = "unknown obs kind"; return 1; }
    const bool tq = kind == OS2R_OBS_TORQUE_NORM || kind == OS2R_OBS_TORQUE_RAW;
    if (t.obs_src[d] < 0 || t.obs_src[d] >= (tq ? 2 : m.nq)) { why = "obs_src out of range"; return 1; }
  }
  if (t.reward_id < 0 || t.reward_id > OS2R_REWARD_STRAIGHT_V1) { why = "unknown reward id"; return 1; }
  if (t.reward_id != OS2R_REWARD_STRAIGHT_V1 && t.idx_pitch_pos < 0) { why = "reward needs the pitch position observed"; return 1; }
  if (t.reward_id == OS2R_REWARD_HOPPING_V1 && t.idx_yaw_vel < 0) { why = "HoppingV1 needs the yaw velocity observed"; return 1; }
  if (t.reward_id == OS2R_REWARD_STRAIGHT_V1 && (t.idx_hip_pos < 0 || t.idx_knee_pos < 0)) { why = "StraightV1 needs hip and knee positions"; return 1; }
  if (t.n_reset_poses < 1 || t.n_reset_poses > OS2R_MAX_RESET_POSES) { why = "n_reset_poses out of range"; return 1; }
  if (c->substeps < 1 || c->substeps > 1000) { why = "substeps out of range"; return 1; }
  if (!is_finite(&c->dt) || !(c->dt > 0.0)) { why = "dt must be positive and finite"; return 1; }
  if (c->pgs_iters < 0 || c->pgs_iters > 10000) { why = "pgs_iters out of range"; return 1; }
  if (!is_finite(&c->contact_margin) || !(c->contact_margin >= 0.0)) { why = "contact_margin must be >= 0 and finite"; return 1; }
  // erp and max_erv go into the right-hand side of every contact row; 0 is legal for both (no error reduction)
  if (!is_finite(&c->erp)) { why = "erp must be finite"; return 1; }
  if (!is_finite(&c->max_erv)) { why = "max_erv must be finite"; return 1; }
  if (!(c->max_erv >= 0.0)) { why = "max_erv must be >= 0"; return 1; }
  if (t.gravity_rollouts < 0) { why = "gravity_rollouts must be >= 0"; return 1; }
  if (c->pgs_normal_iters < 0 || c->pgs_normal_iters > 10000) { why = "pgs_normal_iters out of range"; return 1; }
  if (!is_finite(&c->pgs_tol) || !(c->pgs_tol >= 0.0)) { why = "pgs_tol must be >= 0 and finite"; return 1; }
  if (c->pgs_exact < 0 || c->pgs_exact > 10000) { why = "pgs_exact out of range"; return 1; }
  if (c->pgs_exact > 0 && c->dtype != OS2R_F64) { why = "pgs_exact (the exact finish of the contact solve) needs dtype f64"; return 1; }
  return 0;
}

template <typename T>
StepArgs<T> make_args(Os2rSim* s) {
  StepArgs<T> a;
  std::memset(&a, 0, sizeof(a));
  a.model = (const DevModel<T>*)s->model_d;
  a.task = (const DevTask<T>*)s->task_d;
  a.N = s->cfg.num_envs;
  a.env_offset = s->cfg.env_offset;
  a.seed = s->cfg.seed;
  a.step_count = s->step_count;
  a.substeps = s->cfg.substeps;
  a.rollout_steps = 0;
  a.pgs_iters = s->cfg.pgs_iters;
  a.pgs_normal_iters = s->cfg.pgs_normal_iters;
  a.pgs_exact = s->cfg.pgs_normal_iters > 0 ? s->cfg.pgs_exact : 0;   // the coupled pyramid has no fixed box to pivot on
  a.auto_reset = s->cfg.auto_reset;
  a.dt = (T)s->cfg.dt; a.erp = (T)s->cfg.erp; a.max_erv = (T)s->cfg.max_erv; a.margin = (T)s->cfg.contact_margin;
  a.gravity_z = (T)s->cfg.model.gravity_z;
  a.pgs_tol = (T)s->cfg.pgs_tol;
  a.counters = s->counters;
  a.q = (T*)s->q; a.qd = (T*)s->qd; a.hist = (T*)s->hist;
  a.mass_scale = (T*)s->mass_scale; a.damping = (T*)s->damping; a.friction = (T*)s->friction;
  a.mu = (T*)s->mu; a.gravity = (T*)s->gravity;
  a.steps = s->steps; a.episode = s->episode; a.pose = s->pose; a.violations = s->violations;
  a.solver_l = (T*)s->solver_l; a.solver_flags = s->solver_flags;
  a.debug = s->debug;
  a.reason = s->reason;
  a.done_mask = s->done_mask;
  a.mirror = s->mirror_dev;
  task_layout(s->cfg.task, a.layout_kinds, a.layout_srcs, a.layout_dim);
  return a;
}

template <typename T>
int do_reset(Os2rSim* s, const uint8_t* mask, void* obs, hipStream_t st) {
  StepArgs<T> a = make_args<T>(s);
  a.reset_mask = mask;
  a.obs = (T*)obs;
  if (Launcher<T>::reset(s->nq, s->dr, a, st) != 0) { s->err = "no reset kernel for this chain length"; return OS2R_ERR_INVALID; }
  HIP_TRY(s, hipGetLastError());
  return OS2R_OK;
}

// A kernel of a registered code object: one wave per 64 environments (times grid_y), `args` as the kernel-argument buffer
template <typename Args>
hipError_t jit_launch(hipFunction_t fn, const Args& a, long long N, unsigned grid_y, hipStream_t st) {
  Args args = a;
  size_t size = sizeof(args);
  void* extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &args, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
  return hipModuleLaunchKernel(fn, (unsigned)((N + kWave - 1) / kWave), grid_y, 1, kWave, 1, 1, 0, st, nullptr, extra);
}

// The fused kernel of a handle with a code object, out of fn_rollout / fn_policy of the entry resolved at creation: under the
// conditions the compiled-in robots have a fused variant (ground contact, default solver, no work counters), for the handle's
// per-env-parameter flag as it is now (os2r_set_params and os2r_copy_envs can switch it on); null: the launch loop
template <typename T>
hipFunction_t jit_fused_fn(const Os2rSim* s, const hipFunction_t* by_dr) {
  if (!s->jit || !by_dr || s->counters || !(s->cfg.contact != 0 && s->cmask != 0u)) return nullptr;
  const int exact = s->cfg.pgs_normal_iters > 0 ? s->cfg.pgs_exact : 0;   // (as make_args)
  if (!is_std_solver<T>(s->cfg.pgs_iters, s->cfg.pgs_normal_iters, exact, s->cfg.model.nq)) return nullptr;
  return by_dr[s->dr];
}

template <typename T>
int do_step(Os2rSim* s, const void* actions, void* obs, void* reward, uint8_t* done, void* term, hipStream_t st) {
  StepArgs<T> a = make_args<T>(s);
  a.actions = (const T*)actions; a.obs = (T*)obs; a.reward = (T*)reward; a.done = done; a.term_obs = (T*)term;
  const bool contact = s->cfg.contact != 0 && s->cmask != 0u;
  const bool std_sweeps = is_std_solver<T>(a.pgs_iters, a.pgs_normal_iters, a.pgs_exact, s->cfg.model.nq);
  hipFunction_t jit_fn = !s->jit ? nullptr
      : (std_sweeps && s->jit->fn[contact][s->dr][1]) ? s->jit->fn[contact][s->dr][1] : s->jit->fn[contact][s->dr][0];
  if (s->jit && contact && std_sweeps && s->jit->fn_layout[s->dr] && s->jit->layout_dim == a.layout_dim &&
      s->jit->layout_kinds == a.layout_kinds && s->jit->layout_srcs == a.layout_srcs)
    jit_fn = s->jit->fn_layout[s->dr];
  if (a.counters && jit_fn) { s->err = "no counting variant in run-time code objects"; return OS2R_ERR_INVALID; }
  if (jit_fn) {
    // the robot's own code object: same StepArgs, passed as the kernel-argument buffer
    HIP_TRY(s, jit_launch(jit_fn, a, a.N, 1, st));
  } else if (Launcher<T>::step(s->nq, s->model_id, s->cfg.contact != 0, s->dr, a, st) != 0) {
    s->err = a.counters ? "no counting variant of the step kernel for this configuration" : "no step kernel for this chain length / contact mask";
    return OS2R_ERR_INVALID;
  }
  HIP_TRY(s, hipGetLastError());
  s->step_count += 1;
  return OS2R_OK;
}

// K env-steps: one launch of a fused variant where one exists, K launches of the step kernel otherwise (same results)
template <typename T>
int do_rollout(Os2rSim* s, int K, const void* actions, void* obs, void* reward, uint8_t* done, void* term, uint16_t* reason,
               hipStream_t st) {
  const size_t N = (size_t)s->cfg.num_envs, D = (size_t)s->D;
  const hipFunction_t jit_fn = jit_fused_fn<T>(s, s->jit_rollout ? s->jit_rollout->fn_rollout : nullptr);
  if ((!s->jit || jit_fn) && !s->counters) {
    StepArgs<T> a = make_args<T>(s);
    a.actions = (const T*)actions; a.obs = (T*)obs; a.reward = (T*)reward; a.done = done; a.term_obs = (T*)term;
    a.reason = reason;
    a.done_mask = nullptr;   // (a rollout writes neither of the per-step buffers set on the handle)
    a.rollout_steps = K;
    int rc;
    if (jit_fn) {
      HIP_TRY(s, jit_launch(jit_fn, a, a.N, 1, st));
      rc = 0;
    } else {
      rc = Launcher<T>::step(s->nq, s->model_id, s->cfg.contact != 0, s->dr, a, st);
    }
    if (rc == 0) {
      HIP_TRY(s, hipGetLastError());
      s->step_count += (unsigned long long)K;
      return OS2R_OK;
    }
  }
  uint16_t* const reason_keep = s->reason;
  uint8_t* const mask_keep = s->done_mask;
  s->done_mask = nullptr;
  int rc = OS2R_OK;
  for (int k = 0; k < K && rc == OS2R_OK; ++k) {
    s->reason = reason ? reason + (size_t)k * N : nullptr;
    rc = do_step<T>(s, actions ? (const T*)actions + (size_t)k * N * 2 : nullptr, obs ? (T*)obs + (size_t)k * N * D : nullptr,
                    reward ? (T*)reward + (size_t)k * N : nullptr, done ? done + (size_t)k * N : nullptr,
                    term ? (T*)term + (size_t)k * N * D : nullptr, st);
  }
  s->reason = reason_keep;
  s->done_mask = mask_keep;
  return rc;
}

template <typename T>
int init_params(Os2rSim* s, hipStream_t st) {
  const long long N = s->cfg.num_envs;
  for (int i = 0; i < s->nq; ++i) {
    Launcher<T>::fill((T*)s->mass_scale + i * N, N, T(1), st);
    Launcher<T>::fill((T*)s->damping + i * N, N, (T)s->cfg.model.damping[i], st);
    Launcher<T>::fill((T*)s->friction + i * N, N, (T)s->cfg.model.friction[i], st);
    Launcher<T>::fill((T*)s->mu + i * N, N, (T)s->cfg.model.mu[i], st);
  }
  if (s->cfg.task.reset_mode == OS2R_RESET_RANDOM && s->cfg.task.dr_gravity_std > 0.0)
    Launcher<T>::gravity((T*)s->gravity, N, s->cfg.env_offset, s->cfg.seed, s->cfg.task.dr_gravity_mean,
                         s->cfg.task.dr_gravity_std, st);
  else
    Launcher<T>::fill((T*)s->gravity, N, (T)s->cfg.model.gravity_z, st);
  HIP_TRY(s, hipGetLastError());
  return OS2R_OK;
}

int dev_alloc(Os2rSim* s, void** p, size_t bytes) {
  hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess) { s->err = std::string("hipMalloc: ") + hipGetErrorString(e); return OS2R_ERR_ALLOC; }
  s->allocs.push_back(*p);
  e = hipMemset(*p, 0, bytes);
  if (e != hipSuccess) { s->err = std::string("hipMemset: ") + hipGetErrorString(e); return OS2R_ERR_HIP; }
  return OS2R_OK;
}

// the robot and the task in the handle's dtype, as the kernels read them
template <typename T>
int upload_model(Os2rSim* s) {
  DevModel<T> hm; DevTask<T> ht;
  fill_model(s->cfg.model, s->cfg.contact != 0, hm); fill_task(s->cfg, ht);
  int rc;
  if ((rc = dev_alloc(s, &s->model_d, sizeof(hm)))) return rc;
  if ((rc = dev_alloc(s, &s->task_d, sizeof(ht)))) return rc;
  if (hipMemcpy(s->model_d, &hm, sizeof(hm), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(s->task_d, &ht, sizeof(ht), hipMemcpyHostToDevice) != hipSuccess) { s->err = "model upload failed"; return OS2R_ERR_HIP; }
  return OS2R_OK;
}

// The rows `what` selects, as the copy kernel takes them: row r of an array of the source next to row r of the same array of the
// destination.  `stage` (the in-place case) stands in for the destination (to_stage) or for the source: it holds every row
// once, [row][num_envs of the handle], the 32-bit rows and the pose bytes behind the rows of the handle's dtype.
template <typename T>
CopyArgs<T> copy_rows(Os2rSim* d, Os2rSim* s, int what, void* stage, bool to_stage) {
  CopyArgs<T> a;
  std::memset(&a, 0, sizeof(a));
  const long long Nd = d->cfg.num_envs, Ns = s->cfg.num_envs;
  a.Nd = Nd; a.Ns = Ns; a.gather = 1;
  const int nq = d->nq;
  T* const stage_t = (T*)stage;
  uint32_t* const stage_w = (uint32_t*)(stage_t + (size_t)(10 * nq + 5) * (size_t)Nd);
  auto rows = [&](const void* sp, void* dp, int count) {
    for (int r = 0; r < count; ++r, ++a.nrows) {
      a.src[a.nrows] = stage && !to_stage ? stage_t + (size_t)a.nrows * Nd : (const T*)sp + (size_t)r * Ns;
      a.dst[a.nrows] = stage && to_stage ? stage_t + (size_t)a.nrows * Nd : (T*)dp + (size_t)r * Nd;
    }
  };
  auto words = [&](const void* sp, void* dp) {
    a.src32[a.nwords] = stage && !to_stage ? stage_w + (size_t)a.nwords * Nd : (const uint32_t*)sp;
    a.dst32[a.nwords] = stage && to_stage ? stage_w + (size_t)a.nwords * Nd : (uint32_t*)dp;
    ++a.nwords;
  };
  if (what & OS2R_COPY_STATE) {
    rows(s->q, d->q, nq); rows(s->qd, d->qd, nq); rows(s->hist, d->hist, 4); rows(s->solver_l, d->solver_l, 4 * nq);
    words(s->solver_flags, d->solver_flags); words(s->steps, d->steps); words(s->episode, d->episode);
    uint8_t* const stage_b = (uint8_t*)(stage_w + 3 * (size_t)Nd);
    a.src8 = stage && !to_stage ? stage_b : s->pose;
    a.dst8 = stage && to_stage ? stage_b : d->pose;
  }
  if (what & OS2R_COPY_PARAMS) {
    rows(s->mass_scale, d->mass_scale, nq); rows(s->damping, d->damping, nq); rows(s->friction, d->friction, nq);
    rows(s->mu, d->mu, nq); rows(s->gravity, d->gravity, 1);
  }
  return a;
}

// os2rr_rollout_policy_recorded: where the knots of a policy rollout go
struct KnotSink {
  Os2rSim* knots;   // nullable
  int first_knot, what;
  void* obs;        // nullable, [K][N][D]
};

// do_copy's rule for the destination of a parameter copy: from a source with per-environment parameters (or another gravity) it
// reads its parameter arrays per lane from now on
inline void knots_read_params(Os2rSim* kn, const Os2rSim* s, const KnotSink* sink) {
  if (kn && (sink->what & OS2R_COPY_PARAMS) && (s->dr || s->cfg.model.gravity_z != kn->cfg.model.gravity_z)) kn->dr = true;
}

// K env-steps with the linear policy in the loop: one launch of the fused kernel where os2r_rollout has a fused variant;
// otherwise per env-step the policy kernel (state -> observation -> actions), the step launch with those actions and the
// accumulation of the step's reward and done flag (same results)
// (os2rr_rollout_policy_recorded: with `sink` the environments of the top of env-step k go to lanes (first_knot + k) N .. of
// sink->knots and their observations to sink->obs -- by the fused kernel itself, or in the launch loop by one copy launch per
// env-step and the policy kernel)
template <typename T>
int do_rollout_policy(Os2rSim* s, int K, const void* w, int flags, void* ret, int32_t* len, void* obs, void* reward, uint8_t* done,
                      void* term, uint16_t* reason, hipStream_t st, const void* sigma = nullptr, uint32_t salt = 0u,
                      void* act_out = nullptr, void* eps_out = nullptr, int period = 0, int first_slot = 0,
                      const KnotSink* sink = nullptr) {
  const size_t N = (size_t)s->cfg.num_envs, D = (size_t)s->D;
  PolicyArgs<T> p;
  std::memset(&p, 0, sizeof(p));
  p.w = (const T*)w; p.flags = flags; p.ret = (T*)ret; p.len = len;
  // exploration noise (os2r_rollout_policy_noisy): a null sigma is the deterministic policy
  p.sigma = (const T*)sigma; p.salt = salt; p.act_out = (T*)act_out; p.eps_out = (T*)eps_out;
  // time schedule (os2r_rollout_policy_scheduled): period 0 is the one set of the two entry points above
  p.period = period; p.first_slot = first_slot;
  // (a recorded call takes the recording kernels of the policy object; one that has none -- it would take the appended arguments
  // and record nothing -- leaves the call to the launch loop)
  const hipFunction_t jit_fn = jit_fused_fn<T>(s, !s->jit_policy ? nullptr : sink ? s->jit_policy->fn_policy_rec : s->jit_policy->fn_policy);
  Os2rSim* const kn = sink ? sink->knots : nullptr;
  if ((!s->jit || jit_fn) && !s->counters) {
    if (sink) {
      p.knot_obs = (T*)sink->obs;
      if (kn) {
        p.knot_what = sink->what; p.knot_stride = kn->cfg.num_envs; p.knot_lane = (long long)sink->first_knot * (long long)N;
        p.kq = (T*)kn->q; p.kqd = (T*)kn->qd; p.khist = (T*)kn->hist; p.ksolver_l = (T*)kn->solver_l;
        p.ksolver_flags = kn->solver_flags; p.ksteps = kn->steps; p.kepisode = kn->episode; p.kpose = kn->pose;
        p.kmass_scale = (T*)kn->mass_scale; p.kdamping = (T*)kn->damping; p.kfriction = (T*)kn->friction; p.kmu = (T*)kn->mu;
        p.kgravity = (T*)kn->gravity;
      }
    }
    p.s = make_args<T>(s);
    p.s.obs = (T*)obs; p.s.reward = (T*)reward; p.s.done = done; p.s.term_obs = (T*)term; p.s.reason = reason;
    p.s.done_mask = nullptr;   // (neither of the per-step buffers set on the handle is written)
    p.s.rollout_steps = K;
    if (jit_fn) HIP_TRY(s, jit_launch(jit_fn, p, p.s.N, 1, st));
    if (jit_fn || Launcher<T>::policy_rollout(s->model_id, s->cfg.contact != 0, s->dr, p, st) == 0) {
      HIP_TRY(s, hipGetLastError());
      s->step_count += (unsigned long long)K;
      knots_read_params(kn, s, sink);
      return OS2R_OK;
    }
    p.knot_what = 0;   // (no fused variant after all: the launch loop copies, and its policy kernel takes nothing of the sink but knot_obs)
  }
  int rc = OS2R_OK;
  if (!s->pol_act) {
    if ((rc = dev_alloc(s, &s->pol_act, 2 * N * s->esz))) return rc;
    if ((rc = dev_alloc(s, (void**)&s->pol_open, N))) return rc;
  }
  p.act = (T*)s->pol_act; p.open = s->pol_open;
  uint16_t* const reason_keep = s->reason;
  uint8_t* const mask_keep = s->done_mask;
  s->done_mask = nullptr;
  for (int k = 0; k < K && rc == OS2R_OK; ++k) {
    p.s = make_args<T>(s);   // (with it the step counter of env-step k, which keys the noise)
    p.act_out = act_out ? (T*)act_out + (size_t)k * N * 2 : nullptr;
    p.eps_out = eps_out ? (T*)eps_out + (size_t)k * N * 2 : nullptr;
    if (period > 0 && !(flags & OS2R_POLICY_CLOCK_EPISODE)) {
      // the window clock of env-step k, reduced to its slot here (the sum may not fit 32 bits); the kernel's rule leaves a slot as it is
      const long long t = (long long)first_slot + k;
      p.first_slot = (int)((flags & OS2R_POLICY_SCHEDULE_WRAP) ? t % period : (t < period - 1 ? t : period - 1));
    }
    if (kn) {
      // knot first_knot + k: the copy kernel with the destination's rows moved to the knot's first lane, N lanes, the identity map
      CopyArgs<T> c = copy_rows<T>(kn, s, sink->what, nullptr, false);
      const size_t lane0 = ((size_t)sink->first_knot + (size_t)k) * N;
      for (int r = 0; r < c.nrows; ++r) c.dst[r] += lane0;
      for (int r = 0; r < c.nwords; ++r) c.dst32[r] += lane0;
      if (c.dst8) c.dst8 += lane0;
      c.Nd = c.Ns = (long long)N; c.index = nullptr;
      Launcher<T>::copy_envs(c, st);
    }
    p.knot_obs = sink && sink->obs ? (T*)sink->obs + (size_t)k * N * D : nullptr;
    if (Launcher<T>::policy(s->nq, p, st) != 0) { s->err = "no policy kernel for this chain length"; rc = OS2R_ERR_INVALID; break; }
    // the sums need the step's reward and done flag: the handle's scratch outputs stand in for the ones not asked for
    T* const rew_k = reward ? (T*)reward + (size_t)k * N : (T*)s->b_rew;
    uint8_t* const done_k = done ? done + (size_t)k * N : s->b_done;
    s->reason = reason ? reason + (size_t)k * N : nullptr;
    rc = do_step<T>(s, s->pol_act, obs ? (T*)obs + (size_t)k * N * D : nullptr, rew_k, done_k, term ? (T*)term + (size_t)k * N * D : nullptr, st);
    if (rc == OS2R_OK && (ret || len))
      Launcher<T>::accumulate((T*)ret, len, s->pol_open, rew_k, done_k, (long long)N, k, (flags & OS2R_POLICY_FIRST_EPISODE) != 0, st);
  }
  s->reason = reason_keep;
  s->done_mask = mask_keep;
  if (rc == OS2R_OK) HIP_TRY(s, hipGetLastError());
  if (rc == OS2R_OK) knots_read_params(kn, s, sink);
  return rc;
}

template <typename T>
int do_copy(Os2rSim* d, Os2rSim* s, const int32_t* index, int what, void* obs, hipStream_t st) {
  if (d != s) {
    CopyArgs<T> a = copy_rows<T>(d, s, what, nullptr, false);
    a.index = index;
    Launcher<T>::copy_envs(a, st);
  } else if (index) {
    // within one handle all reads precede all writes: gather into the staging rows, then copy the same lanes back
    if (!d->copy_stage) {
      const size_t N = (size_t)d->cfg.num_envs;
      const int rc = dev_alloc(d, &d->copy_stage, ((size_t)(10 * d->nq + 5) * d->esz + 3 * 4 + 1) * N);
      if (rc) return rc;
    }
    CopyArgs<T> a = copy_rows<T>(d, s, what, d->copy_stage, true);
    a.index = index;
    Launcher<T>::copy_envs(a, st);
    a = copy_rows<T>(d, s, what, d->copy_stage, false);
    a.index = index; a.gather = 0;
    Launcher<T>::copy_envs(a, st);
  }
  if (d != s && (what & OS2R_COPY_PARAMS) && (s->dr || s->cfg.model.gravity_z != d->cfg.model.gravity_z))
    d->dr = true;   // as after os2r_set_params: the step kernels read the parameter arrays per lane from now on
  if (obs) {
    StepArgs<T> a = make_args<T>(d);
    a.obs = (T*)obs;
    if (Launcher<T>::copy_obs(d->nq, a, st) != 0) { d->err = "os2r_copy_envs: no observation kernel for this chain length"; return OS2R_ERR_INVALID; }
  }
  HIP_TRY(d, hipGetLastError());
  return OS2R_OK;
}

// os2r_linearize: one launch, grid.y over the columns the outputs asked for; the handle's arrays are only read
template <typename T>
int do_linearize(Os2rSim* s, const void* actions, const double* eps, void* next, void* jac_a, void* jac_b, hipStream_t st) {
  LinArgs<T> p;
  std::memset(&p, 0, sizeof(p));
  p.s = make_args<T>(s);
  p.s.actions = (const T*)actions;
  // (a query: no violation is counted, the mirror and the work counters stay as they are)
  p.s.violations = nullptr; p.s.mirror = nullptr; p.s.counters = nullptr; p.s.reason = nullptr; p.s.done_mask = nullptr;
  p.eps_q = (T)eps[0]; p.eps_qd = (T)eps[1]; p.eps_a = (T)eps[2];
  if (!(p.eps_q > T(0)) || !(p.eps_qd > T(0)) || !(p.eps_a > T(0))) { s->err = "os2r_linearize: eps must be positive in the handle's dtype (it rounds to zero)"; return OS2R_ERR_INVALID; }
  if (!(p.eps_a < T(1))) { s->err = "os2r_linearize: eps[2] (action step) must be < 1 in the handle's dtype"; return OS2R_ERR_INVALID; }
  p.next = (T*)next; p.jac_a = (T*)jac_a; p.jac_b = (T*)jac_b;
  const int nq = s->nq;
  if (jac_a) for (int j = 0; j < 2 * nq; ++j) p.col[p.ncols++] = j;
  if (jac_b) for (int j = 0; j < 2; ++j) p.col[p.ncols++] = 2 * nq + j;
  if (next) p.col[p.ncols++] = 2 * nq + 2;
  // a handle with a code object: the linearize kernel beside the step kernel do_step picks (the layout variant runs the
  // substep instantiation of ..._s), where the robot's registrations export it; else the generic kernels
  hipFunction_t jit_fn = nullptr;
  if (s->jit && s->jit_lin) {
    const bool contact = s->cfg.contact != 0 && s->cmask != 0u;
    const bool std_step = is_std_solver<T>(p.s.pgs_iters, p.s.pgs_normal_iters, p.s.pgs_exact, s->cfg.model.nq) &&
                          (s->jit->fn[contact][s->dr][1] ||
                           (contact && s->jit->fn_layout[s->dr] && s->jit->layout_dim == p.s.layout_dim &&
                            s->jit->layout_kinds == p.s.layout_kinds && s->jit->layout_srcs == p.s.layout_srcs));
    jit_fn = s->jit_lin->fn_lin[contact][s->dr][std_step];
  }
  if (jit_fn) {
    HIP_TRY(s, jit_launch(jit_fn, p, p.s.N, (unsigned)p.ncols, st));
  } else if (Launcher<T>::linearize(nq, s->model_id, s->cfg.contact != 0, s->dr, p, st) != 0) {
    s->err = "os2r_linearize: no kernel for this chain length";
    return OS2R_ERR_INVALID;
  }
  HIP_TRY(s, hipGetLastError());
  return OS2R_OK;
}

// os2r_lqr_gains: one launch; the handle gives the dtype, nq and the observation layout and is not touched
template <typename T>
int do_lqr_gains(Os2rSim* s, int nknots, long long ntraj, int sweeps, const void* a, const void* b, const double* q, const double* r,
                 const void* p_final, void* gain, void* p_out, uint8_t* flag, const void* actions, const void* obs, void* weights,
                 hipStream_t st) {
  LqrArgs<T> p;
  std::memset(&p, 0, sizeof(p));
  const int nq = s->nq, n = 2 * nq;
  p.a = (const T*)a; p.b = (const T*)b; p.p_final = (const T*)p_final; p.p_out = (T*)p_out; p.gain = (T*)gain; p.flag = flag;
  p.actions = (const T*)actions; p.obs = (const T*)obs; p.weights = (T*)weights;
  p.M = ntraj; p.K = nknots; p.sweeps = sweeps; p.D = s->D;
  const Os2rTaskSpec& t = s->cfg.task;
  for (int d = 0; d < OS2R_MAX_OBS; ++d) {
    p.slot_col[d] = -1;
    if (d >= s->D) continue;
    if (t.obs_kind[d] == OS2R_OBS_POS_RAW || t.obs_kind[d] == OS2R_OBS_POS_PERIODIC_RAW) p.slot_col[d] = t.obs_src[d];
    if (t.obs_kind[d] == OS2R_OBS_VEL_RAW) p.slot_col[d] = nq + t.obs_src[d];
  }
  p.r00 = (T)r[0]; p.r01 = (T)r[1]; p.r11 = (T)r[3];
  for (int i = 0; i < n * n; ++i) p.q[i] = (T)q[i];
  if (launch_lqr_gains<T>(nq, p, st) != 0) {
    s->err = "os2r_lqr_gains: no kernel for this chain length";
    return OS2R_ERR_INVALID;
  }
  HIP_TRY(s, hipGetLastError());
  return OS2R_OK;
}

// What the three os2r_rollout_policy* entry points refuse before they touch the device, in one order.  An entry point fills in
// its name, `unknown` (its flags without the bits it knows) and the rules that apply to it, each field by its name.
struct PolicyCall {
  const char* name; int nsteps; const void* weights; int unknown;
  const char* missing = nullptr;   // an argument of the entry point's own that it requires and that is null: the refusal's text
  bool scheduled = false;          // the scheduled entry point: the rules on the fields below; it is also the one of the three
  int period = 1, first_slot = 0;  //   that names a null handle in os2r_last_error(NULL)
  const void *sigma = nullptr, *noise = nullptr;
  uint32_t salt = 0u;
};

int check_policy_call(Os2rSim* sim, const PolicyCall& c) {
  auto refuse = [&](const char* why) {
    (sim ? sim->err : g_create_error) = std::string(c.name) + ": " + why;
    return (int)OS2R_ERR_INVALID;
  };
  if (!sim) return c.scheduled ? refuse("null handle") : (int)OS2R_ERR_INVALID;
  if (c.nsteps < 1) return refuse("nsteps must be >= 1");
  if (c.scheduled && c.period < 1) return refuse("period must be >= 1");
  if (c.scheduled && c.first_slot < 0) return refuse("first_slot must be >= 0");
  if (!c.weights) return refuse("null weights");
  if (c.missing) return refuse(c.missing);
  if (c.unknown) return refuse("unknown flag bits");
  if (c.scheduled && !c.sigma && c.noise) return refuse("noise_dev needs sigma_dev");
  if (c.scheduled && !c.sigma && c.salt != 0u) return refuse("a non-zero salt needs sigma_dev");
  return OS2R_OK;
}

void free_all(Os2rSim* s) {
  for (void* p : s->allocs) (void)hipFree(p);
  s->allocs.clear();
  if (s->ev0) (void)hipEventDestroy(s->ev0);
  if (s->ev1) (void)hipEventDestroy(s->ev1);
  if (s->mirror_host) (void)hipHostFree(s->mirror_host);
  s->mirror_host = s->mirror_dev = nullptr;
}

int param_view(Os2rSim* s, int field, void** base, int* count) {
  switch (field) {
    case OS2R_PARAM_MASS_SCALE: *base = s->mass_scale; *count = s->nq; return 0;
    case OS2R_PARAM_DAMPING: *base = s->damping; *count = s->nq; return 0;
    case OS2R_PARAM_FRICTION: *base = s->friction; *count = s->nq; return 0;
    case OS2R_PARAM_MU: *base = s->mu; *count = s->nq; return 0;
    case OS2R_PARAM_GRAVITY: *base = s->gravity; *count = 1; return 0;
    default: return 1;
  }
}

}  // namespace

extern "C" {

int os2r_abi_version(void) { return OS2R_ABI_VERSION; }
int os2r_abi_minor(void) { return OS2R_ABI_MINOR; }

int os2r_create(const Os2rConfig* cfg, Os2rSim** out) {
  if (!out) { g_create_error = "null out pointer"; return OS2R_ERR_INVALID; }
  *out = nullptr;
  std::string why;
  if (validate(cfg, why)) { g_create_error = why; return OS2R_ERR_INVALID; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    g_create_error = "no HIP device visible: the stepper has no CPU fallback";
    return OS2R_ERR_NO_DEVICE;
  }
  if (cfg->device < 0 || cfg->device >= ndev) { g_create_error = "device ordinal out of range"; return OS2R_ERR_INVALID; }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess) { g_create_error = "hipGetDeviceProperties failed"; return OS2R_ERR_HIP; }
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    g_create_error = std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only";
    return OS2R_ERR_NO_DEVICE;
  }
  Os2rSim* s = new (std::nothrow) Os2rSim();
  if (!s) { g_create_error = "out of host memory"; return OS2R_ERR_ALLOC; }
  s->cfg = *cfg;
  s->nq = cfg->model.nq;
  s->D = cfg->task.obs_dim;
  s->esz = cfg->dtype == OS2R_F64 ? 8 : 4;
  // parameter arrays are read per lane only when something can make them differ per env:
  // the randomising reset mode, or a later os2r_set_params (which flips this on)
  s->dr = cfg->task.reset_mode == OS2R_RESET_RANDOM;
  s->model_id = static_model_id(cfg->model);
  s->cmask = 0;
  if (cfg->contact)
    for (int k = 0; k < cfg->model.ncand; ++k) s->cmask |= 1u << cfg->model.cand_body[k];
  if (s->model_id < 0) s->jit = find_jit(cfg->model, cfg->dtype, cfg->device, cfg->contact != 0 && s->cmask != 0u, cfg->task);
  if (s->jit) {   // the other kinds serve a handle only beside the robot's own step kernels: one arithmetic per handle
    const bool contact = cfg->contact != 0 && s->cmask != 0u;
    s->jit_rollout = find_jit(cfg->model, cfg->dtype, cfg->device, contact, cfg->task, kJitRollout);
    s->jit_policy = find_jit(cfg->model, cfg->dtype, cfg->device, contact, cfg->task, kJitPolicy);
    s->jit_lin = find_jit(cfg->model, cfg->dtype, cfg->device, contact, cfg->task, kJitLin);
  }
  int rc = OS2R_OK;
  auto fail = [&](int code) { g_create_error = s->err; free_all(s); delete s; return code; };
  DeviceGuard guard(cfg->device);   // allocate and initialise on the handle's device, then give the caller's back
  if (hipSetDevice(cfg->device) != hipSuccess) { s->err = "hipSetDevice failed"; return fail(OS2R_ERR_HIP); }
  const size_t N = (size_t)cfg->num_envs, n = (size_t)s->nq, e = s->esz;
  if ((rc = dev_alloc(s, &s->q, n * N * e))) return fail(rc);
  if ((rc = dev_alloc(s, &s->qd, n * N * e))) return fail(rc);
  if ((rc = dev_alloc(s, &s->hist, 4 * N * e))) return fail(rc);
  if ((rc = dev_alloc(s, &s->mass_scale, n * N * e))) return fail(rc);
  if ((rc = dev_alloc(s, &s->damping, n * N * e))) return fail(rc);
  if ((rc = dev_alloc(s, &s->friction, n * N * e))) return fail(rc);
  if ((rc = dev_alloc(s, &s->mu, n * N * e))) return fail(rc);
  if ((rc = dev_alloc(s, &s->gravity, N * e))) return fail(rc);
  if ((rc = dev_alloc(s, (void**)&s->steps, N * 4))) return fail(rc);
  if ((rc = dev_alloc(s, (void**)&s->episode, N * 4))) return fail(rc);
  if ((rc = dev_alloc(s, (void**)&s->pose, N))) return fail(rc);
  if ((rc = dev_alloc(s, &s->solver_l, 4 * n * N * e))) return fail(rc);
  if ((rc = dev_alloc(s, (void**)&s->solver_flags, N * 4))) return fail(rc);
  if ((rc = dev_alloc(s, (void**)&s->violations, 4))) return fail(rc);
  if ((rc = dev_alloc(s, &s->b_obs, (size_t)s->D * N * e))) return fail(rc);
  if ((rc = dev_alloc(s, &s->b_rew, N * e))) return fail(rc);
  if ((rc = dev_alloc(s, &s->b_term, (size_t)s->D * N * e))) return fail(rc);
  if ((rc = dev_alloc(s, (void**)&s->b_done, N))) return fail(rc);
  if ((rc = by_dtype(s, [&](auto t) { return upload_model<decltype(t)>(s); }))) return fail(rc);
  if (hipEventCreate(&s->ev0) != hipSuccess || hipEventCreate(&s->ev1) != hipSuccess) { s->err = "hipEventCreate failed"; return fail(OS2R_ERR_HIP); }
  // the violation mirror: pinned host memory that the device writes with plain system-scope stores (no atomics across PCIe)
  {
    void* hp = nullptr; void* dp = nullptr;
    if (hipHostMalloc(&hp, 64, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) { s->err = "hipHostMalloc (violation mirror) failed"; return fail(OS2R_ERR_ALLOC); }
    s->mirror_host = (uint32_t*)hp;
    std::memset(hp, 0, 64);
    if (hipHostGetDevicePointer(&dp, hp, 0) != hipSuccess) { s->err = "hipHostGetDevicePointer (violation mirror) failed"; return fail(OS2R_ERR_HIP); }
    s->mirror_dev = (uint32_t*)dp;
  }
  if ((rc = by_dtype(s, [&](auto t) { return init_params<decltype(t)>(s, nullptr); }))) return fail(rc);
  if ((rc = by_dtype(s, [&](auto t) { return do_reset<decltype(t)>(s, nullptr, nullptr, nullptr); }))) return fail(rc);
  if (hipStreamSynchronize(nullptr) != hipSuccess) { s->err = "initial reset failed"; return fail(OS2R_ERR_HIP); }
  *out = s;
  return OS2R_OK;
}

int os2r_destroy(Os2rSim* sim) {
  if (!sim) return OS2R_ERR_INVALID;
  DeviceGuard guard(sim->cfg.device);
  (void)hipDeviceSynchronize();
  free_all(sim);
  delete sim;
  return OS2R_OK;
}

int os2r_reset(Os2rSim* sim, const uint8_t* mask_dev, void* obs_dev, void* stream) {
  if (!sim) return OS2R_ERR_INVALID;
  DeviceGuard guard(sim->cfg.device);
  return by_dtype(sim, [&](auto t) { return do_reset<decltype(t)>(sim, mask_dev, obs_dev, (hipStream_t)stream); });
}

int os2r_step(Os2rSim* sim, const void* actions_dev, void* obs_dev, void* reward_dev, uint8_t* done_dev,
              void* term_obs_dev, void* stream) {
  if (!sim) return OS2R_ERR_INVALID;
  DeviceGuard guard(sim->cfg.device);
  return by_dtype(sim, [&](auto t) { return do_step<decltype(t)>(sim, actions_dev, obs_dev, reward_dev, done_dev, term_obs_dev, (hipStream_t)stream); });
}

int os2r_rollout(Os2rSim* sim, int nsteps, const void* actions_dev, void* obs_dev, void* reward_dev, uint8_t* done_dev,
                 void* term_obs_dev, uint16_t* reason_dev, void* stream) {
  if (!sim || nsteps < 1) return OS2R_ERR_INVALID;
  DeviceGuard guard(sim->cfg.device);
  return by_dtype(sim, [&](auto t) {
    return do_rollout<decltype(t)>(sim, nsteps, actions_dev, obs_dev, reward_dev, done_dev, term_obs_dev, reason_dev, (hipStream_t)stream);
  });
}

int os2r_rollout_policy(Os2rSim* sim, int nsteps, const void* weights_dev, int32_t flags, void* return_dev, int32_t* length_dev,
                        void* obs_dev, void* reward_dev, uint8_t* done_dev, void* term_obs_dev, uint16_t* reason_dev, void* stream) {
  const PolicyCall call{"os2r_rollout_policy", nsteps, weights_dev, flags & ~(OS2R_POLICY_PER_ENV | OS2R_POLICY_TANH | OS2R_POLICY_FIRST_EPISODE)};
  if (int rc = check_policy_call(sim, call)) return rc;
  DeviceGuard guard(sim->cfg.device);
  return by_dtype(sim, [&](auto t) {
    return do_rollout_policy<decltype(t)>(sim, nsteps, weights_dev, flags, return_dev, length_dev, obs_dev, reward_dev, done_dev, term_obs_dev,
                                          reason_dev, (hipStream_t)stream);
  });
}

int os2r_rollout_policy_noisy(Os2rSim* sim, int nsteps, const void* weights_dev, int32_t flags, const void* sigma_dev, uint32_t salt,
                              void* return_dev, int32_t* length_dev, void* obs_dev, void* reward_dev, uint8_t* done_dev,
                              void* term_obs_dev, uint16_t* reason_dev, void* action_dev, void* noise_dev, void* stream) {
  PolicyCall call{"os2r_rollout_policy_noisy", nsteps, weights_dev,
                  flags & ~(OS2R_POLICY_PER_ENV | OS2R_POLICY_TANH | OS2R_POLICY_FIRST_EPISODE | OS2R_POLICY_SIGMA_PER_ENV)};
  if (!sigma_dev) call.missing = "null sigma";
  if (int rc = check_policy_call(sim, call)) return rc;
  DeviceGuard guard(sim->cfg.device);
  return by_dtype(sim, [&](auto t) {
    return do_rollout_policy<decltype(t)>(sim, nsteps, weights_dev, flags, return_dev, length_dev, obs_dev, reward_dev, done_dev, term_obs_dev,
                                          reason_dev, (hipStream_t)stream, sigma_dev, salt, action_dev, noise_dev);
  });
}

int os2r_rollout_policy_scheduled(Os2rSim* sim, int nsteps, const void* weights_dev, int32_t period, int32_t first_slot, int32_t flags,
                                  const void* sigma_dev, uint32_t salt, void* return_dev, int32_t* length_dev, void* obs_dev,
                                  void* reward_dev, uint8_t* done_dev, void* term_obs_dev, uint16_t* reason_dev, void* action_dev,
                                  void* noise_dev, void* stream) {
  PolicyCall call{"os2r_rollout_policy_scheduled", nsteps, weights_dev,
                  flags & ~(OS2R_POLICY_PER_ENV | OS2R_POLICY_TANH | OS2R_POLICY_FIRST_EPISODE | OS2R_POLICY_SIGMA_PER_ENV |
                            OS2R_POLICY_CLOCK_EPISODE | OS2R_POLICY_SCHEDULE_WRAP)};
  call.scheduled = true; call.period = period; call.first_slot = first_slot;
  call.sigma = sigma_dev; call.salt = salt; call.noise = noise_dev;
  if (int rc = check_policy_call(sim, call)) return rc;
  DeviceGuard guard(sim->cfg.device);
  return by_dtype(sim, [&](auto t) {
    return do_rollout_policy<decltype(t)>(sim, nsteps, weights_dev, flags, return_dev, length_dev, obs_dev, reward_dev, done_dev, term_obs_dev,
                                          reason_dev, (hipStream_t)stream, sigma_dev, salt, action_dev, noise_dev, period, first_slot);
  });
}

int os2rr_rollout_policy_recorded(Os2rSim* sim, Os2rSim* knots, int32_t first_knot, int32_t what, void* knot_obs_dev, int nsteps,
                                 const void* weights_dev, int32_t period, int32_t first_slot, int32_t flags, const void* sigma_dev,
                                 uint32_t salt, void* return_dev, int32_t* length_dev, void* obs_dev, void* reward_dev, uint8_t* done_dev,
                                 void* term_obs_dev, uint16_t* reason_dev, void* action_dev, void* noise_dev, void* stream) {
  PolicyCall call{"os2rr_rollout_policy_recorded", nsteps, weights_dev,
                  flags & ~(OS2R_POLICY_PER_ENV | OS2R_POLICY_TANH | OS2R_POLICY_FIRST_EPISODE | OS2R_POLICY_SIGMA_PER_ENV |
                            OS2R_POLICY_CLOCK_EPISODE | OS2R_POLICY_SCHEDULE_WRAP)};
  call.scheduled = true; call.period = period; call.first_slot = first_slot;
  call.sigma = sigma_dev; call.salt = salt; call.noise = noise_dev;
  if (int rc = check_policy_call(sim, call)) return rc;
  auto refuse = [&](const std::string& why) { sim->err = "os2rr_rollout_policy_recorded: " + why; return (int)OS2R_ERR_INVALID; };
  if (!knots && !knot_obs_dev) return refuse("nothing to record into (knots and knot_obs_dev are both null)");
  if (knots) {
    if (knots == sim) return refuse("knots must be another handle than sim");
    if (knots->cfg.dtype != sim->cfg.dtype) return refuse("sim and knots differ in dtype");
    if (knots->cfg.device != sim->cfg.device) return refuse("sim and knots are on different devices");
    if (!os2r::same_model(sim->cfg.model, knots->cfg.model)) return refuse("sim and knots are different robot models");
    if (what == 0) return refuse("nothing selected (what == 0)");
    if (what & ~(OS2R_COPY_STATE | OS2R_COPY_PARAMS)) return refuse("unknown bits in what");
    if (first_knot < 0) return refuse("first_knot must be >= 0");
    const long long need = ((long long)first_knot + (long long)nsteps) * (long long)sim->cfg.num_envs;
    if (need > (long long)knots->cfg.num_envs)
      return refuse("knots has " + std::to_string(knots->cfg.num_envs) + " environments, (first_knot + nsteps) * num_envs = " +
                    std::to_string(need) + " are needed");
  }
  const KnotSink sink{knots, knots ? first_knot : 0, knots ? what : 0, knot_obs_dev};
  DeviceGuard guard(sim->cfg.device);
  return by_dtype(sim, [&](auto t) {
    return do_rollout_policy<decltype(t)>(sim, nsteps, weights_dev, flags, return_dev, length_dev, obs_dev, reward_dev, done_dev, term_obs_dev,
                                          reason_dev, (hipStream_t)stream, sigma_dev, salt, action_dev, noise_dev, period, first_slot, &sink);
  });
}

int os2r_copy_envs(Os2rSim* dst, Os2rSim* src, const int32_t* index_dev, int32_t what, void* obs_dev, void* stream) {
  if (!dst) { g_create_error = "os2r_copy_envs: null destination handle"; return OS2R_ERR_INVALID; }
  if (!src) { dst->err = "os2r_copy_envs: null source handle"; return OS2R_ERR_INVALID; }
  if (what == 0 || (what & ~(OS2R_COPY_STATE | OS2R_COPY_PARAMS))) {
    dst->err = what == 0 ? "os2r_copy_envs: nothing selected (what == 0)" : "os2r_copy_envs: unknown bits in what";
    return OS2R_ERR_INVALID;
  }
  if (src->cfg.dtype != dst->cfg.dtype) { dst->err = "os2r_copy_envs: source and destination differ in dtype"; return OS2R_ERR_INVALID; }
  if (src->cfg.device != dst->cfg.device) { dst->err = "os2r_copy_envs: source and destination are on different devices"; return OS2R_ERR_INVALID; }
  if (!os2r::same_model(src->cfg.model, dst->cfg.model)) { dst->err = "os2r_copy_envs: source and destination are different robot models"; return OS2R_ERR_INVALID; }
  if (!index_dev && src->cfg.num_envs != dst->cfg.num_envs) {
    dst->err = "os2r_copy_envs: the identity map (null index) needs equal num_envs";
    return OS2R_ERR_INVALID;
  }
  DeviceGuard guard(dst->cfg.device);
  return by_dtype(dst, [&](auto t) { return do_copy<decltype(t)>(dst, src, index_dev, what, obs_dev, (hipStream_t)stream); });
}

int os2r_linearize(Os2rSim* sim, const void* actions_dev, const double eps[3], void* next_dev, void* a_dev, void* b_dev, void* stream) {
  if (!sim) { g_create_error = "os2r_linearize: null handle"; return OS2R_ERR_INVALID; }
  if (!actions_dev) { sim->err = "os2r_linearize: null actions"; return OS2R_ERR_INVALID; }
  if (!eps) { sim->err = "os2r_linearize: null eps"; return OS2R_ERR_INVALID; }
  if (!next_dev && !a_dev && !b_dev) { sim->err = "os2r_linearize: all three outputs are null"; return OS2R_ERR_INVALID; }
  for (int k = 0; k < 3; ++k) {
    // (bit pattern first: the library is built without NaN semantics, see validate)
    if (!is_finite(&eps[k])) { sim->err = "os2r_linearize: eps must be finite"; return OS2R_ERR_INVALID; }
    if (!(eps[k] > 0.0)) { sim->err = "os2r_linearize: eps must be positive"; return OS2R_ERR_INVALID; }
  }
  if (eps[2] >= 1.0) { sim->err = "os2r_linearize: eps[2] (action step) must be < 1"; return OS2R_ERR_INVALID; }
  DeviceGuard guard(sim->cfg.device);
  return by_dtype(sim, [&](auto t) { return do_linearize<decltype(t)>(sim, actions_dev, eps, next_dev, a_dev, b_dev, (hipStream_t)stream); });
}

int os2r_lqr_gains(Os2rSim* sim, int32_t nknots, int64_t ntraj, int32_t sweeps, const void* a_dev, const void* b_dev,
                   const double* q_host, const double* r_host, const void* p_final_dev, void* gain_dev, void* p_out_dev,
                   uint8_t* flag_dev, const void* actions_dev, const void* obs_dev, void* weights_dev, void* stream) {
  if (!sim) { g_create_error = "os2r_lqr_gains: null handle"; return OS2R_ERR_INVALID; }
  if (nknots < 1) { sim->err = "os2r_lqr_gains: nknots must be >= 1"; return OS2R_ERR_INVALID; }
  if (ntraj < 1) { sim->err = "os2r_lqr_gains: ntraj must be >= 1"; return OS2R_ERR_INVALID; }
  if (ntraj > (int64_t)kLqrEnvs * 0x7fffffffll) { sim->err = "os2r_lqr_gains: ntraj exceeds what one launch covers"; return OS2R_ERR_INVALID; }
  if (sweeps < 1) { sim->err = "os2r_lqr_gains: sweeps must be >= 1"; return OS2R_ERR_INVALID; }
  if (!a_dev) { sim->err = "os2r_lqr_gains: null a_dev"; return OS2R_ERR_INVALID; }
  if (!b_dev) { sim->err = "os2r_lqr_gains: null b_dev"; return OS2R_ERR_INVALID; }
  if (!q_host) { sim->err = "os2r_lqr_gains: null q_host"; return OS2R_ERR_INVALID; }
  if (!r_host) { sim->err = "os2r_lqr_gains: null r_host"; return OS2R_ERR_INVALID; }
  const int n = 2 * sim->nq;
  // (bit patterns: the library is built without NaN semantics, see is_finite)
  if (!all_finite(q_host, n * n)) { sim->err = "os2r_lqr_gains: Q must be finite"; return OS2R_ERR_INVALID; }
  if (!all_finite(r_host, 4)) { sim->err = "os2r_lqr_gains: R must be finite"; return OS2R_ERR_INVALID; }
  if (!symmetric(q_host, n)) { sim->err = "os2r_lqr_gains: Q must be exactly symmetric"; return OS2R_ERR_INVALID; }
  if (!symmetric(r_host, 2)) { sim->err = "os2r_lqr_gains: R must be exactly symmetric"; return OS2R_ERR_INVALID; }
  if (!gain_dev && !p_out_dev && !weights_dev) { sim->err = "os2r_lqr_gains: all outputs are null (gain, p_out, weights)"; return OS2R_ERR_INVALID; }
  if (weights_dev && (!actions_dev || !obs_dev)) { sim->err = "os2r_lqr_gains: weights need actions_dev and obs_dev"; return OS2R_ERR_INVALID; }
  DeviceGuard guard(sim->cfg.device);
  return by_dtype(sim, [&](auto t) {
    return do_lqr_gains<decltype(t)>(sim, nknots, ntraj, sweeps, a_dev, b_dev, q_host, r_host, p_final_dev, gain_dev, p_out_dev, flag_dev,
                                     actions_dev, obs_dev, weights_dev, (hipStream_t)stream);
  });
}

int os2r_get_state(Os2rSim* sim, void* q_dev, void* qd_dev, void* stream) {
  if (!sim) return OS2R_ERR_INVALID;
  DeviceGuard guard(sim->cfg.device);
  const size_t b = (size_t)sim->nq * sim->cfg.num_envs * sim->esz;
  if (q_dev) HIP_TRY(sim, hipMemcpyAsync(q_dev, sim->q, b, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (qd_dev) HIP_TRY(sim, hipMemcpyAsync(qd_dev, sim->qd, b, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return OS2R_OK;
}

int os2r_set_state(Os2rSim* sim, const void* q_dev, const void* qd_dev, void* stream) {
  if (!sim) return OS2R_ERR_INVALID;
  DeviceGuard guard(sim->cfg.device);
  const size_t b = (size_t)sim->nq * sim->cfg.num_envs * sim->esz;
  if (q_dev) HIP_TRY(sim, hipMemcpyAsync(sim->q, q_dev, b, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (qd_dev) HIP_TRY(sim, hipMemcpyAsync(sim->qd, qd_dev, b, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  // a state set from outside starts like a reset: the contact solver remembers nothing (os2r_set_solver_state restores it)
  HIP_TRY(sim, hipMemsetAsync(sim->solver_flags, 0, (size_t)sim->cfg.num_envs * 4, (hipStream_t)stream));
  HIP_TRY(sim, hipMemsetAsync(sim->solver_l, 0, 4 * b, (hipStream_t)stream));
  return OS2R_OK;
}

int os2r_get_solver_state(Os2rSim* sim, void* lambda_dev, uint32_t* flags_dev, void* stream) {
  if (!sim) return OS2R_ERR_INVALID;
  DeviceGuard guard(sim->cfg.device);
  const size_t N = (size_t)sim->cfg.num_envs;
  if (lambda_dev) HIP_TRY(sim, hipMemcpyAsync(lambda_dev, sim->solver_l, 4 * (size_t)sim->nq * N * sim->esz, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (flags_dev) HIP_TRY(sim, hipMemcpyAsync(flags_dev, sim->solver_flags, N * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return OS2R_OK;
}

int os2r_set_solver_state(Os2rSim* sim, const void* lambda_dev, const uint32_t* flags_dev, void* stream) {
  if (!sim || !lambda_dev || !flags_dev) return OS2R_ERR_INVALID;
  DeviceGuard guard(sim->cfg.device);
  const size_t N = (size_t)sim->cfg.num_envs;
  HIP_TRY(sim, hipMemcpyAsync(sim->solver_l, lambda_dev, 4 * (size_t)sim->nq * N * sim->esz, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  HIP_TRY(sim, hipMemcpyAsync(sim->solver_flags, flags_dev, N * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return OS2R_OK;
}

int os2r_get_action_history(Os2rSim* sim, int which, void* out_dev, void* stream) {
  if (!sim || which < 0 || which > 1 || !out_dev) return OS2R_ERR_INVALID;
  DeviceGuard guard(sim->cfg.device);
  const size_t b = 2 * (size_t)sim->cfg.num_envs * sim->esz;
  HIP_TRY(sim, hipMemcpyAsync(out_dev, (char*)sim->hist + which * b, b, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return OS2R_OK;
}

int os2r_set_action_history(Os2rSim* sim, int which, const void* in_dev, void* stream) {
  if (!sim || which < 0 || which > 1 || !in_dev) return OS2R_ERR_INVALID;
  DeviceGuard guard(sim->cfg.device);
  const size_t b = 2 * (size_t)sim->cfg.num_envs * sim->esz;
  HIP_TRY(sim, hipMemcpyAsync((char*)sim->hist + which * b, in_dev, b, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return OS2R_OK;
}

int os2r_set_params(Os2rSim* sim, int field, const void* src_dev, void* stream) {
  void* base; int count;
  if (!sim || !src_dev || param_view(sim, field, &base, &count)) return OS2R_ERR_INVALID;
  DeviceGuard guard(sim->cfg.device);
  HIP_TRY(sim, hipMemcpyAsync(base, src_dev, (size_t)count * sim->cfg.num_envs * sim->esz, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  sim->dr = true;
  return OS2R_OK;
}

int os2r_get_params(Os2rSim* sim, int field, void* dst_dev, void* stream) {
  void* base; int count;
  if (!sim || !dst_dev || param_view(sim, field, &base, &count)) return OS2R_ERR_INVALID;
  DeviceGuard guard(sim->cfg.device);
  HIP_TRY(sim, hipMemcpyAsync(dst_dev, base, (size_t)count * sim->cfg.num_envs * sim->esz, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return OS2R_OK;
}

int os2r_get_episode_info(Os2rSim* sim, int32_t* steps_dev, uint32_t* episode_dev, uint8_t* pose_dev, void* stream) {
  if (!sim) return OS2R_ERR_INVALID;
  DeviceGuard guard(sim->cfg.device);
  const size_t N = (size_t)sim->cfg.num_envs;
  if (steps_dev) HIP_TRY(sim, hipMemcpyAsync(steps_dev, sim->steps, N * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (episode_dev) HIP_TRY(sim, hipMemcpyAsync(episode_dev, sim->episode, N * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (pose_dev) HIP_TRY(sim, hipMemcpyAsync(pose_dev, sim->pose, N, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return OS2R_OK;
}

int os2r_set_episode_info(Os2rSim* sim, const int32_t* steps_dev, const uint32_t* episode_dev, const uint8_t* pose_dev, void* stream) {
  if (!sim) return OS2R_ERR_INVALID;
  DeviceGuard guard(sim->cfg.device);
  const size_t N = (size_t)sim->cfg.num_envs;
  if (steps_dev) HIP_TRY(sim, hipMemcpyAsync(sim->steps, steps_dev, N * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (episode_dev) HIP_TRY(sim, hipMemcpyAsync(sim->episode, episode_dev, N * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (pose_dev) HIP_TRY(sim, hipMemcpyAsync(sim->pose, pose_dev, N, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return OS2R_OK;
}

int os2r_model_is_compiled_in(const Os2rModel* model) {
  return model && os2r::static_model_id(*model) >= 0 ? 1 : 0;
}

int os2r_register_model_kernels(const Os2rModel* model, int32_t dtype, int32_t device, const char* path) {
  if (!model || !path || (dtype != OS2R_F32 && dtype != OS2R_F64)) { g_create_error = "os2r_register_model_kernels: bad argument"; return OS2R_ERR_INVALID; }
  DeviceGuard guard(device);
  if (hipSetDevice(device) != hipSuccess) { g_create_error = "os2r_register_model_kernels: hipSetDevice failed"; return OS2R_ERR_HIP; }
  JitEntry e;
  e.model = *model; e.dtype = dtype; e.device = device;
  hipError_t rc = hipModuleLoad(&e.module, path);
  if (rc != hipSuccess) { g_create_error = std::string("hipModuleLoad(") + path + "): " + hipGetErrorString(rc); return OS2R_ERR_HIP; }
  int found = 0;
  for (int c = 0; c < 2; ++c)
    for (int d = 0; d < 2; ++d) {
      const std::string name = std::string("os2r_jit_step_c") + char('0' + c) + "_d" + char('0' + d);
      for (int v = 0; v < 2; ++v)
        if (hipModuleGetFunction(&e.fn[c][d][v], e.module, (name + (v ? "_s" : "")).c_str()) == hipSuccess) ++found;
        else e.fn[c][d][v] = nullptr;
    }
  int fused = 0;
  for (int d = 0; d < 2; ++d) {
    const std::string tail = std::string("_c1_d") + char('0' + d);
    if (hipModuleGetFunction(&e.fn_rollout[d], e.module, ("os2r_jit_rollout" + tail).c_str()) == hipSuccess) ++fused;
    else e.fn_rollout[d] = nullptr;
    if (hipModuleGetFunction(&e.fn_policy[d], e.module, ("os2r_jit_policy" + tail).c_str()) == hipSuccess) ++fused;
    else e.fn_policy[d] = nullptr;
    for (int c = 0; c < 2; ++c)
      for (int v = 0; v < 2; ++v) {
        const std::string name = std::string("os2r_jit_lin_c") + char('0' + c) + "_d" + char('0' + d) + (v ? "_s" : "");
        if (hipModuleGetFunction(&e.fn_lin[c][d][v], e.module, name.c_str()) == hipSuccess) ++found;
        else e.fn_lin[c][d][v] = nullptr;
      }
  }
  found += fused;
  hipDeviceptr_t lay = nullptr;
  size_t lay_bytes = 0;
  if (hipModuleGetGlobal(&lay, &lay_bytes, e.module, "os2r_jit_policy_knots") == hipSuccess)
    for (int d = 0; d < 2; ++d)
      if (hipModuleGetFunction(&e.fn_policy_rec[d], e.module, (std::string("os2r_jit_policy_rec_c1_d") + char('0' + d)).c_str()) != hipSuccess)
        e.fn_policy_rec[d] = nullptr;
  lay = nullptr; lay_bytes = 0;
  if (hipModuleGetGlobal(&lay, &lay_bytes, e.module, "os2r_jit_layout") == hipSuccess && lay_bytes >= 3 * sizeof(unsigned long long)) {
    unsigned long long v[3] = {};
    const bool read = hipMemcpy(v, lay, sizeof(v), hipMemcpyDeviceToHost) == hipSuccess;
    // an object that announces a layout has it folded into its fused kernels: one that cannot be read serves no handle
    if (read) { e.fused_kinds = v[0]; e.fused_srcs = v[1]; e.fused_dim = (int)v[2]; }
    else if (fused) { found -= fused; for (int d = 0; d < 2; ++d) e.fn_rollout[d] = e.fn_policy[d] = e.fn_policy_rec[d] = nullptr; }
    if (read) {
      bool both = true;
      for (int d = 0; d < 2; ++d)
        if (hipModuleGetFunction(&e.fn_layout[d], e.module, (std::string("os2r_jit_step_c1_d") + char('0' + d) + "_l").c_str()) != hipSuccess) { e.fn_layout[d] = nullptr; both = false; }
      if (both) { e.layout_kinds = v[0]; e.layout_srcs = v[1]; e.layout_dim = (int)v[2]; }
    }
  }
  (void)hipGetLastError();   // a missing variant is not an error
  if (!found) { (void)hipModuleUnload(e.module); g_create_error = std::string(path) + " exports no os2r_jit_* kernel this library knows"; return OS2R_ERR_INVALID; }
  std::lock_guard<std::mutex> lock(g_jit_mutex);
  g_jit.push_back(e);
  return OS2R_OK;
}

int os2r_get_action_violations(Os2rSim* sim, uint32_t* dst, int32_t clear, void* stream) {
  if (!sim || !dst) return OS2R_ERR_INVALID;
  DeviceGuard guard(sim->cfg.device);
  HIP_TRY(sim, hipMemcpyAsync(dst, sim->violations, 4, hipMemcpyDefault, (hipStream_t)stream));
  if (clear) HIP_TRY(sim, hipMemsetAsync(sim->violations, 0, 4, (hipStream_t)stream));
  return OS2R_OK;
}

int os2r_get_violation_mirror(Os2rSim* sim, const volatile uint32_t** host_words) {
  if (!sim || !host_words) return OS2R_ERR_INVALID;
  *host_words = sim->mirror_host;
  return OS2R_OK;
}

int os2r_get_step_count(Os2rSim* sim, uint64_t* out) {
  if (!sim || !out) return OS2R_ERR_INVALID;
  *out = sim->step_count;
  return OS2R_OK;
}

int os2r_set_step_count(Os2rSim* sim, uint64_t value) {
  if (!sim) return OS2R_ERR_INVALID;
  sim->step_count = value;
  return OS2R_OK;
}

int os2r_bench_steps(Os2rSim* sim, int nsteps, void* stream, float* elapsed_ms) {
  if (!sim || nsteps < 1) return OS2R_ERR_INVALID;
  DeviceGuard guard(sim->cfg.device);
  hipStream_t st = (hipStream_t)stream;
  if (elapsed_ms) HIP_TRY(sim, hipEventRecord(sim->ev0, st));
  for (int k = 0; k < nsteps; ++k) {
    int rc = os2r_step(sim, nullptr, sim->b_obs, sim->b_rew, sim->b_done, sim->b_term, stream);
    if (rc) return rc;
  }
  if (!elapsed_ms) return OS2R_OK;   // enqueue only: several handles on several streams are timed by their caller
  HIP_TRY(sim, hipEventRecord(sim->ev1, st));
  // the caller's clock runs until this returns: poll the event instead of sleeping on it (a blocked host thread is woken tens of
  // microseconds after the last launch has finished -- 1-2 % of a 20-step window)
  for (;;) {
    const hipError_t q = hipEventQuery(sim->ev1);
    if (q == hipSuccess) break;
    if (q != hipErrorNotReady) { sim->err = std::string("hipEventQuery: ") + hipGetErrorString(q); return OS2R_ERR_HIP; }
  }
  HIP_TRY(sim, hipEventElapsedTime(elapsed_ms, sim->ev0, sim->ev1));
  return OS2R_OK;
}

int os2r_bench_steps_multi(Os2rSim* const* sims, void* const* streams, int count, int nsteps) {
  if (!sims || !streams || count < 1 || nsteps < 1) return OS2R_ERR_INVALID;
  for (int i = 0; i < count; ++i)
    if (!sims[i]) return OS2R_ERR_INVALID;
  for (int k = 0; k < nsteps; ++k)
    for (int i = 0; i < count; ++i) {
      Os2rSim* s = sims[i];
      int rc = os2r_step(s, nullptr, s->b_obs, s->b_rew, s->b_done, s->b_term, streams[i]);
      if (rc) return rc;
    }
  return OS2R_OK;
}

int os2r_set_work_counters(Os2rSim* sim, uint64_t* counters_dev) {
  if (!sim) return OS2R_ERR_INVALID;
  sim->counters = (unsigned long long*)counters_dev;
  return OS2R_OK;
}

int os2r_set_done_reasons(Os2rSim* sim, uint16_t* reason_dev) {
  if (!sim) return OS2R_ERR_INVALID;
  sim->reason = reason_dev;
  return OS2R_OK;
}

int os2r_set_done_mask(Os2rSim* sim, uint8_t* mask_dev) {
  if (!sim) return OS2R_ERR_INVALID;
  sim->done_mask = mask_dev;
  return OS2R_OK;
}

#ifdef OS2R_STAMPS
// diagnostic builds only (libos2r_stamps.so): per-wave phase stamps, kStamps x uint64 per workgroup
OS2R_API int os2r_debug_set_stamp_buffer(Os2rSim* sim, unsigned long long* buf_dev) {
  if (!sim) return OS2R_ERR_INVALID;
  sim->debug = buf_dev;
  return OS2R_OK;
}
#endif

const char* os2r_last_error(Os2rSim* sim) { return sim ? sim->err.c_str() : g_create_error.c_str(); }

// libos2r_record.so (include/os2r_record.h) is linked from these objects too and exports the os2rr_* functions only; there the
// thread's handle-less error text is that library's own copy
const char* os2rr_last_error(void) { return g_create_error.c_str(); }
int os2rr_abi_version(void) { return OS2R_RECORD_ABI_VERSION; }

}  // extern "C"
