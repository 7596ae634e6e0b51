// os2r_kernels.hpp — step / reset kernels: substeps + fused epilogue (observation, reward, done,
// auto-reset) in one launch.  Included by the per-dtype instantiation units.
#pragma once
#include "os2r_device.hpp"

namespace os2r {

// ----------------------------------------------------------------------------------------
// epilogue pieces.  Contraction is switched off so that the f64 path performs exactly the
// operations numpy performs in the reference (tasks/monopod.py:257-272, rewards/*.py): the
// affine maps, the periodic wrap and the polynomial sigmoids are then bit-identical.
// ----------------------------------------------------------------------------------------
// tanh for the velocity observations (tasks/monopod.py:270).  The library routine is 165 instructions and the
// epilogue calls it once per observed velocity; this one is ~85: below 0.55 the Taylor series of tanh(x)/x in
// x^2 (19 terms: truncation 5e-19 relative), above it 1 - 2/(exp(2|x|) + 1), whose result lies in [0.5, 1] so
// that the errors of exp, add and divide stay below two spacings.  Within 2 ulp of glibc's tanh on 2e8 arguments
// (tests allow 4).
__device__ __forceinline__ double tanh_t(double x) {
  constexpr double C[19] = {
      -0x1.5555555555555p-2, 0x1.1111111111111p-3, -0x1.ba1ba1ba1ba1cp-5, 0x1.664f4882c10fap-6,
      -0x1.226e355e6c23dp-7, 0x1.d6d3d0e157de0p-9, -0x1.7da36452b75e3p-10, 0x1.3558248036744p-11,
      -0x1.f57d7734d1664p-13, 0x1.967e18afcafadp-14, -0x1.497d8eea25259p-15, 0x1.0b132d39a6050p-16,
      -0x1.b0f72d3ee24e9p-18, 0x1.5ef2da474e5b7p-19, -0x1.1c77df95c1c0dp-20, 0x1.cd299de4ae6bbp-22,
      -0x1.75cde6563fed9p-23, 0x1.2efe8db3aff1fp-24, -0x1.eb3229047434cp-26};
  const double ax = __builtin_fabs(x);
  const bool small = ax < 0.55;
  double r = x;
  if (__ballot(small) != 0ull) {
    const double z = x * x;
    double p = C[18];
#pragma unroll
    for (int i = 17; i >= 0; --i) p = __builtin_fma(p, z, C[i]);
    r = __builtin_fma(x, z * p, x);
  }
  if (__ballot(!small) != 0ull) {
    // (the argument is capped where the result is 1 already: 2 |x| itself overflows in the last binade, and exp of an infinity is
    // a NaN under the no-infinity flags -- tanh_t(DBL_MAX) was a NaN; every finite result is what it was)
    const double t = exp(2.0 * __builtin_fmin(ax, 354.0));    // exp(708) = 3e307: the quotient is 7e-308, the result 1
    const double big = __builtin_copysign(1.0 - 2.0 / (t + 1.0), x);
    r = small ? r : big;
  }
  return r;
}
__device__ __forceinline__ float tanh_t(float x) { return tanhf(x); }
__device__ __forceinline__ double fmod_t(double a, double b) { return fmod(a, b); }
__device__ __forceinline__ float fmod_t(float a, float b) { return fmodf(a, b); }
__device__ __forceinline__ double atanh_t(double x) { return atanh(x); }
__device__ __forceinline__ float atanh_t(float x) { return atanhf(x); }

// numpy.mod(x + pi, 2*pi) - pi
template <typename T>
__device__ __forceinline__ T wrap_pi(T x) {
#pragma clang fp contract(off)
  const T pi = T(3.141592653589793238462643383279502884);
  const T two_pi = T(2) * pi;
  T m = fmod_t(x + pi, two_pi);
  if (m != T(0)) {
    if (m < T(0)) m += two_pi;
  } else {
    m = T(0);
  }
  return m - pi;
}

// value before the affine / tanh map, and the observation itself (tasks/monopod.py:238-272)
// Observation layout: which quantity feeds which slot and through which map.  It is data of the task
// (RtLayout: read from the task struct), and for the layouts of the reference's task modes on the compiled-in
// robots also a compile-time variant (StLayout): the slot loop below then folds into straight-line code --
// no per-slot dispatch on the kind, no select chains over the joints (they were ~500 cycles per slot for a
// wave that owns its SIMD: the whole observation 10.7 k cycles per env-step against 3 k of arithmetic).
struct RtLayout {
  static constexpr bool kStatic = false;
  static constexpr int kDim = 0;
  static constexpr int kind(int) { return 0; }
  static constexpr int src(int) { return 0; }
};
template <unsigned long long KINDS, unsigned long long SRCS, int DIM>
struct StLayout {
  static constexpr bool kStatic = true;
  static constexpr unsigned long long kKinds = KINDS, kSrcs = SRCS;
  static constexpr int kDim = DIM;
  static constexpr int kind(int d) { return (int)((KINDS >> (4 * d)) & 15ull); }
  static constexpr int src(int d) { return (int)((SRCS >> (4 * d)) & 15ull); }
};
constexpr unsigned long long pack_layout(const int* v, int n) {
  unsigned long long r = 0;
  for (int i = 0; i < n; ++i) r |= (unsigned long long)(v[i] & 15) << (4 * i);
  return r;
}

template <typename T, int NQ, typename LAY = RtLayout>
__device__ __forceinline__ void observe(TaskPtr<T> ts, const T (&q)[NQ], const T (&qd)[NQ],
                                        T h1a, T h1b, T (&obs)[OS2R_MAX_OBS], bool& done, unsigned& reason) {
#pragma clang fp contract(off)
  done = false;
  const unsigned fmask = exponent_mask(T(0));   // one opaque mask for the finite tests of all slots
  reason = 0u;   // bit d: observation slot d is outside the reset space (or not finite): which one ended the episode
  int D = LAY::kStatic ? LAY::kDim : ts->obs_dim;
  if constexpr (!LAY::kStatic) asm volatile("" : "+s"(D));   // one copy in a register: not re-fetched (and waited for) slot after slot
  // The slots' constants are fetched four slots at a time, ahead of the slots' arithmetic: left to the
  // point of use, every slot waits for five scalar loads in turn, which a lone wave cannot hide.
  constexpr int H = 4;
  static_assert(OS2R_MAX_OBS % H == 0, "whole batches");
#pragma unroll
  for (int batch = 0; batch < OS2R_MAX_OBS / H; ++batch) {
    if (LAY::kStatic && batch * H >= LAY::kDim) {
#pragma unroll
      for (int k = 0; k < H; ++k) obs[batch * H + k] = T(0);
      continue;
    }
    int kind_[H], src_[H];
    T lo_[H], hi_[H], dlo_[H], dhi_[H];
#pragma unroll
    for (int k = 0; k < H; ++k) {
      const int d = batch * H + k;
      kind_[k] = LAY::kStatic ? LAY::kind(d) : ts->obs_kind[d];
      src_[k] = LAY::kStatic ? LAY::src(d) : ts->obs_src[d];
      lo_[k] = ts->obs_low[d]; hi_[k] = ts->obs_high[d];
      dlo_[k] = ts->done_lo[d]; dhi_[k] = ts->done_hi[d];
    }
#pragma unroll
    for (int k = 0; k < H; ++k) {   // used here: the loads are not sunk into the branches below
      if constexpr (!LAY::kStatic) asm volatile("" : "+s"(kind_[k]), "+s"(src_[k]));
      asm volatile("" : "+s"(lo_[k]), "+s"(hi_[k]), "+s"(dlo_[k]), "+s"(dhi_[k]));
    }
#pragma unroll
    for (int k = 0; k < H; ++k) {
      const int d = batch * H + k;
      if (d >= D) { obs[d] = T(0); continue; }
      const int kind = kind_[k], s = src_[k];
      T x = T(0);
      if (kind == OS2R_OBS_TORQUE_NORM || kind == OS2R_OBS_TORQUE_RAW) {
        x = s == 0 ? h1a : h1b;
      } else if (kind == OS2R_OBS_VEL_TANH || kind == OS2R_OBS_VEL_RAW) {
#pragma unroll
        for (int i = 0; i < NQ; ++i) x = (s == i) ? qd[i] : x;
      } else {
#pragma unroll
        for (int i = 0; i < NQ; ++i) x = (s == i) ? q[i] : x;
      }
      if (kind == OS2R_OBS_POS_PERIODIC_NORM || kind == OS2R_OBS_POS_PERIODIC_RAW) x = wrap_pi(x);
      // done: the reference tests the observation against reset_space; done_lo/done_hi are the
      // exact pre-images of that test on x (host-side bisection), NaN counts as done
      if (x < dlo_[k] || x > dhi_[k] || !finite_t(x, fmask)) { done = true; reason |= 1u << d; }   // NaN counts as done
      T o = x;
      if (kind == OS2R_OBS_POS_NORM || kind == OS2R_OBS_POS_PERIODIC_NORM || kind == OS2R_OBS_TORQUE_NORM) {
        const T lo = lo_[k], hi = hi_[k];
        o = T(2) * (x - lo) / (hi - lo) - T(1);
      } else if (kind == OS2R_OBS_VEL_TANH) {
        o = tanh_t(T(0.05) * x);
      }
      obs[d] = o;
    }
  }
}

// rewards_utils.py:76-122 restricted to the sigmoids the reward classes use
template <typename T>
__device__ __forceinline__ T tol_quadratic(T x, T margin, T value_at_margin) {  // bounds (0,0)
#pragma clang fp contract(off)
  if (x == T(0)) return T(1);
  const T d = (x < T(0) ? T(0) - x : x - T(0)) / margin;
  const T sx = d * sqrt_t(T(1) - value_at_margin);
  return fabs_t(sx) < T(1) ? T(1) - sx * sx : T(0);
}
template <typename T>
__device__ __forceinline__ T tol_linear(T x, T margin, T value_at_margin) {  // bounds (0,0)
#pragma clang fp contract(off)
  if (x == T(0)) return T(1);
  const T d = (x < T(0) ? T(0) - x : x - T(0)) / margin;
  const T sx = d * (T(1) - value_at_margin);
  return fabs_t(sx) < T(1) ? T(1) - sx : T(0);
}

template <typename T>
__device__ __forceinline__ T pick_obs(const T (&obs)[OS2R_MAX_OBS], int idx) {
  T x = T(0);
#pragma unroll
  for (int d = 0; d < OS2R_MAX_OBS; ++d) x = (d == idx) ? obs[d] : x;
  return x;
}

// rewards/__init__.py:66-207.  a0 = actions[0] (just applied), a1 = actions[1] (previous)
template <typename T>
__device__ __forceinline__ T reward_of(TaskPtr<T> ts, const T (&obs)[OS2R_MAX_OBS], T a0x, T a0y,
                                       T a1x, T a1y) {
#pragma clang fp contract(off)
  const T nrm = ts->normalized ? T(1) : T(0);
  const T H = T(0.11) / T(1.57) * nrm + T(0.11) * (T(1) - nrm);
  const T bp = pick_obs(obs, ts->idx_pitch_pos);
  const T lo = H, hi = T(4) * H;
  const bool inb = (lo <= bp) && (bp <= hi);
  const T window = inb ? T(1) : T(0);
  switch (ts->reward_id) {
    case OS2R_REWARD_BALANCING_V1:
    case OS2R_REWARD_STANDING_V1:
      return window;
    case OS2R_REWARD_BALANCING_V2:
      return window * (tol_quadratic(a0x, T(1), T(0.4)) * tol_quadratic(a0y, T(1), T(0.4)));
    case OS2R_REWARD_BALANCING_V3: {
      T bal = T(1);
      if (!inb) {  // long_tail, margin 0.01, value_at_margin 0.1
        const T d = (bp < lo ? lo - bp : bp - hi) / T(0.01);
        const T t = d * sqrt_t(T(1) / T(0.1) - T(1));
        bal = T(1) / (t * t + T(1));
      }
      return bal * (tol_quadratic(a0x - a1x, T(1), T(0.1)) * tol_quadratic(a0y - a1y, T(1), T(0.1)));
    }
    case OS2R_REWARD_HOPPING_V1: {
      const T sd = tol_quadratic(a0x - a1x, T(0.1), T(0)) * tol_quadratic(a0y - a1y, T(0.1), T(0));
      const T hv = pick_obs(obs, ts->idx_yaw_vel);
      T move = T(1);
      if (!((T(0.25) <= hv) && (hv <= T(0.3)))) {  // tanh_squared, margin 0.15, value_at_margin 0.1
        const T d = (hv < T(0.25) ? T(0.25) - hv : hv - T(0.3)) / T(0.15);
        const T th = tanh_t(d * atanh_t(sqrt_t(T(1) - T(0.1))));
        move = T(1) - th * th;
      }
      return window * sd * move;
    }
    case OS2R_REWARD_STRAIGHT_V1: {
      T sc = (tol_quadratic(a0x / T(20), T(1), T(0)) + tol_quadratic(a0y / T(20), T(1), T(0))) / T(2);
      sc = (T(4) + sc) / T(5);
      const T hr = tol_linear(pick_obs(obs, ts->idx_hip_pos), T(1), T(0.1));
      const T kr = tol_linear(pick_obs(obs, ts->idx_knee_pos), T(1), T(0.1));
      return hr * kr * sc;
    }
    default:
      return T(0);
  }
}

// utils/reset.py:4-40
__device__ __forceinline__ void leg_joint_angles(const double (&def6)[6], double pitch, double& hip, double& knee) {
#pragma clang fp contract(off)
  const double ul = def6[0], ll = def6[1], cph = def6[2], lb = def6[3];
  const double lh = (lb * sin(pitch) + cph) / cos(pitch);
  const double lleg = lh - def6[4] - def6[5];
  if (lleg > ul + ll) { hip = 0.0; knee = 0.0; return; }
  const double ua = acos((ul * ul + lleg * lleg - ll * ll) / (2.0 * ul * lleg));
  const double la = asin(ul * sin(ua) / ll) + ua;
  hip = ua;
  knee = -la;
}

// Reset of one environment: randomizers/monopod_no_rand.py:59-98 (fixed) and
// randomizers/monopod.py:89-128,182-215 (randomised pose + parameter resampling).
// freshly sampled per-env parameters of a reset (written back by store_params)
template <typename T, int NQ>
struct ParamVals {
  T ms[NQ], dm[NQ], fr[NQ], mu_[NQ];
  bool fresh = false;
  T gravity = T(0);          // drawn anew after every `gravity_rollouts` rollouts of the environment
  bool gravity_fresh = false;
};

template <typename T, typename MD, bool DR>
__device__ __forceinline__ void reset_env(const StepArgs<T>& A, long long e, uint32_t epi, T (&q)[MD::NQ], T (&qd)[MD::NQ],
                                          ParamVals<T, MD::NQ>& par, uint8_t& pose) {
#pragma clang fp contract(off)
  constexpr int NQ = MD::NQ;
  const TaskPtr<T> ts = as_const(A.task);
  const uint32_t genv = (uint32_t)(A.env_offset + e);
  double u0, u1;
  uniform2(A.seed, genv, kStreamReset, epi, 0, u0, u1);
  int pi = (int)(u0 * ts->n_reset_poses);
  if (pi >= ts->n_reset_poses) pi = ts->n_reset_poses - 1;
  double pitch = 0, hip = 0, knee = 0, yaw = 0;
  int laying = 0, pid = 0;
  for (int k = 0; k < OS2R_MAX_RESET_POSES; ++k) {
    if (k == pi) { pitch = ts->reset_pitch[k]; hip = ts->reset_hip[k]; knee = ts->reset_knee[k]; laying = ts->reset_laying[k]; pid = ts->reset_pose_id[k]; }
  }
  if (ts->reset_mode == OS2R_RESET_FIXED) {
    if (ts->reset_simple) {
      double w0, w1;
      uniform2(A.seed, genv, kStreamReset, epi, 1, w0, w1);
      hip = 2.0 * w0 - 1.0;
      knee = 2.0 * w1 - 1.0;
    }
  } else {
    pitch *= 0.8 + 0.4 * u1;
    double z0, z1, w0, w1, x0, x1;
    normal2(A.seed, genv, kStreamReset, epi, 1, z0, z1);
    uniform2(A.seed, genv, kStreamReset, epi, 2, w0, w1);
    uniform2(A.seed, genv, kStreamReset, epi, 3, x0, x1);
    const double r0 = fabs(0.2 * z0), r1 = fabs(0.2 * z1);
    const double rmax = r0 > r1 ? r0 : r1, rmin = r0 > r1 ? r1 : r0;
    if (!laying) {
      double def6[6];
      for (int k = 0; k < 6; ++k) def6[k] = ts->leg_def[k];
      leg_joint_angles(def6, pitch, hip, knee);
    } else {
      hip = 1.57 - (w0 < 0.5 ? 3.14 : 0.0);
      knee = 0.0;
    }
    hip = hip + (hip > 0.0 ? 1.0 : 0.0) * rmax;
    knee = knee - (knee > 0.0 ? 1.0 : 0.0) * rmin;
    const double dir = 1.0 - (w1 < 0.5 ? 2.0 : 0.0);
    hip *= dir;
    knee *= dir;
    yaw = -0.2 + 0.4 * x0;
  }
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    double v = 0.0;
    if (i == ts->dof_pitch) v = pitch;
    if (i == ts->dof_yaw) v = yaw;
    if (i == ts->dof_hip) v = hip;
    if (i == ts->dof_knee) v = knee;
    q[i] = (T)v;
    qd[i] = T(0);
  }
  pose = (uint8_t)pid;
  if constexpr (DR) {
    if (ts->reset_mode == OS2R_RESET_RANDOM && ts->randomize_params) {
#pragma unroll
      for (int i = 0; i < NQ; ++i) {
        double a0, a1, b0, b1;
        uniform2(A.seed, genv, kStreamParams, epi, 2 * i, a0, a1);
        uniform2(A.seed, genv, kStreamParams, epi, 2 * i + 1, b0, b1);
        par.ms[i] = (T)(ts->dr_mass_lo + (ts->dr_mass_hi - ts->dr_mass_lo) * a0);
        par.fr[i] = (T)(ts->dr_friction_lo + (ts->dr_friction_hi - ts->dr_friction_lo) * a1);
        par.dm[i] = (T)(ts->nominal_damping[i] * (ts->dr_damping_lo + (ts->dr_damping_hi - ts->dr_damping_lo) * b0));
        par.mu_[i] = (T)(ts->dr_mu_base * (ts->dr_mu_lo + (ts->dr_mu_hi - ts->dr_mu_lo) * b1));
      }
      par.fresh = true;
    }
    // randomize_physics of the reference runs when its simulator is re-created, every `num_physics_rollouts`
    // rollouts (randomizers/monopod.py:36-41,56-61): `epi` rollouts of this environment are over now
    if (ts->reset_mode == OS2R_RESET_RANDOM && ts->gravity_rollouts > 0 && epi > 0u && epi % (uint32_t)ts->gravity_rollouts == 0u) {
      double z0, z1;
      normal2(A.seed, genv, kStreamGravity, epi / (uint32_t)ts->gravity_rollouts, 0, z0, z1);
      par.gravity = (T)(ts->dr_gravity_mean + ts->dr_gravity_std * z0);
      par.gravity_fresh = true;
    }
  }
}

// Binds the per-lane parameters of one env-step: nominal ones are compile-time / scalar constants; randomised ones are
// fetched from their HBM arrays into this lane's LDS slots (Params<.., true>), once per env-step.
template <typename T, typename MD, bool DR>
__device__ __forceinline__ void bind_params(const StepArgs<T>& A, long long e, const MD& md, Params<T, MD, DR>& par, T* slots) {
  par.m = md;
  if constexpr (!DR) par.g = A.gravity_z;
  if constexpr (DR) {
    constexpr int NQ = MD::NQ;
    par.g = A.gravity[e];
    // joint by joint: four values in flight, not twenty registers held at once (this runs where the state has just been loaded)
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const T ms = A.mass_scale[i * A.N + e], dm = A.damping[i * A.N + e], fr = A.friction[i * A.N + e], mu = A.mu[i * A.N + e];
      slots[(0 * NQ + i) * kWave] = md.mass(i) * ms;
      slots[(1 * NQ + i) * kWave] = dm;
      slots[(2 * NQ + i) * kWave] = fr;
      slots[(3 * NQ + i) * kWave] = mu;
    }
    par.slots = slots;
  }
}
template <typename T, int NQ>
__device__ __forceinline__ void store_params(const StepArgs<T>& A, long long e, const ParamVals<T, NQ>& pv) {
  if (pv.fresh) {
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      A.mass_scale[i * A.N + e] = pv.ms[i];
      A.damping[i * A.N + e] = pv.dm[i];
      A.friction[i * A.N + e] = pv.fr[i];
      A.mu[i * A.N + e] = pv.mu_[i];
    }
  }
  if (pv.gravity_fresh) A.gravity[e] = pv.gravity;
}

// Coalesced [N][D] row-major store of one wave's observation tile: the 64 rows of a wave are
// one contiguous block of 64*D values, so the tile goes through LDS and is written in lane order.
template <typename T>
__device__ __forceinline__ void store_obs_tile(T* __restrict__ dst, const T (&obs)[OS2R_MAX_OBS], int D, long long e0,
                                               long long N, int lane, T* tile) {
#pragma unroll
  for (int d = 0; d < OS2R_MAX_OBS; ++d)
    if (d < D) tile[lane * D + d] = obs[d];
  __syncthreads();
  const long long rows = (N - e0) < (long long)kWave ? (N - e0) : (long long)kWave;
  const int total = (int)rows * D;
  for (int k = lane; k < total; k += kWave) dst[e0 * D + k] = tile[k];
  __syncthreads();
}

// ----------------------------------------------------------------------------------------
// on-device linear policy (os2r_rollout_policy): a_j = squash(W_j . o + b_j)
// ----------------------------------------------------------------------------------------
// The argument of the policy kernels.  It begins with the StepArgs, so that step_body, which re-reads its arguments from the
// argument segment at offset 0, finds them there; StepArgs itself and every existing kernel stay as they are.
template <typename T>
struct PolicyArgs {
  StepArgs<T> s;
  const T* __restrict__ w;   // [2][D+1] shared, or [2][D+1][N] (OS2R_POLICY_PER_ENV); row j: W_j0 .. W_j,D-1, b_j
  int flags;                 // OS2R_POLICY_*
  T* __restrict__ ret;       // [N] or null: rewards summed in step order
  int32_t* __restrict__ len; // [N] or null: env-steps summed
  T* __restrict__ act;       // launch loop only: [N][2] actions the policy kernel hands to the step launch
  uint8_t* __restrict__ open;// launch loop only: [N] 1 while the environment's returns are still summed
  // os2r_rollout_policy_noisy (appended: the StepArgs stay at offset 0, the fields above where they were)
  const T* __restrict__ sigma;   // null: the deterministic policy; [2] shared, or [2][N] (OS2R_POLICY_SIGMA_PER_ENV)
  T* __restrict__ act_out;       // nullable: applied actions, [K][N][2] (fused) / step k's [N][2] slice (launch loop)
  T* __restrict__ eps_out;       // nullable: the noise eps, same shape
  uint32_t salt;                 // enters the noise counter: c1 = (c >> 32) ^ salt
  // os2r_rollout_policy_scheduled (appended likewise)
  int period;                    // 0: no schedule, w is one set; T >= 1: w is [T] sets, one per slot
  int first_slot;                // the clock's offset: the fused kernel adds its step index k, the launch loop's host has added it
  // os2rr_rollout_policy_recorded (appended likewise): the sink of the knots.  At the top of env-step k environment e goes to lane
  // knot_lane + k * N + e of another handle, whose arrays are [rows][knot_stride]: the row bases below are that handle's own
  int knot_what;                 // OS2R_COPY_* bits; 0: no handle to record into
  long long knot_stride;         // the destination's num_envs
  long long knot_lane;           // first_knot * N (launch loop: (first_knot + k) * N is in the copy launch, this stays unused)
  T* __restrict__ kq;            // OS2R_COPY_STATE: [nq][stride]
  T* __restrict__ kqd;           // [nq][stride]
  T* __restrict__ khist;         // [4][stride]
  T* __restrict__ ksolver_l;     // [4 nq][stride]
  uint32_t* __restrict__ ksolver_flags;
  int32_t* __restrict__ ksteps;
  uint32_t* __restrict__ kepisode;
  uint8_t* __restrict__ kpose;
  T* __restrict__ kmass_scale;   // OS2R_COPY_PARAMS: [nq][stride] each, gravity [stride]
  T* __restrict__ kdamping;
  T* __restrict__ kfriction;
  T* __restrict__ kmu;
  T* __restrict__ kgravity;
  T* __restrict__ knot_obs;      // nullable: the observation the policy evaluates, [K][N][D] (fused) / step k's [N][D] slice (launch loop)
};

// The one policy function of both paths (fused rollout, launch loop).  Evaluation order is part of the contract
// (include/os2r.h): z_j = (((b_j + W_j0*o_0) + W_j1*o_1) + ...), each product rounded on its own.  Shared weights are
// wave-uniform: one scalar base, every lane the same address (the compiler issues 16-byte vector loads off that base, all of
// them ahead of the first product); per-env ones are [2(D+1)][N] and load coalesced.
template <typename T>
__device__ __forceinline__ void policy_presquash(const T* __restrict__ w, int flags, int D, long long N, long long e,
                                                 const T (&obs)[OS2R_MAX_OBS], T (&z)[2]) {
#pragma clang fp contract(off)
  const int R = D + 1;
  if (flags & OS2R_POLICY_PER_ENV) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      T acc = w[(long long)(j * R + D) * N + e];
#pragma unroll
      for (int d = 0; d < OS2R_MAX_OBS; ++d)
        if (d < D) acc = acc + w[(long long)(j * R + d) * N + e] * obs[d];
      z[j] = acc;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      T acc = w[j * R + D];
#pragma unroll
      for (int d = 0; d < OS2R_MAX_OBS; ++d)
        if (d < D) acc = acc + w[j * R + d] * obs[d];
      z[j] = acc;
    }
  }
}

template <typename T>
__device__ __forceinline__ void policy_squash(int flags, T (&z)[2]) {
  if (flags & OS2R_POLICY_TANH) {
    z[0] = tanh_t(z[0]);
    z[1] = tanh_t(z[1]);
  } else {
#pragma unroll
    for (int j = 0; j < 2; ++j) z[j] = z[j] < T(-1) ? T(-1) : (z[j] > T(1) ? T(1) : z[j]);
  }
}

// Exploration noise (os2r_rollout_policy_noisy): one Philox block of stream 5 keyed by (seed, global environment index, step
// counter c, salt) gives the two normals of hip and knee -- evaluated in double in the fp32 kernels too, then rounded once, so
// that both dtypes share one noise stream --; y_j = z_j + (sigma_j * eps_j), the product rounded on its own.
template <typename T>
__device__ __forceinline__ void policy_noise(const T* __restrict__ sigma, int flags, long long N, long long e,
                                             unsigned long long seed, uint32_t genv, unsigned long long c, uint32_t salt,
                                             T (&z)[2], T (&eps)[2]) {
#pragma clang fp contract(off)
  double n0, n1;
  normal2(seed, genv, kStreamPolicyNoise, (uint32_t)c, (uint32_t)(c >> 32) ^ salt, n0, n1);
  eps[0] = (T)n0;
  eps[1] = (T)n1;
  const bool per_env = (flags & OS2R_POLICY_SIGMA_PER_ENV) != 0;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const T sg = per_env ? sigma[(long long)j * N + e] : sigma[j];
    const T d = sg * eps[j];
    z[j] = z[j] + d;
  }
}

// The slot of a time-scheduled policy (os2r_rollout_policy_scheduled): t >= 0 is held at period - 1, or wraps.  t < 2^32, period
// < 2^31: the remainder is taken of each 32-bit summand on its own (a 64-bit remainder is a hundred instructions).
__device__ __forceinline__ long long policy_slot(int flags, int period, unsigned first, unsigned dt) {
  const unsigned per = (unsigned)period;
  if (flags & OS2R_POLICY_SCHEDULE_WRAP) {
    const unsigned s = first % per + dt % per;   // < 2 * per: no carry
    return (long long)(s >= per ? s - per : s);
  }
  const long long t = (long long)first + (long long)dt;
  return t < (long long)per - 1 ? t : (long long)per - 1;
}

// a = squash(z + sigma * eps) of environment e (lane `valid`: not a shadow lane of a tail wave) in the env-step with counter c,
// the k-th of the fused window (launch loop: 0); the action and, with P.sigma, the noise go to act_out / eps_out + 2 * at
// (nullable).  The branches on P.sigma, P.period and the clock flag are wave-uniform: they test kernel arguments.
// With a schedule (P.period > 0) the weights are those of the environment's slot, [period] sets in the layout of one:
//   window clock   slot of first_slot + k, the same for every lane: scalar arithmetic on the base, after which the shared set's
//                  loads are the wave-uniform ones of the one-set path and the per-env ones coalesced
//   episode clock  slot of first_slot + steps[e] (one 4-byte load by the lane; a negative count is taken as 0): a base per lane.
//                  The shared table is gathered -- 2(D+1) independent loads from [period][2][D+1], issued together ahead of the
//                  first product --; per-env, every lane reads its own column at its own slot
template <typename T>
__device__ __forceinline__ void policy_action(const PolicyArgs<T>* P, const StepArgs<T>& A, int D, long long e, bool valid,
                                              unsigned long long c, int k, long long at, const T (&obs)[OS2R_MAX_OBS], T& ax,
                                              T& ay) {
  const int flags = P->flags;
  T z[2];
  if (P->period == 0) {
    policy_presquash<T>(P->w, flags, D, A.N, e, obs, z);
  } else {
    // elements between two slots
    const long long stride = (long long)(2 * (D + 1)) * ((flags & OS2R_POLICY_PER_ENV) ? A.N : 1ll);
    if (flags & OS2R_POLICY_CLOCK_EPISODE) {
      const int st = A.steps[e];
      const long long slot = policy_slot(flags, P->period, (unsigned)P->first_slot, (unsigned)(st < 0 ? 0 : st));
      policy_presquash<T>(P->w + slot * stride, flags, D, A.N, e, obs, z);
    } else {
      const long long slot = policy_slot(flags, P->period, (unsigned)P->first_slot, (unsigned)k);
      policy_presquash<T>(P->w + slot * stride, flags, D, A.N, e, obs, z);
    }
  }
  if (P->sigma) {
    T eps[2];
    policy_noise<T>(P->sigma, flags, A.N, e, A.seed, (uint32_t)(A.env_offset + e), c, P->salt, z, eps);
    policy_squash<T>(flags, z);
    if (valid) {
      if (P->act_out) { P->act_out[2 * at] = z[0]; P->act_out[2 * at + 1] = z[1]; }
      if (P->eps_out) { P->eps_out[2 * at] = eps[0]; P->eps_out[2 * at + 1] = eps[1]; }
    }
  } else {
    policy_squash<T>(flags, z);
    if (valid && P->act_out) { P->act_out[2 * at] = z[0]; P->act_out[2 * at + 1] = z[1]; }
  }
  ax = z[0];
  ay = z[1];
}

// os2rr_rollout_policy_recorded, fused: `ROWS` rows of an SoA array from column e of the source ([rows][Ns]) to column `at` of the
// sink ([rows][Nd]), memory to memory: the loads of a group are issued ahead of its stores (copy_envs_kernel's kCopyGroup), the
// registers live for the group only.  Tail lanes load the environment they shadow and store nothing.
constexpr int kKnotGroup = 8;
template <typename T, int ROWS>
__device__ __forceinline__ void knot_rows(const T* __restrict__ src, long long Ns, long long e, T* __restrict__ dst, long long Nd,
                                          long long at, bool valid) {
#pragma unroll
  for (int r0 = 0; r0 < ROWS; r0 += kKnotGroup) {
    T v[kKnotGroup];
#pragma unroll
    for (int k = 0; k < kKnotGroup; ++k)
      if (r0 + k < ROWS) v[k] = src[(long long)(r0 + k) * Ns + e];
    if (valid) {
#pragma unroll
      for (int k = 0; k < kKnotGroup; ++k)
        if (r0 + k < ROWS) dst[(long long)(r0 + k) * Nd + at] = v[k];
    }
  }
}

// Environment e as it stands at the top of env-step k -- q and qd in the registers just loaded, everything else in the arrays the
// previous env-step (or launch) left -- becomes lane knot_lane + k N + e of the sink: the rows os2r_copy_envs moves for `what`,
// all 4 nq solver rows among them (also the ones this kernel does not load: the copy is exact for impulses it does not remember,
// and in fp32, where they are carried unused).  What this lane reads here it has written itself, one env-step earlier, in program
// order; nothing reads the sink in this launch.
template <typename T, int NQ>
__device__ __forceinline__ void record_knot(const PolicyArgs<T>* P, const StepArgs<T>& A, long long e, bool valid, int k,
                                            const T (&q)[NQ], const T (&qd)[NQ]) {
  const int what = P->knot_what;
  const long long Nd = P->knot_stride, at = P->knot_lane + (long long)k * A.N + e;
  if (what & OS2R_COPY_STATE) {
    if (valid) {
#pragma unroll
      for (int i = 0; i < NQ; ++i) {
        P->kq[i * Nd + at] = q[i];
        P->kqd[i * Nd + at] = qd[i];
      }
    }
    knot_rows<T, 4>(A.hist, A.N, e, P->khist, Nd, at, valid);
    knot_rows<T, 4 * NQ>(A.solver_l, A.N, e, P->ksolver_l, Nd, at, valid);
    const uint32_t fl = A.solver_flags[e], ep = A.episode[e];
    const int32_t st = A.steps[e];
    const uint8_t po = A.pose[e];
    if (valid) {
      P->ksolver_flags[at] = fl;
      P->ksteps[at] = st;
      P->kepisode[at] = ep;
      P->kpose[at] = po;
    }
  }
  if (what & OS2R_COPY_PARAMS) {
    knot_rows<T, NQ>(A.mass_scale, A.N, e, P->kmass_scale, Nd, at, valid);
    knot_rows<T, NQ>(A.damping, A.N, e, P->kdamping, Nd, at, valid);
    knot_rows<T, NQ>(A.friction, A.N, e, P->kfriction, Nd, at, valid);
    knot_rows<T, NQ>(A.mu, A.N, e, P->kmu, Nd, at, valid);
    knot_rows<T, 1>(A.gravity, A.N, e, P->kgravity, Nd, at, valid);
  }
}

// ----------------------------------------------------------------------------------------
// env-step kernel: GazeboRuntime.step (runtimes/gazebo_runtime.py:65-97) for every env
// ----------------------------------------------------------------------------------------
// LDS of one wave: during the physics iterations it holds the Minv*J^T rows of the contact
// problem (3 rows x NQ values per body, one slot per lane); afterwards the same storage is the
// observation tile of the coalesced [N][D] store.
template <int NQ>
constexpr int lds_words() {
  // Cholesky factor of Minv / per-joint ABA data (U, 1/D, u)
  constexpr int rows = NQ * (NQ + 1) / 2, aba = 8 * NQ;
  constexpr int m = rows > aba ? rows : aba;
  return kWave * (m > OS2R_MAX_OBS ? m : OS2R_MAX_OBS);
}
// wave-shared copy of the contact candidate table, behind the per-lane slots
constexpr int kCandWords = 3 * OS2R_MAX_CAND;

template <typename T, typename MD>
__device__ __forceinline__ MD make_model(const StepArgs<T>& A) {
  if constexpr (MD::kStatic) return MD{};
  else return MD{as_const(A.model)};
}

// One env-step of this wave's 64 environments: the body of every step kernel (the templated ones below and
// the model-specialised ones of os2r_jit_unit.hip).  STD_SWEEPS: the solver's sweep counts are the default
// ones and known at compile time (the launcher checks the handle's configuration).
// COUNT: the counting variant (os2r_set_work_counters): same arithmetic, and the wave's work of the launch is added to
// A.counters[0..kWorkCounters) by one lane at the end.
constexpr int kWorkCounters = OS2R_NUM_WORK_COUNTERS;
// SOLVER (os2r_device.hpp): kSolverBoth unless the launcher knows the handle's solver
constexpr int std_solver(bool std_sweeps, bool is_f64, bool std_exact) {
  return !is_f64 ? kSolverSweeps : (std_sweeps ? (std_exact ? kSolverExact : kSolverSweeps) : kSolverBoth);
}
// ROLLOUT: A.rollout_steps env-steps in this launch (os2r_rollout): every wave advances its own 64 environments step
// after step -- no device-wide barrier between the env-steps, where one launch per env-step makes 1024 waves wait for
// the slowest -- with the state in registers from the first step to the last; step k writes its observation, reward,
// done flag (terminal observation, done reason) at offset k of the [K][N]... output arrays and takes its actions from
// slice k of the [K][N][2] input (or draws them with the step counter + k).  The arithmetic of a step is the same code.
// POLICY (with ROLLOUT; os2r_rollout_policy): the kernel's argument is a PolicyArgs; each step's action is the linear policy of
// the observation the environment's previous step returned -- recomputed from the state the step loads anyway -- and the
// owning lane adds the step's reward and count to the environment's return and length.
// RECORD (with POLICY; os2rr_rollout_policy_recorded): at the top of every env-step the environment goes to the sink named in the
// PolicyArgs.  A variant of its own (policy_record_kernel): as a run-time branch of the POLICY kernels it cost calls that record
// nothing 1.4 - 3 % of their rate.
template <typename T, typename MD, bool CONTACT, bool DR, bool STD_SWEEPS = false, typename LAY = RtLayout, bool COUNT = false,
          int SOLVER = std_solver(STD_SWEEPS, sizeof(T) == 8, StdSolver<T>::kExact), bool ROLLOUT = false, bool POLICY = false,
          bool RECORD = false>
__device__ __forceinline__ void step_body(const StepArgs<T>& A) {
  static_assert(!POLICY || ROLLOUT, "the policy runs in the fused rollout");
  static_assert(!RECORD || POLICY, "the knots are recorded by the policy rollout");
  constexpr int NQ = MD::NQ;
  // run-time models scan a wave-shared LDS copy of the candidate table; the compiled-in ones read the
  // (wave-uniform) coordinates through scalar loads, straight into the operands of the scan
  constexpr bool kCandInLds = CONTACT && MD::CMASK != 0u && !MD::kStatic;
#ifdef OS2R_STAMPS
  const unsigned long long stamp_entry = __builtin_amdgcn_s_memtime();
  const unsigned long long real_entry = __builtin_amdgcn_s_memrealtime();
#endif
  // [per-lane slots of the physics iteration | per-lane parameter slots (DR) | wave-shared candidate table (run-time models)]
  constexpr int kParamWords = DR ? 4 * NQ * kWave : 0;
  __shared__ T tile[lds_words<NQ>() + kParamWords + (kCandInLds ? kCandWords : 0)];
  const int lane = threadIdx.x;
  const long long e0 = (long long)blockIdx.x * kWave;
  const bool valid = e0 + lane < A.N;
  const long long e_lane = valid ? e0 + lane : A.N - 1;  // tail lanes shadow the last env, stores are masked
  const MD md = make_model<T, MD>(A);
  T* cand_lds = tile + lds_words<NQ>() + kParamWords;
  if constexpr (kCandInLds) {
    const int nc3 = 3 * md.cand_begin(NQ);
    for (int k = lane; k < nc3; k += kWave) cand_lds[k] = md.cand(k / 3, k % 3);
    __syncthreads();
  }
  const TaskPtr<T> ts_launch = as_const(A.task);
  const int D = LAY::kStatic ? LAY::kDim : ts_launch->obs_dim;
  // The host's view of the clamped-action count (os2r_get_violation_mirror): the first wave of a launch copies the count that
  // every EARLIER launch left -- they have all finished: stream order -- and this launch's step counter into two words of mapped
  // host memory, so a host binding can look at it without a copy, an event or a wait on the step path.
  if (blockIdx.x == 0 && lane == 0 && A.mirror) {
    const unsigned seen = __hip_atomic_load(A.violations, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(A.mirror, seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(A.mirror + 1, (uint32_t)A.step_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
#ifdef OS2R_STAMPS
  unsigned long long stamps[kStamps] = {}, stamp_prev = __builtin_amdgcn_s_memtime();
  stamps[10] = stamp_prev - stamp_entry;   // prologue: loads, action, torques
#endif
  T sn[NQ], cs[NQ];   // sin/cos of the joint angles, carried from one physics iteration to the next
  WorkCounts wc;
  const int nsteps = ROLLOUT ? A.rollout_steps : 1;
  [[maybe_unused]] bool summing = true;   // POLICY: this environment's return and length still take its steps
  for (int k = 0; k < nsteps; ++k) {
    const long long ko = ROLLOUT ? (long long)k * A.N : 0ll;   // this step's slice of the output arrays
    // (a rollout passes the state from one env-step to the next through memory like separate launches do -- its own
    // lines, L2-resident: held in registers across the epilogue it costs the 5-dof kernels 140-390 B of scratch per lane --
    // and its environment index is a fresh value in every step: otherwise the address of every state array, sixty of
    // them, is hoisted out of the step loop and held in registers across it: 450 B of scratch)
    long long e = e_lane;
    if constexpr (ROLLOUT) asm volatile("" : "+v"(e));
    TaskPtr<T> ts = ts_launch;   // (and the task's constants are fetched where they are used, step by step)
    if constexpr (ROLLOUT) asm volatile("" : "+s"(ts));
    T q[NQ], qd[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      q[i] = A.q[i * A.N + e];
      qd[i] = A.qd[i * A.N + e];
    }
    Params<T, MD, DR> par;
    bind_params<T, MD, DR>(A, e, md, par, tile + lds_words<NQ>() + lane);

    // what the exact finish hands from one physics iteration to the next (os2r_device.hpp): part of the environment's state
    constexpr bool kCarry = sizeof(T) == 8 && SOLVER != kSolverSweeps;
    SolverCarry<T, NQ> carry;
    if constexpr (kCarry) {
      carry.act = A.solver_flags[e];
#pragma unroll
      for (int b = 0; b < NQ; ++b) {
        if (CONTACT && ((MD::CMASK >> b) & 1u)) {
          carry.ln[b] = A.solver_l[(0 * NQ + b) * A.N + e];
          carry.lx[b] = A.solver_l[(1 * NQ + b) * A.N + e];
          carry.ly[b] = A.solver_l[(2 * NQ + b) * A.N + e];
        }
        carry.lf[b] = A.solver_l[(3 * NQ + b) * A.N + e];
      }
    }
    const unsigned long long step_count = A.step_count + (unsigned long long)k;
    // action: caller-provided or drawn from the counter RNG (stream 1, counter = step count)
    T ax, ay;
    if constexpr (POLICY) {
      // the observation the previous step (or reset) returned: observe() of the stored state, as reset_kernel makes it
      // (the weights are loaded here and are dead before the physics iterations)
      const PolicyArgs<T>* pa = (const PolicyArgs<T>*)__builtin_amdgcn_kernarg_segment_ptr();
      // os2rr_rollout_policy_recorded: the environment as it stands here goes to the sink, before anything of the step is formed
      // (a wave-uniform test of a kernel argument; the sink's pointers are read from the argument segment here, step by step,
      // and are dead before the physics iterations, like the weights)
      if constexpr (RECORD) {
        if (pa->knot_what != 0) {
          const PolicyArgs<T>* pk = pa;
          asm volatile("" : "+s"(pk));
          record_knot<T, NQ>(pk, A, e, valid, k, q, qd);
        }
      }
      const T h2x = A.hist[2 * A.N + e], h2y = A.hist[3 * A.N + e];
      T o[OS2R_MAX_OBS];
      bool dn0;
      unsigned why0;
      observe<T, NQ, LAY>(ts, q, qd, h2x, h2y, o, dn0, why0);
      if constexpr (RECORD) {
        if (pa->knot_obs) {
          // ... and the observation the policy is about to see, knot-major [K][N][D] (the tile is free until the physics iterations)
          const PolicyArgs<T>* pk = pa;
          asm volatile("" : "+s"(pk));
          store_obs_tile<T>(pk->knot_obs + ko * D, o, D, e0, A.N, lane, tile);
        }
      }
      // (with sigma: the noise is drawn and a, eps of step k are stored here by the owning lane: nothing of it lives on)
      policy_action<T>(pa, A, D, e, valid, step_count, k, ko + e, o, ax, ay);
    } else if (A.actions) {
      ax = A.actions[2 * (ko + e)];
      ay = A.actions[2 * (ko + e) + 1];
      // (the lanes behind the last environment of a tail wave shadow it and must not count its action again)
      const bool outside = (ax < T(-1) || ax > T(1) || ay < T(-1) || ay > T(1)) && e0 + lane < A.N;
      if (__ballot(outside) != 0ull && outside && A.violations) atomicAdd(A.violations, 1u);
    } else {
      double u0, u1;
      uniform2(A.seed, (uint32_t)(A.env_offset + e), kStreamAction, (uint32_t)step_count, (uint32_t)(step_count >> 32), u0, u1);
      ax = (T)(2.0 * u0 - 1.0);
      ay = (T)(2.0 * u1 - 1.0);
    }
    ax = ax < T(-1) ? T(-1) : (ax > T(1) ? T(1) : ax);
    ay = ay < T(-1) ? T(-1) : (ay > T(1) ? T(1) : ay);
    T tau_hip, tau_knee, asx, asy;
    {
#pragma clang fp contract(off)
      tau_hip = md.max_torque(0) * ax;    // tasks/monopod.py:223
      tau_knee = md.max_torque(1) * ay;
      asx = tau_hip / md.max_torque(0);   // what action_history stores (:233-235)
      asy = tau_knee / md.max_torque(1);
    }

    for (int s = 0; s < A.substeps; ++s) {  // runtimes/gazebo_runtime.py:70-77
      substep<T, MD, CONTACT, DR, COUNT, SOLVER>(
                                         md, par, q, qd, sn, cs, s == 0, tau_hip, tau_knee, A.dt, A.erp, A.max_erv, A.margin,
                                         STD_SWEEPS ? std_iters<T>(NQ) : A.pgs_iters, STD_SWEEPS ? StdSolver<T>::kNormalIters : A.pgs_normal_iters,
                                         A.pgs_exact, A.pgs_tol, tile, cand_lds, as_const(A.model), wc, carry
#ifdef OS2R_STAMPS
                                         , stamps, stamp_prev
#endif
      );
    }
    __syncthreads();
    // Everything behind the physics iterations addresses the environment through a value the compiler cannot see through:
    // otherwise the addresses of the arrays stored below -- sixty 64-bit values -- are computed at the top of the kernel and
    // held in registers across the physics loop (measured: 36 AGPR copies more for the solver's state alone).
    long long ep = e;
    asm volatile("" : "+v"(ep));
    // ... and reads the kernel arguments afresh from the argument segment: held in scalar registers from the top of the kernel
    // they (two dozen pointers) are spilled to VGPR lanes across the physics loop
    const OS2R_CONST StepArgs<T>* args_e = (const OS2R_CONST StepArgs<T>*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(args_e));
    const StepArgs<T>& Ae = *(const StepArgs<T>*)args_e;
    // (This reads the argument segment at offset 0: every kernel that inlines step_body -- step_kernel below, the run-time
    // code objects of os2r_jit_unit.hip -- takes ONE argument, the StepArgs by value.  A wrapper with another leading argument
    // would read garbage here; the counting variants, which the tests and bench.py's replay run, check it and trap.)
    if constexpr (COUNT) {
      if (Ae.N != A.N || Ae.q != A.q || Ae.solver_l != A.solver_l) __builtin_trap();
    }
    // The contact solver's state goes back to HBM here, straight after the last physics iteration: held until the end of
    // the env-step it would be live across the whole epilogue -- forty registers more at the kernel's widest point.
    if constexpr (kCarry) {
      if (valid) {
        Ae.solver_flags[ep] = carry.act;
#pragma unroll
        for (int b = 0; b < NQ; ++b) {
          // (an impulse that is not remembered is stored as zero: the arrays are a function of the trajectory alone)
          const bool cb = ((carry.act >> b) & 1u) != 0u;
          Ae.solver_l[(0 * NQ + b) * Ae.N + ep] = cb ? carry.ln[b] : T(0);
          Ae.solver_l[(1 * NQ + b) * Ae.N + ep] = cb ? carry.lx[b] : T(0);
          Ae.solver_l[(2 * NQ + b) * Ae.N + ep] = cb ? carry.ly[b] : T(0);
          Ae.solver_l[(3 * NQ + b) * Ae.N + ep] = carry.lf[b];
        }
      }
    }

    bool bad = false;
#pragma unroll
    for (int i = 0; i < NQ; ++i) bad = bad || wild_t(q[i]) || wild_t(qd[i]);     // not finite, or beyond 1e30

    // (the bookkeeping of an environment -- action history, step and episode counters -- is fetched where it is used and
    // stored at the end of every env-step, in a rollout as well: nothing of it is held across the physics iterations)
    const T h1x = Ae.hist[0 * Ae.N + ep], h1y = Ae.hist[1 * Ae.N + ep];  // becomes action_history[1]
    T obs[OS2R_MAX_OBS];
    bool dn;
    unsigned why;
    OS2R_STAMP(20);
    observe<T, NQ, LAY>(ts, q, qd, h1x, h1y, obs, dn, why);
    OS2R_STAMP(21);
    const T rew = reward_of<T>(ts, obs, asx, asy, h1x, h1y);
    OS2R_STAMP(22);
    int steps = Ae.steps[ep] + 1;
    const bool trunc = ts->max_episode_steps > 0 && steps >= ts->max_episode_steps;
    const uint8_t flag = (uint8_t)((dn ? 1 : 0) | (trunc ? 2 : 0) | (bad ? 4 : 0));

    if (Ae.term_obs) store_obs_tile<T>(Ae.term_obs + ko * D, obs, D, e0, Ae.N, lane, tile);

    uint32_t epi = Ae.episode[ep];
    uint8_t pose = Ae.pose[ep];
    const bool do_reset = flag != 0 && Ae.auto_reset != 0;
    ParamVals<T, NQ> pv;
    if (__ballot(do_reset) != 0ull) {
      if (do_reset) {
        reset_env<T, MD, DR>(Ae, ep, epi, q, qd, pv, pose);
        epi += 1;
        steps = 0;
        bool dn2;
        unsigned why2;
        observe<T, NQ, LAY>(ts, q, qd, h1x, h1y, obs, dn2, why2);
        // a new episode: the contact solver remembers nothing
        if constexpr (kCarry) {
          if (valid) {
            Ae.solver_flags[ep] = 0u;
#pragma unroll
            for (int k = 0; k < 4 * NQ; ++k) Ae.solver_l[k * Ae.N + ep] = T(0);
          }
        }
      }
    }
    if (Ae.obs) store_obs_tile<T>(Ae.obs + ko * D, obs, D, e0, Ae.N, lane, tile);
    OS2R_STAMP(23);
    if (valid) {
      Ae.hist[2 * Ae.N + ep] = h1x;
      Ae.hist[3 * Ae.N + ep] = h1y;
      Ae.hist[0 * Ae.N + ep] = asx;
      Ae.hist[1 * Ae.N + ep] = asy;
      Ae.steps[ep] = steps;
      if (do_reset) {
        Ae.episode[ep] = epi;
        Ae.pose[ep] = pose;
        store_params<T, NQ>(Ae, ep, pv);
      }
      if (Ae.reward) Ae.reward[ko + ep] = rew;
      if (Ae.done) Ae.done[ko + ep] = flag;
      if (Ae.reason) Ae.reason[ko + ep] = (uint16_t)why;
      if (Ae.done_mask) Ae.done_mask[ko + ep] = flag != 0 ? (uint8_t)1 : (uint8_t)0;
      if constexpr (POLICY) {
        // return and length: a read-modify-write by the owning lane (the same lines as the state), started afresh at k = 0
        const PolicyArgs<T>* pe = (const PolicyArgs<T>*)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(pe));
        if (summing) {
          if (pe->ret) pe->ret[ep] = (k == 0 ? T(0) : pe->ret[ep]) + rew;
          if (pe->len) pe->len[ep] = (k == 0 ? 0 : pe->len[ep]) + 1;
        }
        if ((pe->flags & OS2R_POLICY_FIRST_EPISODE) && flag != 0) summing = false;
      }
    }
    if (valid) {
#pragma unroll
      for (int i = 0; i < NQ; ++i) {
        Ae.q[i * Ae.N + ep] = q[i];
        Ae.qd[i * Ae.N + ep] = qd[i];
      }
    }
    if constexpr (ROLLOUT) {
      // the next step of this lane reads what this one has just written: same lane, same addresses, program order (vector
      // memory operations of a wave are performed in order); the compiler is kept from moving those loads up
      asm volatile("" ::: "memory");
    }
  }
  if constexpr (COUNT) {
    if (A.counters && lane == 0) {
      const unsigned long long v[kWorkCounters] = {(unsigned long long)A.substeps * (unsigned long long)nsteps, wc.scanned, wc.row_bodies, wc.body_sweeps,
                                                    wc.sweeps, wc.lane_contacts, wc.live_lane_sweeps, wc.full_sincos,
                                                    wc.exact_solves, wc.lane_exact_solves};
#pragma unroll
      for (int k = 0; k < kWorkCounters; ++k) atomicAdd(A.counters + k, v[k]);
    }
  }

#ifdef OS2R_STAMPS
  stamps[11] = __builtin_amdgcn_s_memtime() - stamp_prev;   // the state and flag stores, issued
  // the wave's life in shader-clock ticks and in ticks of the constant 100 MHz counter: their quotient is the clock
  // the chip held under this load (MI355X_MICROARCH.md, DVFS give-back (6))
  stamps[24] = __builtin_amdgcn_s_memtime() - stamp_entry;
  const unsigned long long real_exit = __builtin_amdgcn_s_memrealtime();
  stamps[25] = real_exit - real_entry;
#ifdef OS2R_STAMPS_LIGHT
  stamps[22] = real_entry;   // absolute: comparable between the waves of a launch
  stamps[23] = real_exit;
  {
    unsigned hw_id;            // where the wave ran: XCC_ID / SE / CU / SIMD fields of HW_ID and XCC_ID
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));
    unsigned xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    stamps[21] = ((unsigned long long)xcc << 32) | hw_id;
  }
#endif
  if (A.debug && lane == 0)
    for (int k = 0; k < kStamps; ++k) A.debug[blockIdx.x * kStamps + k] = stamps[k];
#endif
}

// Registers decide how many waves share a SIMD.  fp64 state needs ~370 registers (256 VGPR + AGPR copies): one wave.
// The fp32 kernels need 200 -- hardware reciprocal / rsqrt estimates with one Newton step instead of the IEEE divide
// and sqrt expansions, a fp32 Cody-Waite sincos, no SLP vectorisation (csrc/Makefile) -- and are built for two waves
// per SIMD without scratch: the second wave takes the issue slots a lone wave leaves empty (a lone wave issues one
// VALU instruction every 4 cycles, the SIMD takes an fp32 one every 2), 1.6x from 131 072 envs per GPU on.
#define OS2R_STEP_KERNEL_ATTRS(REAL) \
  __launch_bounds__(os2r::kWave) __attribute__((amdgpu_waves_per_eu(sizeof(REAL) == 4 ? 2 : 1)))

template <typename T, typename MD, bool CONTACT, bool DR, bool STD_SWEEPS, typename LAY = RtLayout, bool COUNT = false,
          int SOLVER = std_solver(STD_SWEEPS, sizeof(T) == 8, StdSolver<T>::kExact), bool ROLLOUT = false>
__global__ OS2R_STEP_KERNEL_ATTRS(T) void step_kernel(const StepArgs<T> A) {
  step_body<T, MD, CONTACT, DR, STD_SWEEPS, LAY, COUNT, SOLVER, ROLLOUT>(A);
}

// os2r_rollout_policy, fused: the rollout variant of step_kernel (default solver compiled in) with the policy in the loop.  Its
// one argument begins with the StepArgs (step_body reads the argument segment at offset 0).
template <typename T, typename MD, bool CONTACT, bool DR, typename LAY>
__global__ OS2R_STEP_KERNEL_ATTRS(T) void policy_rollout_kernel(const PolicyArgs<T> P) {
  step_body<T, MD, CONTACT, DR, true, LAY, false, std_solver(true, sizeof(T) == 8, StdSolver<T>::kExact), true, true>(P.s);
}

// os2rr_rollout_policy_recorded, fused: the same kernel with the sink in its step loop, under a name of its own
template <typename T, typename MD, bool CONTACT, bool DR, typename LAY>
__global__ OS2R_STEP_KERNEL_ATTRS(T) void policy_record_kernel(const PolicyArgs<T> P) {
  step_body<T, MD, CONTACT, DR, true, LAY, false, std_solver(true, sizeof(T) == 8, StdSolver<T>::kExact), true, true, true>(P.s);
}

// os2r_rollout_policy, launch loop (the configurations without a fused variant): per env-step this kernel turns the stored state
// into the observation and the policy's actions ([N][2], P.act), the step launch takes them, policy_accumulate_kernel sums.
template <typename T, int NQ>
__global__ __launch_bounds__(kWave) void policy_kernel(const PolicyArgs<T> P) {
  const StepArgs<T>& A = P.s;
  const int lane = threadIdx.x;
  const long long e0 = (long long)blockIdx.x * kWave;
  const bool valid = e0 + lane < A.N;
  const long long e = valid ? e0 + lane : A.N - 1;
  const TaskPtr<T> ts = as_const(A.task);
  T q[NQ], qd[NQ];
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    q[i] = A.q[i * A.N + e];
    qd[i] = A.qd[i * A.N + e];
  }
  const T h2x = A.hist[2 * A.N + e], h2y = A.hist[3 * A.N + e];
  T obs[OS2R_MAX_OBS];
  bool dn;
  unsigned why;
  observe<T, NQ>(ts, q, qd, h2x, h2y, obs, dn, why);
  if (P.knot_obs) {   // os2rr_rollout_policy_recorded: this env-step's [N][D] slice of the knots' observations
    __shared__ T tile[kWave * OS2R_MAX_OBS];
    store_obs_tile<T>(P.knot_obs, obs, ts->obs_dim, e0, A.N, lane, tile);
  }
  T ax, ay;
  policy_action<T>(&P, A, ts->obs_dim, e, valid, A.step_count, 0, e, obs, ax, ay);
  if (valid) {
    P.act[2 * e] = ax;
    P.act[2 * e + 1] = ay;
  }
}

// step k's reward and done flag into the return and length (launch loop); the same sums as the fused epilogue
template <typename T>
__global__ void policy_accumulate_kernel(T* __restrict__ ret, int32_t* __restrict__ len, uint8_t* __restrict__ open,
                                         const T* __restrict__ rew, const uint8_t* __restrict__ done, long long N, int k,
                                         int first_episode) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N) return;
  const bool summing = k == 0 || open[e] != 0;
  if (summing) {
    if (ret) ret[e] = (k == 0 ? T(0) : ret[e]) + rew[e];
    if (len) len[e] = (k == 0 ? 0 : len[e]) + 1;
  }
  open[e] = (summing && !(first_episode && done[e] != 0)) ? (uint8_t)1 : (uint8_t)0;
}

// ----------------------------------------------------------------------------------------
// masked reset kernel: GazeboEnvRandomizer.reset -> randomize_task -> get_observation
// ----------------------------------------------------------------------------------------
template <typename T, int NQ, bool DR>
__global__ __launch_bounds__(kWave) void reset_kernel(const StepArgs<T> A) {
  __shared__ T tile[kWave * OS2R_MAX_OBS];
  const int lane = threadIdx.x;
  const long long e0 = (long long)blockIdx.x * kWave;
  const bool valid = e0 + lane < A.N;
  const long long e = valid ? e0 + lane : A.N - 1;
  const TaskPtr<T> ts = as_const(A.task);
  T q[NQ], qd[NQ];
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    q[i] = A.q[i * A.N + e];
    qd[i] = A.qd[i * A.N + e];
  }
  using MD = RtModel<T, NQ>;
  ParamVals<T, NQ> pv;
  const bool doit = A.reset_mask ? A.reset_mask[e] != 0 : true;
  uint32_t epi = A.episode[e];
  uint8_t pose = A.pose[e];
  if (doit) {
    reset_env<T, MD, DR>(A, e, epi, q, qd, pv, pose);
    epi += 1;
  }
  const T h1x = A.hist[2 * A.N + e], h1y = A.hist[3 * A.N + e];
  T obs[OS2R_MAX_OBS];
  bool dn;
  unsigned why;
  observe<T, NQ>(ts, q, qd, h1x, h1y, obs, dn, why);
  if (A.obs) store_obs_tile<T>(A.obs, obs, ts->obs_dim, e0, A.N, lane, tile);
  if (valid && doit) {
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      A.q[i * A.N + e] = q[i];
      A.qd[i * A.N + e] = qd[i];
    }
    A.episode[e] = epi;
    A.pose[e] = pose;
    A.steps[e] = 0;
    store_params<T, NQ>(A, e, pv);
    A.solver_flags[e] = 0u;   // a new episode: the contact solver remembers nothing
#pragma unroll
    for (int k = 0; k < 4 * NQ; ++k) A.solver_l[k * A.N + e] = T(0);
  }
}

// per-env gravity drawn once at create (randomizers/monopod.py:56-61)
template <typename T>
__global__ void gravity_kernel(T* __restrict__ gravity, long long N, long long env_offset, unsigned long long seed,
                               double mean, double std_) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N) return;
  double z0, z1;
  normal2(seed, (uint32_t)(env_offset + e), kStreamGravity, 0, 0, z0, z1);
  gravity[e] = (T)(mean + std_ * z0);
}

template <typename T>
__global__ void fill_kernel(T* __restrict__ dst, long long n, T value) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = value;
}

// ----------------------------------------------------------------------------------------
// os2r_copy_envs: environment e of the destination becomes environment index[e] of the source
// ----------------------------------------------------------------------------------------
// Pure memory movement, the opposite corner from the step kernel: no arithmetic, a dozen registers, as many waves per
// SIMD as the hardware holds.  Every array of a handle is SoA [rows][N]; the host lists the selected rows of both handles
// in one flat table (they live in a dozen allocations), and the grid's second dimension walks it kCopyGroup rows at a
// time: a lane issues the loads of its group, then the stores, so a wave has kCopyGroup requests in flight and a small
// batch still fills the machine (256 envs: 4 x 8 waves instead of 4).  Row r is read at src[r][i] and stored at
// dst[r][e]: stores are always coalesced, loads are coalesced for the identity map and one address per wave for a fork.
constexpr int kCopyMaxRows = 10 * OS2R_MAX_DOF + 5;   // q, qd: nq each; history: 4; solver impulses: 4 nq; parameters: 4 nq + 1
constexpr int kCopyGroup = 8;
constexpr int kCopyTable = (kCopyMaxRows + kCopyGroup - 1) / kCopyGroup * kCopyGroup;   // whole groups: a group's addresses are one fetch
template <typename T>
struct CopyArgs {
  const int32_t* index;   // [Nd] or null (identity: Ns == Nd)
  long long Nd, Ns;       // environments of the destination / the source
  int gather;             // 1: lane e reads column index[e]; 0: column e, the index only says which lanes take part
  int nrows;              // rows of the handle's dtype
  int nwords;             // 32-bit rows: solver flags, elapsed steps, episode index
  const T* src[kCopyTable];
  T* dst[kCopyTable];
  const uint32_t* src32[3];
  uint32_t* dst32[3];
  const uint8_t* src8;    // the reset pose id, or null
  uint8_t* dst8;
};

template <typename T>
__global__ __launch_bounds__(kWave) void copy_envs_kernel(const CopyArgs<T> A) {
  const long long e = (long long)blockIdx.x * kWave + threadIdx.x;
  if (e >= A.Nd) return;
  long long i = e;
  if (A.index) {
    const long long ix = A.index[e];
    if (ix < 0 || ix >= A.Ns) return;   // "keep": nothing of this environment is read or written
    if (A.gather) i = ix;
  }
  const int r0 = (int)blockIdx.y * kCopyGroup;
  if (r0 < A.nrows) {
    const T* sp[kCopyGroup];
    T* dp[kCopyGroup];
    T v[kCopyGroup];
#pragma unroll
    for (int k = 0; k < kCopyGroup; ++k) {   // (past nrows the table holds nulls, which are fetched and never used)
      sp[k] = A.src[r0 + k];
      dp[k] = A.dst[r0 + k];
    }
#pragma unroll
    for (int k = 0; k < kCopyGroup; ++k)
      if (r0 + k < A.nrows) v[k] = sp[k][i];
#pragma unroll
    for (int k = 0; k < kCopyGroup; ++k)
      if (r0 + k < A.nrows) dp[k][e] = v[k];
  } else {   // the last group: the integer rows
    uint32_t w[3];
    uint8_t b = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (k < A.nwords) w[k] = A.src32[k][i];
    if (A.src8) b = A.src8[i];
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (k < A.nwords) A.dst32[k][e] = w[k];
    if (A.src8) A.dst8[e] = b;
  }
}

// the observation of every environment's stored state, [N][D]: observe() as reset_kernel and policy_kernel evaluate it
template <typename T, int NQ>
__global__ __launch_bounds__(kWave) void copy_envs_obs_kernel(const StepArgs<T> A) {
  __shared__ T tile[kWave * OS2R_MAX_OBS];
  const int lane = threadIdx.x;
  const long long e0 = (long long)blockIdx.x * kWave;
  const bool valid = e0 + lane < A.N;
  const long long e = valid ? e0 + lane : A.N - 1;
  const TaskPtr<T> ts = as_const(A.task);
  T q[NQ], qd[NQ];
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    q[i] = A.q[i * A.N + e];
    qd[i] = A.qd[i * A.N + e];
  }
  const T h1x = A.hist[2 * A.N + e], h1y = A.hist[3 * A.N + e];
  T obs[OS2R_MAX_OBS];
  bool dn;
  unsigned why;
  observe<T, NQ>(ts, q, qd, h1x, h1y, obs, dn, why);
  store_obs_tile<T>(A.obs, obs, ts->obs_dim, e0, A.N, lane, tile);
}

// ----------------------------------------------------------------------------------------
// os2r_linearize: finite-difference Jacobians of the transition x' = f(x, a) of one env-step
// ----------------------------------------------------------------------------------------
// One wave per (64 environments, column): grid.y walks the requested columns -- the 2 nq state columns of A, the two action
// columns of B, the nominal point of `next` -- so that 64 environments of the 5-dof robot occupy 25 SIMDs, not one.  A wave
// runs the physics of os2r_step (the same loads, bind_params, torques and substep instantiation as step_body) from the
// column's upper point, stores f_hi into the column's output slots, runs it again from the lower point and replaces the slots
// by (f_hi - f_lo) / (hi - lo): the same lane, the same addresses, program order, as the return of the policy epilogue.  Nothing
// of width 2 nq lives across a physics loop, and nothing of the handle is written.
constexpr int kLinMaxCols = 2 * OS2R_MAX_DOF + 3;
// The argument begins with the StepArgs (as PolicyArgs does): bind_params and the loads take them as they are.
template <typename T>
struct LinArgs {
  StepArgs<T> s;             // s.actions: the nominal actions [N][2]; nothing behind the handle's arrays is written
  T eps_q, eps_qd, eps_a;
  T* __restrict__ next;      // [2nq][N] or null
  T* __restrict__ jac_a;     // [2nq][2nq][N] or null
  T* __restrict__ jac_b;     // [2nq][2][N] or null
  int ncols;                 // grid.y
  int col[kLinMaxCols];      // column of wave row y: 0..nq-1 q_j, nq..2nq-1 qd_j, 2nq / 2nq+1 the actions, 2nq+2 the nominal point
};

template <typename T, typename MD, bool CONTACT, bool DR, bool STD_SWEEPS, int SOLVER>
__device__ __forceinline__ void linearize_body(const LinArgs<T>& P) {
  const StepArgs<T>& A = P.s;
  constexpr int NQ = MD::NQ;
  constexpr bool kCandInLds = CONTACT && MD::CMASK != 0u && !MD::kStatic;
  constexpr int kParamWords = DR ? 4 * NQ * kWave : 0;
  __shared__ T tile[lds_words<NQ>() + kParamWords + (kCandInLds ? kCandWords : 0)];
  const int lane = threadIdx.x;
  const long long e0 = (long long)blockIdx.x * kWave;
  const bool valid = e0 + lane < A.N;
  const long long e_lane = valid ? e0 + lane : A.N - 1;  // tail lanes shadow the last env, stores are masked
  const MD md = make_model<T, MD>(A);
  T* cand_lds = tile + lds_words<NQ>() + kParamWords;
  if constexpr (kCandInLds) {
    const int nc3 = 3 * md.cand_begin(NQ);
    for (int k = lane; k < nc3; k += kWave) cand_lds[k] = md.cand(k / 3, k % 3);
    __syncthreads();
  }
  const int col = P.col[blockIdx.y];   // wave-uniform
  const int npass = col == 2 * NQ + 2 ? 1 : 2;
  T sn[NQ], cs[NQ];
  WorkCounts wc;
#ifdef OS2R_STAMPS
  unsigned long long stamps[kStamps] = {}, stamp_prev = 0;   // (the diagnostic build's substep takes them; nothing reads these)
#endif
#pragma nounroll
  for (int pass = 0; pass < npass; ++pass) {
    // (as in a rollout: the environment index is a fresh value in every pass, so that no address is held across the physics loop)
    long long e = e_lane;
    asm volatile("" : "+v"(e));
    T q[NQ], qd[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      q[i] = A.q[i * A.N + e];
      qd[i] = A.qd[i * A.N + e];
    }
    Params<T, MD, DR> par;
    bind_params<T, MD, DR>(A, e, md, par, tile + lds_words<NQ>() + lane);
    constexpr bool kCarry = sizeof(T) == 8 && SOLVER != kSolverSweeps;
    SolverCarry<T, NQ> carry;
    if constexpr (kCarry) {
      carry.act = A.solver_flags[e];
#pragma unroll
      for (int b = 0; b < NQ; ++b) {
        if (CONTACT && ((MD::CMASK >> b) & 1u)) {
          carry.ln[b] = A.solver_l[(0 * NQ + b) * A.N + e];
          carry.lx[b] = A.solver_l[(1 * NQ + b) * A.N + e];
          carry.ly[b] = A.solver_l[(2 * NQ + b) * A.N + e];
        }
        carry.lf[b] = A.solver_l[(3 * NQ + b) * A.N + e];
      }
    }
    T ax = A.actions[2 * e], ay = A.actions[2 * e + 1];
    ax = ax < T(-1) ? T(-1) : (ax > T(1) ? T(1) : ax);   // a query: clamped silently, no violation counted
    ay = ay < T(-1) ? T(-1) : (ay > T(1) ? T(1) : ay);
    // the column's point: x_j + h, then x_j - h (one rounded add each); an action stops at its limit
    if (npass == 2) {
#pragma clang fp contract(off)
      const T sign = pass == 0 ? T(1) : T(-1);
      const T hq = sign * P.eps_q, hv = sign * P.eps_qd, ha = sign * P.eps_a;
#pragma unroll
      for (int i = 0; i < NQ; ++i) {
        q[i] = opaque(col == i ? q[i] + hq : q[i]);
        qd[i] = opaque(col == NQ + i ? qd[i] + hv : qd[i]);
      }
      T px = ax + ha, py = ay + ha;
      px = px < T(-1) ? T(-1) : (px > T(1) ? T(1) : px);
      py = py < T(-1) ? T(-1) : (py > T(1) ? T(1) : py);
      ax = opaque(col == 2 * NQ ? px : ax);
      ay = opaque(col == 2 * NQ + 1 ? py : ay);
    }
    T tau_hip, tau_knee;
    {
#pragma clang fp contract(off)
      tau_hip = md.max_torque(0) * ax;
      tau_knee = md.max_torque(1) * ay;
    }
    for (int s = 0; s < A.substeps; ++s) {
      substep<T, MD, CONTACT, DR, false, SOLVER>(
          md, par, q, qd, sn, cs, s == 0, tau_hip, tau_knee, A.dt, A.erp, A.max_erv, A.margin,
          STD_SWEEPS ? std_iters<T>(NQ) : A.pgs_iters, STD_SWEEPS ? StdSolver<T>::kNormalIters : A.pgs_normal_iters,
          A.pgs_exact, A.pgs_tol, tile, cand_lds, as_const(A.model), wc, carry
#ifdef OS2R_STAMPS
          , stamps, stamp_prev
#endif
      );
    }
    __syncthreads();
    // behind the physics loop: a fresh environment index and the arguments re-read from the argument segment (step_body)
    long long ep = e;
    asm volatile("" : "+v"(ep));
    const OS2R_CONST LinArgs<T>* args_e = (const OS2R_CONST LinArgs<T>*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(args_e));
    const LinArgs<T>& Pe = *(const LinArgs<T>*)args_e;
    const long long N = Pe.s.N;
    // the column's slots: element [i][j] of an [2nq][width][N] array
    T* out = Pe.jac_a;
    int width = 2 * NQ, j = col;
    if (col >= 2 * NQ) { out = Pe.jac_b; width = 2; j = col - 2 * NQ; }
    if (col == 2 * NQ + 2) { out = Pe.next; width = 1; j = 0; }
    if (valid) {
#pragma clang fp contract(off)
      if (pass == 0) {   // f_hi waits in the output slots; the nominal point is the output
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
          out[(long long)(i * width + j) * N + ep] = q[i];
          out[(long long)((NQ + i) * width + j) * N + ep] = qd[i];
        }
      } else {
        // hi - lo of the column, from the stored value again: the same two rounded adds
        T hi, lo;
        if (col < 2 * NQ) {
          const T x = col < NQ ? Pe.s.q[(long long)col * N + ep] : Pe.s.qd[(long long)(col - NQ) * N + ep];
          const T h = col < NQ ? Pe.eps_q : Pe.eps_qd;
          hi = x + h;
          lo = x - h;
        } else {
          T a = Pe.s.actions[2 * ep + j];
          a = a < T(-1) ? T(-1) : (a > T(1) ? T(1) : a);
          hi = a + Pe.eps_a;
          hi = hi > T(1) ? T(1) : hi;
          lo = a - Pe.eps_a;
          lo = lo < T(-1) ? T(-1) : lo;
        }
        const T den = opaque(hi) - opaque(lo);
        // one rounded subtraction, one IEEE division: none of the reciprocal estimates of the physics code
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
          const long long at_q = (long long)(i * width + j) * N + ep, at_v = (long long)((NQ + i) * width + j) * N + ep;
          const T fq = out[at_q], fv = out[at_v];
          out[at_q] = (fq - opaque(q[i])) / den;
          out[at_v] = (fv - opaque(qd[i])) / den;
        }
      }
    }
    // the second pass reads what this one stored: vector memory operations of a wave are performed in order
    asm volatile("" ::: "memory");
  }
}

template <typename T, typename MD, bool CONTACT, bool DR, bool STD_SWEEPS, int SOLVER>
__global__ OS2R_STEP_KERNEL_ATTRS(T) void linearize_kernel(const LinArgs<T> P) {
  linearize_body<T, MD, CONTACT, DR, STD_SWEEPS, SOLVER>(P);
}

// launch tables (defined in the per-dtype instantiation units)
template <typename T>
struct Launcher {
  // model_id: index of the matching constexpr table (os2r_models_gen.hpp) or -1 for the run-time model
  static int step(int nq, int model_id, bool contact, bool dr, const StepArgs<T>& args, hipStream_t stream);
  static int reset(int nq, bool dr, const StepArgs<T>& args, hipStream_t stream);
  static void gravity(T* g, long long N, long long off, unsigned long long seed, double mean, double std_, hipStream_t s);
  static void fill(T* dst, long long n, T value, hipStream_t s);
  // os2r_rollout_policy: the fused kernel (2: none for this configuration), the policy kernel of the launch loop, the sums
  static int policy_rollout(int model_id, bool contact, bool dr, const PolicyArgs<T>& args, hipStream_t stream);
  static int policy(int nq, const PolicyArgs<T>& args, hipStream_t stream);
  static void accumulate(T* ret, int32_t* len, uint8_t* open, const T* rew, const uint8_t* done, long long N, int k,
                         int first_episode, hipStream_t s);
  // os2r_copy_envs: the copy itself, and the observation of the stored state into args.obs
  static void copy_envs(const CopyArgs<T>& args, hipStream_t s);
  static int copy_obs(int nq, const StepArgs<T>& args, hipStream_t s);
  // os2r_linearize: the variant whose substep instantiation is the one Launcher::step runs for this handle
  static int linearize(int nq, int model_id, bool contact, bool dr, const LinArgs<T>& args, hipStream_t s);
};

}  // namespace os2r
