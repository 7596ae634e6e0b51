/*
 * os2r.h — C-ABI of the MI355X-native batched monopod stepper.
 *
 * This is the drop-in boundary for the gym_os2r "env.step" hot path.  The
 * reference reaches its physics backend through these Python->SWIG call sites
 * (all paths relative to the reference checkout):
 *
 *   gym_os2r/runtimes/gazebo_runtime.py:70-77   10x { task.set_action(a); gazebo.run() }
 *   gym_os2r/runtimes/gazebo_runtime.py:80-95   get_observation / get_reward / is_done / get_info
 *   gym_os2r/runtimes/gazebo_runtime.py:111-114 scenario.GazeboSimulator(1/physics_rate, rtf, steps_per_run=1)
 *   gym_os2r/tasks/monopod.py:225,234           model.set_joint_generalized_force_targets / ..._targets()
 *   gym_os2r/tasks/monopod.py:248-249           model.joint_positions / joint_velocities
 *   gym_os2r/randomizers/monopod.py:125-128     model.to_gazebo().reset_joint_positions / _velocities
 *   gym_os2r/randomizers/monopod.py:60          world.to_gazebo().set_gravity
 *   gym_os2r/randomizers/monopod.py:182-215     per-reset SDF randomisation (mass/friction/damping/mu)
 *
 * One Os2rSim owns the state of N independent environments resident in HBM
 * (struct-of-arrays, one GPU lane per environment).  Every entry point returns
 * an int status (0 = OK), never throws, and is stream-ordered on the hipStream_t
 * passed as `void* stream` (NULL = the default stream).  All `*_dev` pointers
 * are device pointers owned by the caller (e.g. torch tensors' data_ptr()); the
 * library owns only its internal state.  A handle is not thread-safe.
 *
 * Plain C: no torch / pybind / HIP types appear in any signature.
 */
#ifndef OS2R_H_
#define OS2R_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the entry points declared here are its whole dynamic symbol table. */
#if defined(__GNUC__) || defined(__clang__)
#define OS2R_API __attribute__((visibility("default")))
#else
#define OS2R_API
#endif

#define OS2R_ABI_VERSION 6   /* os2r_create also takes configs stamped 5 (Os2rConfig did not change in 6) */
#define OS2R_ABI_MINOR 1     /* entry points added within ABI 6 (os2r_abi_minor): 1: os2r_rollout_policy_noisy */
/* os2r_copy_envs and, after it, os2r_linearize, os2r_rollout_policy_scheduled and os2r_lqr_gains were added later without a new
 * minor: a binding finds out whether they are there by looking the symbol up */

#define OS2R_MAX_DOF 5      /* yaw, pitch, boom_connector, hip, knee                       */
#define OS2R_MAX_CAND 192   /* ground-contact candidate points of one model                */
#define OS2R_MAX_OBS 12     /* 5 pos + 5 vel + 2 measured torques                          */
#define OS2R_MAX_RESET_POSES 8

/* status codes */
enum {
  OS2R_OK = 0,
  OS2R_ERR_INVALID = 1,   /* bad argument / inconsistent config                            */
  OS2R_ERR_HIP = 2,       /* a HIP runtime call failed, see os2r_last_error                 */
  OS2R_ERR_NO_DEVICE = 3, /* no gfx950 device visible                                       */
  OS2R_ERR_ALLOC = 4
};

/* arithmetic type of the device path */
enum { OS2R_F32 = 0, OS2R_F64 = 1 };

/* ------------------------------------------------------------------------- *
 * Compiled robot model: a serial chain of nq revolute joints hanging off the
 * world, produced by the model compiler from a URDF (+ STL collision meshes)
 * with fixed joints lumped into their parent body
 * (gym_os2r/models/models/<variant>/<variant>.urdf).
 * Joint i connects body i-1 (body -1 = world) to body i.
 * ------------------------------------------------------------------------- */
typedef struct Os2rModel {
  int32_t nq;                          /* 2..5 degrees of freedom                            */
  int32_t axis[OS2R_MAX_DOF];          /* joint axis in the joint frame: 0=x 1=y 2=z         */
  double rfix[OS2R_MAX_DOF][9];        /* row-major rotation: joint frame in parent body     */
  double rpos[OS2R_MAX_DOF][3];        /* joint origin in parent body frame [m]              */
  double mass[OS2R_MAX_DOF];           /* (lumped) body mass [kg]                            */
  double com[OS2R_MAX_DOF][3];         /* centre of mass in body frame [m]                   */
  double icom[OS2R_MAX_DOF][6];        /* inertia about COM, body axes: xx xy xz yy yz zz    */
  double damping[OS2R_MAX_DOF];        /* viscous joint damping [N m s/rad]                  */
  double friction[OS2R_MAX_DOF];       /* Coulomb joint friction [N m]                       */
  double mu[OS2R_MAX_DOF];             /* contact friction coefficient of body i vs ground   */
  int32_t act_dof[2];                  /* dof index of hip_joint, knee_joint                 */
  double max_torque[2];                /* [N m], settings.yaml spaces/action                 */
  double gravity_z;                    /* world gravity along z [m/s^2] (negative)           */
  int32_t ncand;                       /* number of contact candidate points                 */
  int32_t cand_body[OS2R_MAX_CAND];    /* body index of each candidate, non-decreasing       */
  double cand_p[OS2R_MAX_CAND][3];     /* candidate position in its body frame [m]           */
  double cand_center[OS2R_MAX_DOF][3]; /* bounding sphere of body i's candidates (body frame) */
  double cand_radius[OS2R_MAX_DOF];    /*   used to skip the scan of a body far from the ground */
} Os2rModel;

/* observation slot kinds (gym_os2r/tasks/monopod.py:238-272, monopod_no_norm.py:222-246) */
enum {
  OS2R_OBS_POS_NORM = 0,       /* 2*(x-low)/(high-low)-1                                   */
  OS2R_OBS_POS_PERIODIC_NORM,  /* wrap to [-pi,pi) then the affine map                     */
  OS2R_OBS_VEL_TANH,           /* tanh(0.05*v)                                              */
  OS2R_OBS_TORQUE_NORM,        /* previous action through the affine map (low=-1, high=1)  */
  OS2R_OBS_POS_RAW,            /* no_norm task: x                                           */
  OS2R_OBS_POS_PERIODIC_RAW,   /* no_norm task: wrap only                                   */
  OS2R_OBS_VEL_RAW,            /* no_norm task: v                                           */
  OS2R_OBS_TORQUE_RAW          /* no_norm task: previous action                             */
};

/* reward ids (gym_os2r/rewards/__init__.py) */
enum {
  OS2R_REWARD_BALANCING_V1 = 0, /* :66-81  (StandingV1 :135-149 is the same formula)        */
  OS2R_REWARD_BALANCING_V2 = 1, /* :83-101                                                   */
  OS2R_REWARD_BALANCING_V3 = 2, /* :103-131                                                  */
  OS2R_REWARD_STANDING_V1 = 3,
  OS2R_REWARD_HOPPING_V1 = 4,   /* :151-180                                                  */
  OS2R_REWARD_STRAIGHT_V1 = 5   /* :183-207                                                  */
};

/* reset modes */
enum {
  OS2R_RESET_FIXED = 0,   /* MonopodEnvNoRandomizer (randomizers/monopod_no_rand.py:59-98)  */
  OS2R_RESET_RANDOM = 1   /* MonopodEnvRandomizer   (randomizers/monopod.py:89-128,182-215) */
};

typedef struct Os2rTaskSpec {
  int32_t obs_dim;
  int32_t obs_kind[OS2R_MAX_OBS];
  int32_t obs_src[OS2R_MAX_OBS];   /* dof index (pos/vel kinds) or action index (torque)    */
  double obs_low[OS2R_MAX_OBS];    /* normalisation limits (periodic: -(pi+eps))            */
  double obs_high[OS2R_MAX_OBS];
  double done_lo[OS2R_MAX_OBS];    /* done iff !(done_lo <= y <= done_hi), y = value before */
  double done_hi[OS2R_MAX_OBS];    /*   the affine/tanh map (after the periodic wrap)       */
  int32_t reward_id;
  int32_t normalized;              /* 1: MonopodTask, 0: monopod_no_norm.MonopodTask        */
  int32_t idx_pitch_pos;           /* obs indices the rewards read; -1 if masked/absent     */
  int32_t idx_yaw_vel;
  int32_t idx_hip_pos;
  int32_t idx_knee_pos;
  int32_t max_episode_steps;       /* gym TimeLimit (gym_os2r/__init__.py:19,56); 0 = none  */
  /* reset */
  int32_t reset_mode;
  int32_t n_reset_poses;
  int32_t reset_pose_id[OS2R_MAX_RESET_POSES];   /* index into the settings 'resets' table  */
  int32_t reset_laying[OS2R_MAX_RESET_POSES];
  double reset_pitch[OS2R_MAX_RESET_POSES];
  double reset_hip[OS2R_MAX_RESET_POSES];        /* precomputed IK (utils/reset.py) or 1.57 */
  double reset_knee[OS2R_MAX_RESET_POSES];
  int32_t reset_simple;            /* 1: task_mode 'simple' (hip,knee ~ U(-1,1), quirk)     */
  double leg_def[6];               /* ul, ll, cph, lb, hip_offset, clipping_adjust [mm]     */
  int32_t dof_yaw, dof_pitch, dof_bc, dof_hip, dof_knee; /* chain dof index or -1           */
  /* domain randomisation (randomizers/monopod.py:56-61,182-215); used when reset_mode==1  */
  int32_t randomize_params;        /* 1: resample mass/friction/damping/mu at every reset   */
  double dr_mass_lo, dr_mass_hi;          /* coefficient, U(0.8,1.2)                        */
  double dr_friction_lo, dr_friction_hi;  /* absolute,    U(0.01,0.05)                      */
  double dr_damping_lo, dr_damping_hi;    /* coefficient, U(0.8,1.2), zeros ignored         */
  double dr_mu_base, dr_mu_lo, dr_mu_hi;  /* 0.33 * U(0.8,1.2)                              */
  double dr_gravity_mean, dr_gravity_std; /* N(-9.8,0.2), drawn once at create              */
  int32_t gravity_rollouts;        /* > 0: gravity is drawn anew for an environment after every    */
                                   /*   this many of its rollouts (the reference re-creates the    */
                                   /*   simulator then: randomizers/monopod.py:36-41,56-61,371);   */
                                   /*   0: once at create                                          */
  int32_t reserved_;
} Os2rTaskSpec;

typedef struct Os2rConfig {
  int32_t abi_version;     /* OS2R_ABI_VERSION (5 is accepted too: same struct)               */
  int32_t dtype;           /* OS2R_F32 / OS2R_F64.  F32: done and every done-reason bit equal  */
                           /*   what the reference decides in f64 on the f32 state (the done   */
                           /*   bounds are rounded inward to float); observations and rewards  */
                           /*   are only close: a normalised observation may read -/+1.0f      */
                           /*   while the environment is inside the reset space.               */
  int64_t num_envs;        /* environments owned by this handle (this rank's shard)          */
  int64_t env_offset;      /* global index of local env 0 (multi-GPU sharding; RNG key)      */
  uint64_t seed;
  int32_t device;          /* HIP device ordinal                                             */
  int32_t substeps;        /* physics_rate/agent_rate = 10 (runtimes/gazebo_runtime.py:46)   */
  double dt;               /* 1/physics_rate = 1e-4 s                                        */
  int32_t contact;         /* 0: ground contact off (bring-up config C2), 1: on              */
  int32_t pgs_iters;       /* upper bound on the projected Gauss-Seidel sweeps per substep   */
                           /*   over all rows (phase 2)                                      */
  int32_t pgs_normal_iters;/* preceding sweeps over normal + joint-friction rows that fix    */
                           /*   the tangential bounds (0: coupled pyramid)    */
  int32_t auto_reset;      /* SubprocVecEnv semantics (common/vec_env/subproc_vec_env.py:15) */
  double erp;              /* contact error-reduction parameter (finite; 0: none)            */
  double max_erv;          /* cap on the error-reduction velocity [m/s] (finite, >= 0)       */
  double contact_margin;   /* candidates closer than this to the ground join the contact [m] */
  double pgs_tol;          /* an environment stops sweeping once a checked sweep moved no more     */
                           /*   energy than this [J]; 0: exact fixed points only                   */
  int32_t pgs_exact;       /* exact finish of the boxed LCP: an environment that   */
                           /*   has not converged after the first three sweeps of phase 2 (which    */
                           /*   starts from the impulses of the environment's previous iteration,   */
                           /*   os2r_get_solver_state) solves its                                   */
                           /*   free rows exactly (a 5x5 system in the whitened velocities), with  */
                           /*   active-set pivots (a step cut at a bound; an inconsistent free set */
                           /*   left by a step to the first bound), at most this many solves per   */
                           /*   substep; a checked sweep follows each unblocked solve.             */
                           /*   0: sweeps only, checked every                                      */
                           /*   4th (the round-1/2 solver).  Ignored with pgs_normal_iters == 0;   */
                           /*   needs dtype OS2R_F64.                                              */
  int32_t reserved0_;
  Os2rModel model;
  Os2rTaskSpec task;
} Os2rConfig;

/* per-environment parameter arrays, SoA [count][num_envs] in the handle's dtype */
enum {
  OS2R_PARAM_MASS_SCALE = 0, /* [nq]  body mass coefficient                                 */
  OS2R_PARAM_DAMPING = 1,    /* [nq]  absolute damping                                       */
  OS2R_PARAM_FRICTION = 2,   /* [nq]  absolute Coulomb friction                              */
  OS2R_PARAM_MU = 3,         /* [nq]  body-vs-ground friction coefficient                    */
  OS2R_PARAM_GRAVITY = 4     /* [1]   gravity_z                                              */
};

typedef struct Os2rSim Os2rSim;

OS2R_API int os2r_abi_version(void);
OS2R_API int os2r_abi_minor(void);   /* OS2R_ABI_MINOR of the built library: a binding asks it whether an entry point is there */

/* Allocates device state for cfg->num_envs environments, initialises per-env
 * parameters to the model's nominal values (gravity: N(mean,std) per env when
 * task.reset_mode==OS2R_RESET_RANDOM) and performs a full reset. */
OS2R_API int os2r_create(const Os2rConfig* cfg, Os2rSim** out);
OS2R_API int os2r_destroy(Os2rSim* sim);

/* Reset the environments whose mask byte is non-zero (mask_dev == NULL: all).
 * Replaces GazeboEnvRandomizer.reset -> randomize_task -> task.reset_task.
 * obs_dev (nullable) receives the [num_envs, obs_dim] observation of every env. */
OS2R_API int os2r_reset(Os2rSim* sim, const uint8_t* mask_dev, void* obs_dev, void* stream);

/* One env-step for every environment: `substeps` physics iterations with the
 * action held, then observation, reward, done; done environments are reset in
 * the same launch when auto_reset is set.  Replaces GazeboRuntime.step.
 *   actions_dev  [num_envs,2] in the handle's dtype, values in [-1,1]
 *                (NULL: draw U(-1,1) actions on device from the counter RNG)
 *   obs_dev      [num_envs,obs_dim]   observation (post-reset if auto-reset)
 *   reward_dev   [num_envs]
 *   done_dev     [num_envs] uint8     bit0 done, bit1 TimeLimit truncation,
 *                                     bit2 non-finite state guard
 *   term_obs_dev [num_envs,obs_dim]   nullable; observation before auto-reset
 *                                     (info['terminal_observation'])            */
OS2R_API int os2r_step(Os2rSim* sim, const void* actions_dev, void* obs_dev, void* reward_dev,
              uint8_t* done_dev, void* term_obs_dev, void* stream);

/* `nsteps` env-steps of every environment, as `nsteps` calls of os2r_step would make them -- bit for bit -- but without a
 * device-wide barrier between the env-steps: where a fused variant of the step kernel exists (the compiled-in robots
 * with ground contact, the default solver settings and a reference task layout) the whole rollout is ONE launch in which
 * every wave advances its own 64 environments step after step, state in registers; otherwise the library makes the
 * `nsteps` launches itself.  For open-loop action sequences and random rollouts (the reference's workers advance
 * independently of each other: gym_os2r/common/vec_env/subproc_vec_env.py:15-21); a linear policy in the loop runs the same way
 * through os2r_rollout_policy (below).
 *   actions_dev  [nsteps][num_envs][2] or NULL (on-device U(-1,1) actions, step counter as in os2r_step)
 *   obs_dev      [nsteps][num_envs][obs_dim], reward_dev [nsteps][num_envs], done_dev [nsteps][num_envs] uint8,
 *   term_obs_dev [nsteps][num_envs][obs_dim] (nullable), reason_dev [nsteps][num_envs] uint16 (nullable; the done
 *                reasons of os2r_set_done_reasons per step -- the buffer set there is not written by a rollout)  */
OS2R_API int os2r_rollout(Os2rSim* sim, int nsteps, const void* actions_dev, void* obs_dev, void* reward_dev,
                          uint8_t* done_dev, void* term_obs_dev, uint16_t* reason_dev, void* stream);

/* Closed-loop rollouts with an on-device linear policy (ABI 6): `nsteps` env-steps of every environment in which the action of
 * each env-step is a = squash(W.o + b), evaluated on the environment's own observation o -- the one its previous env-step (or
 * reset) returned, post-reset after an auto-reset; it is recomputed from the stored state at the top of each env-step.  The
 * handle advances exactly as `nsteps` calls of os2r_step(actions = policy(o)) would advance it, bit for bit: state, contact
 * solver state, action history, episode counters, resets and TimeLimit truncations, step counter += nsteps.  Policy actions lie
 * in [-1, 1]: they are never counted as violations.  The handle's done-reason and done-mask buffers are not written.  Fused
 * into one launch where os2r_rollout has a fused variant; otherwise the library runs a policy launch, the step launch and an
 * accumulation launch per env-step (same results).
 *   weights_dev  handle's dtype; row j (0 = hip, 1 = knee) holds W_j0 ... W_j,D-1, b_j (D = obs_dim):
 *                [2][D+1] shared by all environments, or [2][D+1][num_envs] (env index fastest) with OS2R_POLICY_PER_ENV
 *   flags        OS2R_POLICY_* bits
 *                z_j = (((b_j + W_j0*o_0) + W_j1*o_1) + ...), every product rounded on its own (no fused multiply-add): a plain
 *                loop of tensor operations reproduces the action bit for bit; a_j = min(max(z_j, -1), 1), or tanh(z_j)
 *   return_dev   [num_envs] handle's dtype (nullable), overwritten: the rewards summed in step order, (r_0 + r_1) + ...
 *   length_dev   [num_envs] int32 (nullable): the number of env-steps summed.  Without OS2R_POLICY_FIRST_EPISODE both cover
 *                all `nsteps`; with it the sums stop after the first env-step whose done byte is non-zero (that step included)
 *                -- the environment itself keeps stepping and resetting
 *   obs_dev, reward_dev, done_dev, term_obs_dev, reason_dev: the [nsteps][num_envs]... outputs of os2r_rollout, every one
 *                nullable here: a pure evaluation writes nothing per step but the state
 * Errors: OS2R_ERR_INVALID for nsteps < 1, a null weights_dev or an unknown flag bit (os2r_last_error says which).          */
#define OS2R_POLICY_PER_ENV 1       /* weights [2][D+1][N], env index fastest; else one set [2][D+1] for all envs */
#define OS2R_POLICY_TANH 2          /* a_j = tanh(z_j); else a_j = min(max(z_j, -1), 1)                      */
#define OS2R_POLICY_FIRST_EPISODE 4 /* return/length stop after the env's first done flag in the window      */
OS2R_API int os2r_rollout_policy(Os2rSim* sim, int nsteps, const void* weights_dev, int32_t flags,
                                 void* return_dev, int32_t* length_dev,
                                 void* obs_dev, void* reward_dev, uint8_t* done_dev, void* term_obs_dev,
                                 uint16_t* reason_dev, void* stream);

/* The same rollout with Gaussian exploration noise on the policy's pre-squash output (ABI 6, minor 1).  In env-step k of the
 * window, with c = step counter + k (os2r_get_step_count before the call) and e the environment's local index:
 *   (u0, u1) = the two 53-bit uniforms of the Philox4x32-10 block with counter {env_offset + e, 5, c0, c1} and key = seed, where
 *              c0 = low 32 bits of c and c1 = (c >> 32) ^ salt: random stream 5, one block per environment and env-step
 *   eps_0    = sqrt(-2 log(1 - u0)) * cos(2 pi u1), eps_1 = sqrt(-2 log(1 - u0)) * sin(2 pi u1), evaluated in double and
 *              rounded once to the handle's dtype: an f32 handle draws the f64 handle's noise, rounded
 *   y_j      = z_j + (sigma_j * eps_j), z_j as above; the product is rounded on its own, then one add
 *   a_j      = min(max(y_j, -1), 1), or tanh(y_j): noisy actions are squashed, so they are never counted as violations
 * The noise is a pure function of (seed, global environment index, step counter, salt): shards of one batch, a restored
 * checkpoint and windows split differently draw the same noise; another salt draws independent noise at the same step
 * counter (two evaluations from one checkpoint).  sigma_j = 0 gives the deterministic action.  The handle advances exactly
 * as `nsteps` calls of os2r_step(actions = a) would: os2r_rollout on the reported actions replays the window bit for bit.
 *   sigma_dev   handle's dtype: [2] (hip, knee) shared by all environments, or [2][num_envs] (env index fastest) with
 *               OS2R_POLICY_SIGMA_PER_ENV
 *   salt        any 32-bit value; the same salt reproduces the same noise
 *   action_dev  [nsteps][num_envs][2] handle's dtype (nullable): the applied action a
 *   noise_dev   [nsteps][num_envs][2] handle's dtype (nullable): eps
 * Everything else as os2r_rollout_policy, which itself refuses OS2R_POLICY_SIGMA_PER_ENV.
 * Errors: OS2R_ERR_INVALID for nsteps < 1, a null weights_dev or sigma_dev, or an unknown flag bit.                             */
#define OS2R_POLICY_SIGMA_PER_ENV 8 /* sigma [2][N], env index fastest; else one pair [2] for all envs (noisy entry point only) */
OS2R_API int os2r_rollout_policy_noisy(Os2rSim* sim, int nsteps, const void* weights_dev, int32_t flags,
                                       const void* sigma_dev, uint32_t salt,
                                       void* return_dev, int32_t* length_dev,
                                       void* obs_dev, void* reward_dev, uint8_t* done_dev, void* term_obs_dev,
                                       uint16_t* reason_dev, void* action_dev, void* noise_dev, void* stream);

/* The same rollout with a time-scheduled linear policy (added within ABI 6 without a new minor: look the symbol up): the weights
 * are a table of `period` sets, and in each env-step every environment evaluates the set of its slot.  For time-varying gains:
 * TVLQR tracking of a recorded trajectory, the forward pass of iLQR, a periodic feed-forward-plus-feedback gait.
 *   weights_dev  [period][2][D+1] shared by all environments, or [period][2][D+1][num_envs] (env index fastest) with
 *                OS2R_POLICY_PER_ENV; row layout, evaluation order and squash of one set exactly as in os2r_rollout_policy
 *   clock        in env-step k of the call (k = 0 .. nsteps-1) environment e takes t = first_slot + k, or, with
 *                OS2R_POLICY_CLOCK_EPISODE, t = first_slot + steps[e]: the environment's elapsed episode steps as
 *                os2r_get_episode_info would report them at the top of that env-step -- 0 in the first env-step after a reset or an
 *                auto-reset (a negative count set through os2r_set_episode_info is taken as 0)
 *   slot         s = min(t, period-1): the last set is held; or s = t mod period with OS2R_POLICY_SCHEDULE_WRAP
 *                On the window clock one window of K env-steps equals two of K1 and K2 = K - K1 env-steps, the second with
 *                first_slot + K1, bit for bit.
 *   sigma_dev    nullable: NULL is the deterministic policy (salt must then be 0, noise_dev NULL); otherwise the noise is that of
 *                os2r_rollout_policy_noisy, bit for bit: same stream, same counter, same flags (OS2R_POLICY_SIGMA_PER_ENV)
 *   action_dev   [nsteps][num_envs][2] (nullable): the applied actions, with and without sigma: os2r_rollout on them replays the
 *                window bit for bit
 *   noise_dev    [nsteps][num_envs][2] (nullable; needs sigma_dev)
 * Everything else -- returns, lengths, OS2R_POLICY_FIRST_EPISODE, the per-step outputs, step counter += nsteps, no violation
 * counting, the handle's done-reason and done-mask buffers not written, one fused launch or the launch loop -- as
 * os2r_rollout_policy.  period = 1 is os2r_rollout_policy (_noisy) itself.  Both of those refuse the two flag bits below.
 * Errors: OS2R_ERR_INVALID for nsteps < 1, period < 1, first_slot < 0, a null weights_dev, an unknown flag bit, noise_dev without
 * sigma_dev, a non-zero salt without sigma_dev (os2r_last_error says which).                                                    */
#define OS2R_POLICY_CLOCK_EPISODE 16 /* slot from the environment's elapsed episode steps, not the window's step index */
#define OS2R_POLICY_SCHEDULE_WRAP 32 /* slot = t mod period; else t is held at period-1 */
OS2R_API int os2r_rollout_policy_scheduled(Os2rSim* sim, int nsteps, const void* weights_dev, int32_t period,
                                           int32_t first_slot, int32_t flags, const void* sigma_dev, uint32_t salt,
                                           void* return_dev, int32_t* length_dev,
                                           void* obs_dev, void* reward_dev, uint8_t* done_dev, void* term_obs_dev,
                                           uint16_t* reason_dev, void* action_dev, void* noise_dev, void* stream);

/* Model-specialised kernels.  A robot that is not one of the four compiled-in reference variants
 * runs on generic kernels that read its constants through scalar loads (about half the speed).
 * A host binding may instead compile the step kernels for that robot -- gym_os2r_amd/jit.py does:
 * it writes the robot's constants as a constexpr table and runs `hipcc --genco` on
 * gym-os2r_amd/csrc/os2r_jit_unit.hip -- and register the code object here.  os2r_create then
 * uses it for every handle on `device` whose dtype matches and whose Os2rModel equals `model`
 * bit for bit (gravity_z excluded: it is a per-handle value).  Variants the code object does not
 * export (os2r_jit_step_c{0,1}_d{0,1}: contact off/on, per-env parameters off/on) fall back to the
 * generic kernels.  A code object may also export os2r_jit_step_c1_d{0,1}_l together with the data
 * symbol os2r_jit_layout = {kinds, sources, slots} (4 bits per observation slot): the contact
 * kernels with that observation layout folded in; handles whose task has exactly that layout use
 * them, and of several code objects of one robot the one built for the handle's layout is taken.
 * Further optional kernels, each in the step object or (as jit.py builds them, from
 * gym-os2r_amd/csrc/os2r_jit_fused_unit.hip) in a code object of its own registered by a call of
 * its own; a handle takes them only beside step kernels of the same robot:
 *   os2r_jit_rollout_c1_d{0,1}       os2r_rollout in one launch (argument: the step kernels')
 *   os2r_jit_policy_c1_d{0,1}        the three os2r_rollout_policy entry points in one launch
 *   os2r_jit_lin_c{0,1}_d{0,1}[_s]   os2r_linearize on the robot's own arithmetic; _s beside the
 *                                    step kernels' _s (default sweep counts compiled in)
 * The first two serve handles with ground contact, the default solver settings and no work
 * counters -- where the compiled-in robots have a fused variant; every other handle keeps its
 * launch loop.  If their object carries os2r_jit_layout they have that layout folded in and
 * serve handles of that layout only; without the symbol they serve any layout.  A policy object
 * may also export os2r_jit_policy_rec_c1_d{0,1}, the policy kernels that read the sink of
 * os2rr_rollout_policy_recorded of include/os2r_record.h (the fields appended to their argument), together with the data
 * symbol os2r_jit_policy_knots that announces them; on a handle whose policy object lacks the
 * symbol or the kernels -- hand-built, or built before the sink existed: its kernels would take
 * the arguments and record nothing -- a recorded call takes the launch loop.  An object is
 * accepted if it exports at least one kernel named in this comment.  A handle keeps what was
 * registered when it was created.
 * Errors: os2r_last_error(NULL).                                                            */
OS2R_API int os2r_model_is_compiled_in(const Os2rModel* model);
OS2R_API int os2r_register_model_kernels(const Os2rModel* model, int32_t dtype, int32_t device,
                                const char* code_object_path);

/* Caller-provided actions outside [-1, 1]: the reference asserts on them in Python
 * (tasks/monopod.py:222, runtimes/gazebo_runtime.py:67-68) and its backend clamps the torque
 * (tasks/monopod.py:313-316).  The kernel clamps and counts them; this copies the running count
 * of offending environments to dst (device or pinned host memory, ordered on the stream, so a
 * host binding can look at it one call later without stalling) and clears it if `clear`.   */
OS2R_API int os2r_get_action_violations(Os2rSim* sim, uint32_t* dst, int32_t clear, void* stream);
/* The same count without a copy on the step path (ABI 5): *host_words points at two 32-bit words of pinned host memory owned by
 * the handle.  The first wave of every os2r_step / os2r_rollout launch stores there [0] the running count as EARLIER launches left
 * it (what os2r_get_action_violations would copy before this launch; never cleared by this path) and [1] the low 32 bits of the
 * launch's step counter (os2r_get_step_count before the call), so a host binding reads the verdict on step k once [1] > k --
 * a plain load, no event, no memcpy between the launches (a 4-byte copy plus an event per step cost a 65 536-env gym-level
 * loop 8 % of its rate: profiles/r05_host_surface.txt).  Valid until os2r_destroy.                                          */
OS2R_API int os2r_get_violation_mirror(Os2rSim* sim, const volatile uint32_t** host_words);

/* State access in chain dof order, SoA [nq][num_envs], handle's dtype.  os2r_set_state also clears the contact
 * solver's state (below): a state set from outside starts like a reset.                                     */
OS2R_API int os2r_get_state(Os2rSim* sim, void* q_dev, void* qd_dev, void* stream);
OS2R_API int os2r_set_state(Os2rSim* sim, const void* q_dev, const void* qd_dev, void* stream);

/* The contact solver's state (fp64 handles with the exact finish; carried but unused otherwise).  The reference's
 * backend keeps one persistent constraint solver per world (behind gym_os2r/runtimes/gazebo_runtime.py:76,111-114);
 * here every environment remembers the impulses that ended its last physics iteration, and the next one -- of the same
 * env-step or of the next -- starts its contact solve from them.  A reset clears it.
 *   lambda_dev [4*nq][num_envs], handle's dtype: rows b, nq + b, 2nq + b: normal and the two tangential (world x, y)
 *              impulses of body b's ground contact; row 3nq + j: Coulomb friction impulse of joint j
 *   flags_dev  [num_envs] uint32: bit b: body b had a contact (its three impulses are remembered); bit 31: an iteration
 *              has run since the reset (the joint impulses are remembered)
 * Part of a checkpoint: restore it after os2r_set_state.  get: either pointer may be NULL.                        */
OS2R_API int os2r_get_solver_state(Os2rSim* sim, void* lambda_dev, uint32_t* flags_dev, void* stream);
OS2R_API int os2r_set_solver_state(Os2rSim* sim, const void* lambda_dev, const uint32_t* flags_dev, void* stream);

/* Action history: [2][num_envs] SoA; which=0 last applied action, 1 the one before
 * (tasks/monopod.py:95-98,232-235).                                              */
OS2R_API int os2r_get_action_history(Os2rSim* sim, int which, void* out_dev, void* stream);
OS2R_API int os2r_set_action_history(Os2rSim* sim, int which, const void* in_dev, void* stream);

/* Per-env parameter arrays (domain randomisation), SoA [count][num_envs]. */
OS2R_API int os2r_set_params(Os2rSim* sim, int field, const void* src_dev, void* stream);
OS2R_API int os2r_get_params(Os2rSim* sim, int field, void* dst_dev, void* stream);

/* Episode bookkeeping: elapsed steps (int32), episode index (uint32), reset pose
 * id (uint8, info['reset_orientation']); any pointer may be NULL.               */
OS2R_API int os2r_get_episode_info(Os2rSim* sim, int32_t* steps_dev, uint32_t* episode_dev,
                          uint8_t* pose_dev, void* stream);
/* The inverse (any pointer may be NULL): together with os2r_set_state, os2r_set_action_history, os2r_set_params
 * and os2r_set_step_count it restores a handle exactly -- a checkpoint resumed on another handle continues bit
 * for bit (the reference has no save/restore, only env.seed).                                              */
OS2R_API int os2r_set_episode_info(Os2rSim* sim, const int32_t* steps_dev, const uint32_t* episode_dev,
                          const uint8_t* pose_dev, void* stream);

/* Copy whole environments between two handles, or within one, in one launch (fork, resample, broadcast, permute).
 * For every environment e of `dst`, with i = index_dev[e]: if 0 <= i < num_envs of `src`, the arrays selected by `what` of
 * dst[e] become those of src[i], bit for bit; any other i leaves dst[e] untouched (a negative index is the documented
 * "keep"; an index past the source is never dereferenced).  OS2R_COPY_STATE | OS2R_COPY_PARAMS moves everything that
 * determines an environment's future; what stays the destination's is its identity and configuration: the step counter,
 * the seed and env_offset (which key the random streams, so clones diverge on their own under device-drawn actions or noise
 * and replay exactly under explicit actions), the task, the solver settings and the caller-set output buffers.
 *   index_dev  [dst num_envs] int32 device memory; NULL: the identity map (needs equal num_envs)
 *   what       OS2R_COPY_* bits, at least one
 *   obs_dev    nullable, [dst num_envs][dst obs_dim]: the observation of EVERY environment of `dst` after the copy, kept ones
 *              included, under dst's task: the observation of the stored state, as the reset returns it; for equal tasks it
 *              is, bit for bit, what the source's last step or reset returned for src[i]
 * `src` == `dst` is allowed with any map (permutation, broadcast, partial): the result is as if all reads preceded all
 * writes; the rows go through a buffer owned by the handle, allocated by the first such call (which synchronises for it;
 * every later call allocates nothing).  The two handles must agree in dtype, device and robot (Os2rModel equal bit for bit,
 * gravity_z excluded, as for os2r_register_model_kernels); num_envs, task, reward, auto_reset, solver settings and env_offset
 * may differ.  After a copy of parameters from a handle with per-environment parameters (or another gravity) the
 * destination's kernels read the parameter arrays per lane, as after os2r_set_params.  Stream-ordered on `stream`; the
 * caller orders src's pending work before it.  Nothing synchronises the host.
 * Errors: OS2R_ERR_INVALID for a null handle (null dst: os2r_last_error(NULL)), what == 0 or an unknown bit, a dtype, device
 * or model mismatch, or the identity map with unequal num_envs; os2r_last_error(dst) names the cause.                       */
#define OS2R_COPY_STATE 1   /* q, qd, action history 0 and 1, solver impulses and flags, elapsed steps, episode index, pose id */
#define OS2R_COPY_PARAMS 2  /* mass_scale, damping, friction, mu, gravity */
OS2R_API int os2r_copy_envs(Os2rSim* dst, Os2rSim* src, const int32_t* index_dev, int32_t what, void* obs_dev, void* stream);

/* Finite-difference Jacobians of one env-step, in one launch.  For every environment e let x = (q_0 .. q_{nq-1},
 * qd_0 .. qd_{nq-1}) be the stored state and a = actions_dev[e] ([num_envs][2], the handle's dtype), clamped to [-1, 1]
 * silently: this is a query and counts no violation.  The transition f(x, a) is the (q, qd) an os2r_step with that action
 * leaves after its `substeps` physics iterations, started from the environment's own solver state and parameters: no
 * observation, reward, done or reset (as on a handle with auto_reset = 0).
 *   eps        {eps_q [rad], eps_qd [rad/s], eps_a [action units]}, host memory, read before the call returns; each finite
 *              and > 0 (also after rounding to the handle's dtype), eps[2] < 1
 *   Points, all in the handle's dtype: state column j is evaluated at x_j + h and x_j - h (one rounded add each; h = eps[0]
 *   for a q column, eps[1] for a qd column); action column j at min(a_j + eps[2], 1) and max(a_j - eps[2], -1), so the quotient
 *   turns one-sided at a torque limit on its own.  Column j of A or B is (f(hi) - f(lo)) / (hi - lo): one rounded subtraction
 *   above, one below, one IEEE division -- in fp32 too.
 *   next_dev   nullable, [2nq][N]: f(x, a), the q' rows first, then the qd' rows
 *   a_dev      nullable, [2nq][2nq][N]: element [i][j] = d x'_i / d x_j
 *   b_dev      nullable, [2nq][2][N]:   element [i][j] = d x'_i / d a_j
 * All three are struct-of-arrays with the environment index fastest; at least one is required, and the evaluations of a null
 * output are not run.  The columns are independent waves: 64 environments of the 5-dof robot fill 25 SIMDs.
 * The handle is only read: state, solver state, histories, parameters, episode and step counters, the violation count and
 * its mirror, the done-reason / done-mask buffers and the work counters are as they were.  Stream-ordered on `stream`, no
 * host synchronisation, no allocation, no buffer of the handle's.
 * Contract: every f(.) above equals, bit for bit, what os2r_step leaves in os2r_get_state when started from that point, the
 * same solver state, the same parameters and that action, for every configuration os2r_create accepts.  For a robot that
 * runs a registered code object (os2r_register_model_kernels) that holds against the robot's own step kernels whenever its
 * registrations export the matching os2r_jit_lin_* kernel (gym_os2r_amd/jit.py builds them all).  Only where they do not
 * -- an object built by hand without them, OS2R_JIT_FUSED=0 in the Python package -- this call runs the generic
 * run-time-model kernels of the library, and the equality holds against those (a handle created without any registration).
 * A quotient whose two evaluations end in different contact modes is the secant across the kink: eps is the caller's tool,
 * the library does not judge it.
 * Errors: OS2R_ERR_INVALID for a null handle (os2r_last_error(NULL)), null actions_dev, null eps, all outputs null, an eps
 * that is not finite or not > 0, or eps[2] >= 1; os2r_last_error names the cause.                                          */
OS2R_API int os2r_linearize(Os2rSim* sim, const void* actions_dev, const double eps[3], void* next_dev, void* a_dev, void* b_dev,
                            void* stream);

/* Batched backward Riccati recursion (time-varying or stationary discrete LQR) in one launch: the gains K_k of
 * a = a0 - K_k (x - x_k) for many independent trajectories, from Jacobians in os2r_linearize's layout, written in the layout
 * os2r_rollout_policy_scheduled reads.  The handle supplies the dtype, nq (n = 2 nq), the device and the task's observation
 * layout and is only read, as by os2r_linearize: no write to state, counters, mirror or a buffer of the handle's, no allocation,
 * no host synchronisation, stream-ordered.  nknots * ntraj need not be the handle's num_envs.
 * With K = nknots, M = ntraj, L = K M, lane of (knot k, trajectory m) = k M + m; every device array in the handle's dtype:
 *   a_dev       [n][n][L], os2r_linearize's a_dev of a handle whose environments are ordered knot-major
 *   b_dev       [n][2][L]
 *   q_host      [n][n] row-major doubles, r_host [2][2]: host memory, read before the call returns, passed as kernel arguments;
 *               finite and exactly symmetric; rounded once to the handle's dtype
 *   p_final_dev nullable, [n][n][M]: the cost-to-go behind the last knot, upper triangle (i <= j) read; NULL: Q.  p_out_dev may
 *               alias it
 *   gain_dev    nullable, [K][2][n][M]: K_k
 *   p_out_dev   nullable, [n][n][M]: P after the last processed knot, both triangles
 *   flag_dev    nullable, [K][M] uint8: 1 where the knot's 2 x 2 system was refused (below), else 0; the last sweep's verdict
 *   weights_dev nullable, [K][2][D+1][M]: the OS2R_POLICY_PER_ENV table of os2r_rollout_policy_scheduled with period = K; needs
 *               actions_dev [L][2] (the array given to os2r_linearize; clamped to [-1, 1] as there) and obs_dev [L][D] (the
 *               observation at each knot, as os2r_copy_envs returns it)
 *   sweeps      >= 1: the knots are passed `sweeps` times, each from k = K-1 down to 0, P carried across (nknots = 1: the
 *               stationary iteration; several knots: the periodic Riccati iteration of a wrapped schedule); gains, flags and
 *               weights are those of the last pass
 * At least one of gain_dev, p_out_dev, weights_dev is required.
 * Arithmetic (part of the contract): the handle's dtype, every product rounded on its own (no fused multiply-add), every sum of
 * products sum_l x_l y_l evaluated as ((x_0 y_0 + x_1 y_1) + x_2 y_2) + ... with l ascending.  Per knot, A = A_k, B = B_k, P the
 * current symmetric cost-to-go:
 *   1. PB[i][c] = sum_l P[i][l] B[l][c];  S00 = R00 + sum_l B[l][0] PB[l][0],  S01 = R01 + sum_l B[l][0] PB[l][1],
 *      S11 = R11 + sum_l B[l][1] PB[l][1]
 *   2. det = S00 S11 - S01 S01;  ok = S00 > 0 and det > 0 and det finite
 *   3. PA[i][j] = sum_l P[i][l] A[l][j];  G[c][j] = sum_l B[l][c] PA[l][j]
 *   4. K[0][j] = (S11 G[0][j] - S01 G[1][j]) / det,  K[1][j] = (S00 G[1][j] - S01 G[0][j]) / det, one IEEE division each (in
 *      fp32 too); a knot that is not ok gets K = 0 and flag 1, and the recursion goes on with that K (P <- Q + A^T P A)
 *   5. for i <= j: P'[i][j] = (Q[i][j] + sum_l A[l][i] PA[l][j]) - (G[0][i] K[0][j] + G[1][i] K[1][j]),  P'[j][i] = P'[i][j]
 *   6. weights: slot d of kind OS2R_OBS_POS_RAW / OS2R_OBS_POS_PERIODIC_RAW shows state column obs_src[d], of kind
 *      OS2R_OBS_VEL_RAW column nq + obs_src[d]: W[k][j][d] = -K[j][column]; every other slot gets 0;
 *      W[k][j][D] = a0_j - sum_d W[k][j][d] o0_d, the sum over the raw slots in slot order
 * The library does not judge Q >= 0 or the conditioning: flag_dev is the caller's tool.
 * Errors: OS2R_ERR_INVALID for a null handle (os2r_last_error(NULL)); nknots, ntraj or sweeps < 1; null a_dev, b_dev, q_host
 * or r_host; a Q or R that is not finite or not symmetric; all outputs null; weights_dev without actions_dev or obs_dev;
 * os2r_last_error names the cause.                                                                                          */
OS2R_API int os2r_lqr_gains(Os2rSim* sim, int32_t nknots, int64_t ntraj, int32_t sweeps,
                            const void* a_dev, const void* b_dev,
                            const double* q_host, const double* r_host,
                            const void* p_final_dev, void* gain_dev, void* p_out_dev, uint8_t* flag_dev,
                            const void* actions_dev, const void* obs_dev, void* weights_dev, void* stream);

/* Global step counter that keys the on-device action RNG. */
OS2R_API int os2r_get_step_count(Os2rSim* sim, uint64_t* out);
OS2R_API int os2r_set_step_count(Os2rSim* sim, uint64_t value);

/* Timing helper for benchmarks: runs `nsteps` os2r_step launches with on-device
 * random actions on the given stream, bracketed by HIP events recorded on that
 * stream; returns the elapsed GPU time in milliseconds. Every output of os2r_step
 * (observation, reward, done, terminal observation) goes to internal scratch
 * buffers: the timed launch is the one a gym-level env.step makes.
 * elapsed_ms == NULL: the launches are only enqueued (no events, no synchronisation) -- for a caller that drives
 * several handles on several streams (shards of one batch that advance independently) and times them itself.  */
OS2R_API int os2r_bench_steps(Os2rSim* sim, int nsteps, void* stream, float* elapsed_ms);
/* The same for `count` handles on `count` streams -- the shards of one batch --, enqueue only: step k of every shard is
 * enqueued before step k + 1 of any (round robin), so that all the streams start together.                        */
OS2R_API int os2r_bench_steps_multi(Os2rSim* const* sims, void* const* streams, int count, int nsteps);

/* Work counters (measurement support, bench.py's roofline): while a buffer of OS2R_NUM_WORK_COUNTERS uint64 (device
 * memory, zeroed by the caller) is set, os2r_step launches the counting variant of the step kernel -- the same
 * arithmetic, bit for bit -- whose waves add the work they did to it: [0] wave x physics iterations, [1] bodies whose
 * candidate scan ran, [2] bodies whose contact rows were set up, [3] phase-2 sweeps x bodies they covered,
 * [4] phase-2 sweeps executed, [5] (environment, body) contacts, [6] phase-2 sweeps x environments still live in
 * them, [7] wave x iterations that evaluated sin/cos in full, [8] exact free-set solves executed by waves, [9] exact
 * solves x environments that took part.  Counting variants exist for the compiled-in robots
 * with ground contact, the default sweep counts and a reference task layout (OS2R_ERR_INVALID otherwise).
 * NULL switches counting off.                                                                                   */
#define OS2R_NUM_WORK_COUNTERS 10
OS2R_API int os2r_set_work_counters(Os2rSim* sim, uint64_t* counters_dev);

/* Done reasons (replaces the debug line that names the observation which caused a reset,
 * gym_os2r/tasks/monopod.py:288-296): while a buffer of num_envs uint16 (device memory) is set, every os2r_step
 * writes per environment which observation slots were outside the reset space at the end of the step -- bit d:
 * slot d of the task's observation layout (a non-finite value counts) -- i.e. what set bit0 of `done`; 0 for an
 * environment that is not done or only truncated.  NULL switches it off.                                       */
OS2R_API int os2r_set_done_reasons(Os2rSim* sim, uint16_t* reason_dev);

/* Done mask (ABI 5): while a buffer of num_envs uint8 (device memory) is set, every os2r_step also writes 1 where `done` is
 * non-zero and 0 elsewhere -- the boolean `done` that GazeboRuntime.step returns (gym_os2r/runtimes/gazebo_runtime.py:91-97)
 * and SubprocVecEnv stacks (common/vec_env/subproc_vec_env.py:119-123), so a host binding needs no kernel of its own to turn
 * the flag bits into it.  A binding that hands out a fresh array per step sets the pointer before each call (a pointer store).
 * Not written by os2r_rollout.  NULL switches it off.                                                                     */
OS2R_API int os2r_set_done_mask(Os2rSim* sim, uint8_t* mask_dev);

OS2R_API const char* os2r_last_error(Os2rSim* sim); /* sim == NULL: error of the last failed create */

#ifdef __cplusplus
}
#endif
#endif /* OS2R_H_ */
