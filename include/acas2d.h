/*
 * acas2d.h -- C ABI of the MI355X-native batched ACAS2D step engine (libacas2d_hip.so).
 *
 * The reference (Christos-14/gym-ACAS2D) is pure Python and has no FFI; the boundary it exposes
 * for this path is the gym.Env surface  ACAS2DEnv.reset() / ACAS2DEnv.step(action)
 * (gym_ACAS2D/envs/environment.py:29-48).  Each entry point below names the reference interface
 * it replaces.  The Python host (gym-acas2d_amd/) binds these with ctypes; INTEGRATION.md shows
 * the stub a reference maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / C++ types cross this boundary;
 *   - every pointer in Acas2dState / Acas2dStepIO is a DEVICE pointer owned by the caller; the
 *     library allocates nothing, keeps no global state besides a thread-local error string;
 *   - all calls are asynchronous on `stream` (a hipStream_t passed as void*, NULL = default
 *     stream) and are safe to capture into a hipGraph;
 *   - return value: 0 on success, negative ACAS2D_E* on failure, text via acas2d_last_error();
 *     no exceptions cross the ABI.  Where the reference raises ValueError for NaN headings
 *     (rewards.py:6-9) the engine propagates NaN instead;
 *   - `_f32` / `_f64` give the element type of every floating-point buffer (`void*` fields).
 *
 * Data layout in HBM (struct of arrays; E = n_envs, N = n_traffic, D = 5 + 3N):
 *   own_x, own_y, own_psi, own_v           T[E]      player aircraft      (aircraft.py:8-14)
 *   goal_x, goal_y                         T[E]      goal position        (game.py:80-81)
 *   trf_x, trf_y, trf_psi, trf_v           T[E][N]   traffic block, env-major so that one env's
 *                                                    block is contiguous  (game.py:96-116)
 *   steps                                  i32[E]    game.steps           (game.py:30,197)
 *   total_reward                           T[E]      game.total_reward    (game.py:32,287)
 *   status                                 u8[E]     0 = running, else latched outcome
 *                                                    (game.running/outcome, game.py:36,39)
 *   episode                                u32[E]    reset counter (input of the reset RNG)
 *   actions T[E]; obs T[E][D] row-major; reward T[E]; done u8[E]; outcome u8[E]
 */
#ifndef ACAS2D_H
#define ACAS2D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ACAS2D_ABI_VERSION 7

/* error codes */
#define ACAS2D_OK 0
#define ACAS2D_EINVAL (-22)  /* bad argument (NULL pointer, n_traffic < 1, ...) */
#define ACAS2D_EHIP (-5)     /* HIP runtime error at launch */

/* step flags */
#define ACAS2D_AUTO_RESET 1u /* SB3 VecEnv semantics: reset finished envs inside the step */

/* Acas2dConfig.math.  The float32 entry points always run the FAST formulation (algebraically identical to
 * the reference, fewer roundings, hardware transcendentals; 1e-5-grade observations).  The float64 entry points
 * run  DEFAULT: the reference's operation order literally, with libm (agrees with the CPU reference to ~1e-13:
 *               the parity mode);
 *      FAST:    the FAST formulation in float64 arithmetic -- d_cpa and d_dev in their algebraic forms (no
 *               atan2 / atan / sin per aircraft), reciprocal multiplications, a range-limited sincos -- within
 *               1e-9 of the reference on every fixture (tests/test_gpu_parity.py), at more than twice the rate.
 *               One documented difference: the SIGN of a d_cpa observation entry is unspecified where the
 *               reference's relative velocity component v12x is an exact 0 (|v12x| < 1e-9: equal airspeeds with
 *               parallel or mirror-image headings) -- kinematics.py:47 takes arctan(v12y / v12x), whose sign there
 *               is a coin toss of libm's cos; the magnitude still agrees to 1e-9 and DEFAULT reproduces the sign. */
#define ACAS2D_MATH_DEFAULT 0
#define ACAS2D_MATH_FAST 1

/* outcome codes = settings.py:6 OUTCOME_NAMES */
#define ACAS2D_OUTCOME_NONE 0
#define ACAS2D_OUTCOME_GOAL 1
#define ACAS2D_OUTCOME_COLLISION 2
#define ACAS2D_OUTCOME_TIMEOUT 3

/* Every tunable of gym_ACAS2D/settings.py:1-54 that the step path reads, plus the normalisers
 * of game.py:120-128 and rewards.py:22-23,46-47 (constants under the reference's fixed start and
 * goal).  Always float64 here; the f32 entry points round each field once on the host. */
typedef struct Acas2dConfig {
    double dt;               /* 1 / FPS                          aircraft.py:18        */
    double acc_lat_limit;    /* ACC_LAT_LIMIT                    settings.py:42        */
    int32_t max_steps;       /* MAX_STEPS                        settings.py:9         */
    int32_t math;            /* ACAS2D_MATH_*: which formulation the float64 entry points run */
    double collision_dist;   /* 2 * COLLISION_RADIUS             game.py:187           */
    double goal_radius;      /* GOAL_RADIUS                      game.py:192           */
    double safe_distance;    /* SAFE_DISTANCE                    rewards.py:16         */
    double d_goal_max;       /* obs normaliser                   game.py:120           */
    double d_dev_max;        /* obs normaliser                   game.py:122           */
    double d_sep_max;        /* obs normaliser                   game.py:124           */
    double d_cpa_max;        /* obs normaliser                   game.py:126           */
    double v_closing_max;    /* obs normaliser                   game.py:128           */
    double rw_d_goal_max;    /* reward-side d_goal_max           rewards.py:46-47      */
    double rw_d_dev_max;     /* reward-side d_dev_max            rewards.py:22-23      */
    double reward_goal;      /* REWARD_GOAL                      settings.py:47        */
    double reward_collision; /* REWARD_COLLISION                 settings.py:48        */
    /* reset distribution, game.py:80-116 */
    double own_x0, own_y0, own_v;       /* game.py:85-87                                */
    double own_heading0;                /* relative_angle(start -> goal), game.py:91    */
    double own_heading_jitter;          /* PLAYER_INITIAL_HEADING_LIM, settings.py:43   */
    double goal_x, goal_y;              /* game.py:80-81                                */
    double t0_x, t0_y_base, t0_y_span;  /* game.py:100-101                              */
    double t0_heading_base, t0_heading_step, t0_heading_jitter; /* game.py:105-106      */
    double tn_x_max, tn_y_max;          /* game.py:109-110                              */
    double speed_factor_min, speed_factor_max, airspeed;        /* game.py:103,112      */
} Acas2dConfig;

/* Per-env state, device pointers (element type T = float for _f32, double for _f64). */
typedef struct Acas2dState {
    void *own_x, *own_y, *own_psi, *own_v;
    void *goal_x, *goal_y;
    void *trf_x, *trf_y, *trf_psi, *trf_v;
    int32_t *steps;
    void *total_reward;
    uint8_t *status;
    uint32_t *episode;
    /* Optional (NULL = off): T[E][16], the per-step record row behind testing_main.py:114-138's CSV columns
     * (the lists ACAS2DGame appends to, game.py:132-160, :231-241, :266-276):
     *   [0] psi  [1] d_sep (minimum separation AFTER the player moved and BEFORE the traffic did, :236-237)
     *   [2] a_lat  [3] d_goal  [4] delta_heading  [5] v_closing  [6] d_cpa  [7] d_dev
     *   [8] r_d_goal  [9] r_h_goal  [10] r_d_cpa  [11] r_d_dev  [12] r_step (step reward before the terminal
     *   bonuses; the undiscounted step_reward_5 in the row acas2d_reset_* writes, :160)  [13..15] zero.
     * Written by acas2d_step_* WITHOUT ACAS2D_AUTO_RESET (the single-env semantics those scripts run) and by
     * acas2d_reset_* when it computes an observation. */
    void *trace;
} Acas2dState;

/* Inputs / outputs of one step, device pointers.  term_obs, ep_return, ep_steps may be NULL. */
typedef struct Acas2dStepIO {
    const void *actions; /* T[E]      action[0] in [-1, 1]              game.py:225           */
    void *obs;           /* T[E][D]   observe()                         game.py:194-220       */
    void *reward;        /* T[E]      evaluate()                        game.py:249-292       */
    uint8_t *done;       /* u8[E]     is_done()                         game.py:294-314       */
    uint8_t *outcome;    /* u8[E]     game.outcome of THIS step (0 while running)             */
    void *term_obs;      /* T[E][D]   AUTO_RESET: last obs of a finished episode (rows of
                                      envs that did not finish are left untouched)            */
    void *ep_return;     /* T[E]      AUTO_RESET: game.total_reward at done                   */
    int32_t *ep_steps;   /* i32[E]    AUTO_RESET: game.steps at done (= step() calls + 1)     */
} Acas2dStepIO;

int acas2d_abi_version(void);
size_t acas2d_config_size(void);      /* sizeof(Acas2dConfig): layout check for bindings */
size_t acas2d_state_size(void);       /* sizeof(Acas2dState) */

const char *acas2d_last_error(void);  /* thread-local; valid until the next failing call  */

/*
 * acas2d_step_*: replaces ACAS2DEnv.step(action) (environment.py:29-42) for n_envs independent
 * envs: game.action -> game.observe -> game.evaluate -> game.is_done, one kernel launch.
 *   flags & ACAS2D_AUTO_RESET: finished envs store term_obs/ep_return/ep_steps, bump episode[e],
 *     are re-initialised with the distribution of game.py:80-116 from the counter-based RNG
 *     Philox4x32-7(key = seed, counter = (env_offset + e, episode[e], entity)) and return the
 *     new episode's first observation in obs (SB3 DummyVecEnv.step_wait semantics).
 *   otherwise: status[e] latches the outcome; stepping a finished env keeps moving the player
 *     but freezes its traffic (game.py:243-245).
 * env_offset = global index of env 0 of this shard (results are invariant to the sharding).
 *
 * state_out (ABI 6): NULL or == state: the step updates `state` in place.  Otherwise DOUBLE-BUFFERED state: the
 *   step reads `state` and writes the arrays it rewrites for every env -- own_x, own_y, own_psi, steps,
 *   total_reward, trf_x, trf_y -- into state_out's buffers instead (the caller then passes the two structs the
 *   other way round at the next step; results are bit-identical to stepping in place).  Why: a store that hits
 *   a cache line its launch loaded stays dirty in the XCD's L2 until the write-back at the END of the kernel,
 *   whereas stores to the other generation stream out during it (65 536 x 8 float32: 4.23 vs 4.65 us per launch).
 *   Layout contract: state_out's own_x, own_y, own_psi, steps and total_reward lie at ONE element offset from
 *   state's, its trf_x and trf_y at one (e.g. every such array allocated as [2][E] / [2][E][N], the two structs
 *   pointing at the two halves), less than 2^31 elements away, and not one byte of them inside any array of
 *   `state` (trace aside) -- the arrays shared between the two included; every other field (own_v,
 *   goal_*, trf_psi, trf_v, status, episode, trace: changed at a reset only, in place) is the SAME buffer in
 *   both structs.  Needs ACAS2D_AUTO_RESET.  A hipGraph that captures an odd number of steps must not be
 *   replayed twice in a row (each replay would read the generation the previous one also read).
 *
 * Consecutive layout (ABI 7; optional, detected per launch, results identical either way): when the float32 arrays a
 *   step READS are consecutive rows of four blocks --
 *       own_x, own_y, own_psi, total_reward, steps     T[5][E]        own_v, goal_x, goal_y, episode    T[4][E]
 *       trf_x, trf_y                                   T[2][E][N]     trf_psi, trf_v                    T[2][E][N]
 *   (i.e. own_y == own_x + E, ..., (void*)steps == own_x + 4 E, trf_y == trf_x + E N, ...; a second generation is then
 *   a whole second T[5][E] / T[2][E][N] block, which satisfies state_out's contract above) -- five base pointers and the
 *   env count name every input of the step.  gfx950 hands the first 14 dwords of a kernel's arguments to each wavefront
 *   in registers, so the auto-reset step then issues ALL its loads with its first instructions instead of behind a
 *   scalar-load round trip to the argument segment (65 536 x 8: 5.19 -> 4.7 us per launch, 4.36 -> 3.8 where no env
 *   finishes).  Needs n_traffic with a packed work shape, E N < 2^29, and n_envs a whole multiple of eight workgroups'
 *   envs (1 024 at n_traffic = 8: the kernel then has no bounds checks).  acas2d_state_is_consecutive() tells whether
 *   a state qualifies; any other layout or size runs the general kernel.
 *
 * n_envs < 2^31 per call (shard beyond that: env_offset).
 */
int acas2d_step_f32(const Acas2dConfig *cfg, const Acas2dState *state, const Acas2dState *state_out,
                    const Acas2dStepIO *io, uint32_t flags, uint64_t seed, int64_t env_offset,
                    int64_t n_envs, int32_t n_traffic, void *stream);
int acas2d_step_f64(const Acas2dConfig *cfg, const Acas2dState *state, const Acas2dState *state_out,
                    const Acas2dStepIO *io, uint32_t flags, uint64_t seed, int64_t env_offset,
                    int64_t n_envs, int32_t n_traffic, void *stream);

/*
 * acas2d_rollout_*: n_steps consecutive ACAS2DEnv.step() calls fused into ONE launch -- the inner
 * loop of a rollout collector (baseline_main.py:39-61 / testing_main.py:69-105 with the actions
 * known up front; SB3's collect_rollouts once the policy runs on the device).  The state stays in
 * registers, step t reads actions[t][E] and writes obs[t][E][D], reward[t][E], done[t][E],
 * outcome[t][E]; term_obs [t][E][D], ep_return [t][E], ep_steps [t][E] are optional (NULL) and
 * written only where done[t][e].  ACAS2D_AUTO_RESET semantics always.  Bit-identical to n_steps
 * acas2d_step_* calls.  Needs a packed work shape: n_traffic in {1, 2, 3} or a multiple of
 * 16 / sizeof(T) that tiles a wave (4, 8, 16, 32, 64 for f32), else ACAS2D_EINVAL.
 */
int acas2d_rollout_f32(const Acas2dConfig *cfg, const Acas2dState *state, const Acas2dStepIO *io,
                       int32_t n_steps, uint64_t seed, int64_t env_offset, int64_t n_envs,
                       int32_t n_traffic, void *stream);
int acas2d_rollout_f64(const Acas2dConfig *cfg, const Acas2dState *state, const Acas2dStepIO *io,
                       int32_t n_steps, uint64_t seed, int64_t env_offset, int64_t n_envs,
                       int32_t n_traffic, void *stream);

/*
 * acas2d_rollout_policy_*: the rollout above with the policy evaluated INSIDE the kernel -- the
 * whole loop of testing_main.py:69-105 (`action, _ = model.predict(obs, deterministic=True);
 * obs, reward, done, info = env.step(action)`) in one launch.  The policy is Stable-Baselines3
 * 1.1.0's MlpPolicy actor as stored in the reference's model zips (policy.pth:
 * mlp_extractor.policy_net.{0,2}, action_net): obs -> Linear(D,64) tanh -> Linear(64,64) tanh ->
 * Linear(64,1); the deterministic action is the mean clipped to [-1, 1].  float32 weights and
 * float32 arithmetic in both element types (policy.predict() casts the observation to float32).
 *   obs_in          T[E][D]  the observation the first action is taken on (reset()'s / the last step's)
 *   io->actions     T[n_steps][E]  OUTPUT here: the action each step took
 *   everything else as acas2d_rollout_*.
 * Needs a thread-per-env work shape: n_traffic in {1, 2, 3, 4, 8} (f32) / {1, 2, 3} (f64); float32 with 8, 16, 32
 * or 64 traffic aircraft: acas2d_rollout_policy_group_f32 below (likewise for acas2d_collect_* and
 * acas2d_evaluate_policies_*).
 */
typedef struct Acas2dPolicy {
    const void *w1t, *b1;    /* float[D][64]  = policy_net.0.weight TRANSPOSED, float[64] */
    const void *w2t, *b2;    /* float[64][64] = policy_net.2.weight TRANSPOSED, float[64] */
    const void *w3, *b3;     /* float[64]     = action_net.weight,              float[1]  */
    int32_t hidden;          /* 64 */
    int32_t _pad;
} Acas2dPolicy;

int acas2d_rollout_policy_f32(const Acas2dConfig *cfg, const Acas2dState *state, const Acas2dStepIO *io,
                              const Acas2dPolicy *policy, const void *obs_in, int32_t n_steps,
                              uint64_t seed, int64_t env_offset, int64_t n_envs, int32_t n_traffic,
                              void *stream);
int acas2d_rollout_policy_f64(const Acas2dConfig *cfg, const Acas2dState *state, const Acas2dStepIO *io,
                              const Acas2dPolicy *policy, const void *obs_in, int32_t n_steps,
                              uint64_t seed, int64_t env_offset, int64_t n_envs, int32_t n_traffic,
                              void *stream);

/*
 * acas2d_collect_*: the collector of one PPO iteration in ONE launch -- SB3 1.1.0's `collect_rollouts` as
 * training_main.py:44-52 runs it through `PPO.learn()`: for n_steps steps, `actions, values, log_probs =
 * policy(obs)` (the action DRAWN from N(mean, exp(log_std))), `env.step(clip(actions, -1, 1))`.  acas2d_rollout_policy_*
 * with the value net and the Gaussian sampling inside the kernel:
 *   actor, obs_in, io                 as acas2d_rollout_policy_*; io->actions[t][e] receives the RAW (unclipped) action
 *   v1t .. vb3                        the value net, same layout as the actor (mlp_extractor.value_net.{0,2}, value_net)
 *   log_std                           float[1]
 *   values, logp                      T[n_steps][E] outputs: V(obs_t), log N(action_t; mean_t, exp(log_std))
 *   noise_seed, noise_step            eps ~ N(0, 1) comes from Philox4x32-7(key = noise_seed, counter = (env_offset + e,
 *                                     noise_step + t, tag)) by Box-Muller: the stream depends on the global env index and
 *                                     the step number only (pass the number of steps collected so far)
 * A non-finite observation entry (the reference's NaN d_cpa in exact parallel flight, kinematics.py:48) reaches the
 * two networks as 0; the observation itself is stored as it is.  Same work shapes as acas2d_rollout_policy_*.
 */
typedef struct Acas2dActorCritic {
    Acas2dPolicy actor;
    const void *v1t, *vb1;   /* float[D][64]  = value_net.0.weight TRANSPOSED, float[64] */
    const void *v2t, *vb2;   /* float[64][64] = value_net.2.weight TRANSPOSED, float[64] */
    const void *v3, *vb3;    /* float[64]     = value_net.weight,              float[1]  */
    const void *log_std;     /* float[1] */
    void *values, *logp;     /* T[n_steps][E] */
    uint64_t noise_seed;
    uint32_t noise_step;
    uint32_t _pad;
} Acas2dActorCritic;

int acas2d_collect_f32(const Acas2dConfig *cfg, const Acas2dState *state, const Acas2dStepIO *io,
                       const Acas2dActorCritic *ac, const void *obs_in, int32_t n_steps, uint64_t seed,
                       int64_t env_offset, int64_t n_envs, int32_t n_traffic, void *stream);
int acas2d_collect_f64(const Acas2dConfig *cfg, const Acas2dState *state, const Acas2dStepIO *io,
                       const Acas2dActorCritic *ac, const void *obs_in, int32_t n_steps, uint64_t seed,
                       int64_t env_offset, int64_t n_envs, int32_t n_traffic, void *stream);

/*
 * acas2d_collect_set_f32: acas2d_collect_f32 for K independent actor-critics ("members": the seeds or hyper-parameter
 * sets of a sweep) in ONE launch.  Additive to ABI 7.
 *   ac                ONE Acas2dActorCritic whose weight pointers name K stacks, in the layouts acas2d_evaluate_policies_*
 *                     documents for the actor: w1t float[K][D][64], b1 float[K][64], w2t float[K][64][64], b2 float[K][64],
 *                     w3 float[K][64], b3 float[K][1]; v1t .. vb3 likewise; log_std float[K].  ac->noise_seed is ignored.
 *   n_members         K >= 1
 *   noise_seeds       DEVICE uint64[K]: member k's noise key.  The counter is acas2d_collect_*'s: (global env index,
 *                     ac->noise_step + t)
 *   n_envs            K * EM with EM a multiple of 64: member k owns the envs [k EM, (k + 1) EM), so that a wavefront's
 *                     envs belong to one member and its weights stay scalar operands
 *   io, values, logp  the collector's [n_steps][n_envs] layout
 * The slice of member k equals acas2d_collect_f32 run alone on those envs -- policy k, noise_seed = noise_seeds[k],
 * env_offset + k EM, the same env seed -- bit for bit: per step it is that launch's code.  Rejected with ACAS2D_EINVAL
 * before anything is launched: n_members < 1, an n_envs that is not K x a multiple of 64, a NULL stack or noise_seeds,
 * and any n_traffic outside {1, 2, 3, 4, 8}: the group-cooperative launches of n_traffic 16 / 32 / 64 are
 * acas2d_collect_set_group_f32, below.  Out of scope: float64.
 */
int acas2d_collect_set_f32(const Acas2dConfig *cfg, const Acas2dState *state, const Acas2dStepIO *io,
                           const Acas2dActorCritic *ac, int32_t n_members, const uint64_t *noise_seeds,
                           const void *obs_in, int32_t n_steps, uint64_t seed, int64_t env_offset, int64_t n_envs,
                           int32_t n_traffic, void *stream);

/*
 * acas2d_evaluate_policies_*: K deterministic policies scored on the same n_episodes episodes in ONE launch -- the
 * evaluation of testing_main.py / SB3's EvalCallback for a set of checkpoints.  Additive to ABI 7.
 *   state, n_envs     the envs; the first K * EP are used, EP = n_episodes rounded up to a multiple of 64: env
 *                     k * EP + i holds episode i for policy k (i >= n_episodes: padding, never scored)
 *   policies          ONE Acas2dPolicy whose pointers name the K actors stacked: w1t float[K][D][64], b1 float[K][64],
 *                     w2t float[K][64][64], b2 float[K][64], w3 float[K][64], b3 float[K][1]
 *   obs_in            T[K * EP][D]  the observation each env's first action is taken on
 *   n_steps           the step budget (max_steps + 1 covers every episode)
 *   outcome, steps    uint8 / int32 [K][n_episodes]: each env's FIRST episode -- its outcome and game.steps at done,
 *   total_reward      T[K][n_episodes]  and its return; 0 / 0 / 0 where the episode is not done within n_steps
 * Per step the arithmetic of acas2d_rollout_policy_*, so row k equals that rollout of policy k on the same episodes
 * bit for bit.  Nothing else is written: no per-step outputs, and the state is left as it was given.  A lane stops at
 * its episode's end and a wavefront once all its lanes have.  Work shapes as acas2d_rollout_policy_*.
 */
int acas2d_evaluate_policies_f32(const Acas2dConfig *cfg, const Acas2dState *state, int64_t n_envs,
                                 const Acas2dPolicy *policies, int32_t n_policies, int32_t n_episodes,
                                 const void *obs_in, int32_t n_steps, uint64_t seed, int64_t env_offset,
                                 int32_t n_traffic, uint8_t *outcome, int32_t *steps, void *total_reward,
                                 void *stream);
int acas2d_evaluate_policies_f64(const Acas2dConfig *cfg, const Acas2dState *state, int64_t n_envs,
                                 const Acas2dPolicy *policies, int32_t n_policies, int32_t n_episodes,
                                 const void *obs_in, int32_t n_steps, uint64_t seed, int64_t env_offset,
                                 int32_t n_traffic, uint8_t *outcome, int32_t *steps, void *total_reward,
                                 void *stream);

/*
 * acas2d_rollout_policy_group_f32 / acas2d_collect_group_f32 / acas2d_evaluate_policies_group_f32: the three launches
 * above for n_traffic in {8, 16, 32, 64}, float32 -- arguments, outputs and rejections as their siblings'.  Additive
 * to ABI 7.  The env's G lanes of the packed work shapes (4,2) (4,4) (4,8) (4,16) evaluate the network together:
 * each lane 64 / G hidden units (at (4,16) one unit for the four envs of its wavefront), with the same fma sequence per
 * unit and the same order in the head as the thread-per-env kernels, so that at n_traffic = 8 (where both exist) the results are equal bit for bit.  A lane reads
 * its slice of a weight row as 16-byte vectors: w1t, b1, w2t, b2 (v1t, vb1, v2t, vb2) must be 16-byte aligned.
 * Any other traffic count is rejected (ACAS2D_EINVAL; n_traffic in {1, 2, 3, 4} belongs to the siblings).  There are
 * no float64 variants: the float64 policy kernels stay at n_traffic <= 4.
 */
int acas2d_rollout_policy_group_f32(const Acas2dConfig *cfg, const Acas2dState *state, const Acas2dStepIO *io,
                                    const Acas2dPolicy *policy, const void *obs_in, int32_t n_steps,
                                    uint64_t seed, int64_t env_offset, int64_t n_envs, int32_t n_traffic,
                                    void *stream);
int acas2d_collect_group_f32(const Acas2dConfig *cfg, const Acas2dState *state, const Acas2dStepIO *io,
                             const Acas2dActorCritic *ac, const void *obs_in, int32_t n_steps, uint64_t seed,
                             int64_t env_offset, int64_t n_envs, int32_t n_traffic, void *stream);
int acas2d_evaluate_policies_group_f32(const Acas2dConfig *cfg, const Acas2dState *state, int64_t n_envs,
                                       const Acas2dPolicy *policies, int32_t n_policies, int32_t n_episodes,
                                       const void *obs_in, int32_t n_steps, uint64_t seed, int64_t env_offset,
                                       int32_t n_traffic, uint8_t *outcome, int32_t *steps, void *total_reward,
                                       void *stream);

/*
 * acas2d_evaluate_policies_stats_f32 / _f64 / _group_f32: the three evaluation entry points above with per-episode
 * safety statistics -- how close the aircraft came to traffic, for how long it was inside the safe distance, how hard it
 * manoeuvred and how far it left its path: the columns of testing_main.py's CSV that the fused evaluator did not give.
 * Additive to ABI 7.  The arguments of the plain sibling with `stats` in front of `stream`; the same work shapes
 * (thread-per-env n_traffic in {1, 2, 3, 4, 8} float32 and {1, 2, 3, 4} float64, group {8, 16, 32, 64} float32); outcome,
 * steps and total_reward equal the sibling's bit for bit.
 * Six more outputs, [K][n_episodes] like the other three, written with them at the episode's done.  They cover the ROWS
 * OF THE EPISODE'S step() CALLS: rows 1 .. n-1 of the reference's record lists.  Row 0 of those lists, which
 * ACAS2DGame.__init__ appends before the first step, is excluded.
 *   min_sep       T      min over step rows of the minimum separation as action() logs it (game.py:236-237: the player
 *                        has moved, the traffic not yet) -- the values of d_sep_record
 *   min_sep_step  int32  1-based index of the FIRST step row that attains it = its position in d_sep_record
 *   los_steps     int32  number of step rows with d_sep < safe_distance
 *   max_a_lat     T      max over step rows of |a_lat|
 *   max_dev       T      max over step rows of |d_dev| (d_dev is signed in the reference)
 *   sum_dev       T      sum over step rows of |d_dev|: plain adds in step order, so a sequential host sum in T gives the
 *                        same bits; the mean over the episode's rows is sum_dev / (steps - 1)
 * The minimum and the maxima are kept as  x < m ? x : m  /  x > m ? x : m  from +inf / 0, so a NaN never replaces a held
 * value and never counts as a loss of separation (min_sep_step stays 0 if no row ever compared below +inf).  An
 * episode not done within n_steps gets 0 in all six, as in the other three.
 * Rejected with ACAS2D_EINVAL before anything is launched: everything the sibling rejects, a NULL stats, a NULL member
 * of it.
 */
typedef struct Acas2dEvalStats {
    void *min_sep;                 /* T[K][n_episodes] */
    int32_t *min_sep_step;         /* [K][n_episodes] */
    int32_t *los_steps;            /* [K][n_episodes] */
    void *max_a_lat, *max_dev, *sum_dev;   /* T[K][n_episodes] */
} Acas2dEvalStats;
int acas2d_evaluate_policies_stats_f32(const Acas2dConfig *cfg, const Acas2dState *state, int64_t n_envs,
                                       const Acas2dPolicy *policies, int32_t n_policies, int32_t n_episodes,
                                       const void *obs_in, int32_t n_steps, uint64_t seed, int64_t env_offset,
                                       int32_t n_traffic, uint8_t *outcome, int32_t *steps, void *total_reward,
                                       const Acas2dEvalStats *stats, void *stream);
int acas2d_evaluate_policies_stats_f64(const Acas2dConfig *cfg, const Acas2dState *state, int64_t n_envs,
                                       const Acas2dPolicy *policies, int32_t n_policies, int32_t n_episodes,
                                       const void *obs_in, int32_t n_steps, uint64_t seed, int64_t env_offset,
                                       int32_t n_traffic, uint8_t *outcome, int32_t *steps, void *total_reward,
                                       const Acas2dEvalStats *stats, void *stream);
int acas2d_evaluate_policies_stats_group_f32(const Acas2dConfig *cfg, const Acas2dState *state, int64_t n_envs,
                                             const Acas2dPolicy *policies, int32_t n_policies, int32_t n_episodes,
                                             const void *obs_in, int32_t n_steps, uint64_t seed, int64_t env_offset,
                                             int32_t n_traffic, uint8_t *outcome, int32_t *steps, void *total_reward,
                                             const Acas2dEvalStats *stats, void *stream);

/*
 * acas2d_monte_carlo_f32 / _f64 / _group_f32: a Monte Carlo safety campaign -- the evaluation with statistics above, but
 * every lane plays one DRAWN encounter after another and each finished episode is folded into per-policy accumulators on
 * the device.  Additive to ABI 7.  The arguments of acas2d_evaluate_policies_stats_* with n_lanes where that has
 * n_episodes, without the three per-episode outputs, and `mc` where that has `stats`; the same work shapes and the same
 * rejections in the same words.
 *   Lane (k, i), i < n_lanes, is env k * EP + i of the state (EP = n_lanes rounded up to 64; i >= n_lanes: padding, plays
 *   nothing, counts nothing).  It plays the episodes c = first_episode .. first_episode + episodes_per_lane - 1 of RNG index
 *   env_offset + i: the index WITHIN the block, so the K policies meet the same encounters (common random numbers) and
 *   (seed, env_offset + i, c) names an encounter whatever K is.  Episode first_episode arrives as `state` / `obs_in`;
 *   every later one is drawn by the in-step reset of the rollout kernels -- the draws of acas2d_reset_* for that
 *   (seed, index, counter), bit for bit -- and its first observation is observed from the drawn state exactly as
 *   acas2d_reset_*(do_init = 0) observes an injected one, so that an encounter replayed through
 *   acas2d_evaluate_policies_stats_* gives the same bits.  Every lane plays the same NUMBER OF EPISODES, not a step budget:
 *   a budget would cut long episodes and so over-count the short ones, which are the collisions.
 *   n_steps  the launch's step budget; it must cover every episode: n_steps >= episodes_per_lane * max_steps, and
 *            episodes_per_lane * (max_steps + 1) must fit an int32 and episodes_per_lane be at most 2^24 (a lane's sums and a
 *            wavefront's counts are 32-bit within a launch)
 * Accumulators: ADDED TO, NEVER CLEARED -- launches chain, first_episode advancing by episodes_per_lane, and a campaign
 * is as long as wanted while a launch stays short.  The host sets lane_worst_sep to +inf and everything else to 0.
 *   outcome_count      int64 [K][4]        episodes per outcome 0 .. 3 (0 stays 0: every episode ends by timeout at the latest)
 *   sum_steps          int64 [K]           sum of game.steps at done
 *   los_episodes       int64 [K]           episodes with los_steps > 0
 *   sum_los_steps      int64 [K]           sum of los_steps
 *   sep_hist           int64 [K][n_bins]   histogram of the episodes' min_sep: bin (int)(min_sep * inv_bin_width), evaluated
 *                                          in T; a bin >= n_bins and a non-finite value go to bin n_bins - 1
 *   lane_return_sum    double [K][n_lanes] sum of (double)total_reward, plain adds in the lane's episode order
 *   lane_return_sq     double [K][n_lanes] sum of (double)total_reward squared, likewise
 *   lane_worst_sep     T [K][n_lanes]      the smallest min_sep the lane has seen (x < m ? x : m: the first occurrence wins)
 *   lane_worst_episode uint32 [K][n_lanes] the counter of that episode
 * The integer sums are exact and independent of any order; the per-lane ones are bitwise reproducible.  min_sep and
 * los_steps are those of Acas2dEvalStats, restarted at every episode.
 * Rejected with ACAS2D_EINVAL before anything is launched: everything acas2d_evaluate_policies_stats_* rejects, a NULL mc
 * or member, episodes_per_lane < 1, n_bins < 1, first_episode + episodes_per_lane > 2^32, an n_steps that does not cover
 * the episodes.
 */
typedef struct Acas2dMonteCarlo {
    int64_t *outcome_count, *sum_steps, *los_episodes, *sum_los_steps, *sep_hist;
    double *lane_return_sum, *lane_return_sq;
    void *lane_worst_sep;              /* T[K][n_lanes] */
    uint32_t *lane_worst_episode;
    int32_t n_bins;
    int32_t episodes_per_lane;
    double inv_bin_width;              /* handed to the kernel as T */
    uint32_t first_episode;
    uint32_t _pad;
} Acas2dMonteCarlo;
size_t acas2d_monte_carlo_size(void);  /* sizeof(Acas2dMonteCarlo), for bindings */
int acas2d_monte_carlo_f32(const Acas2dConfig *cfg, const Acas2dState *state, int64_t n_envs,
                           const Acas2dPolicy *policies, int32_t n_policies, int32_t n_lanes, const void *obs_in,
                           int32_t n_steps, uint64_t seed, int64_t env_offset, int32_t n_traffic,
                           const Acas2dMonteCarlo *mc, void *stream);
int acas2d_monte_carlo_f64(const Acas2dConfig *cfg, const Acas2dState *state, int64_t n_envs,
                           const Acas2dPolicy *policies, int32_t n_policies, int32_t n_lanes, const void *obs_in,
                           int32_t n_steps, uint64_t seed, int64_t env_offset, int32_t n_traffic,
                           const Acas2dMonteCarlo *mc, void *stream);
int acas2d_monte_carlo_group_f32(const Acas2dConfig *cfg, const Acas2dState *state, int64_t n_envs,
                                 const Acas2dPolicy *policies, int32_t n_policies, int32_t n_lanes, const void *obs_in,
                                 int32_t n_steps, uint64_t seed, int64_t env_offset, int32_t n_traffic,
                                 const Acas2dMonteCarlo *mc, void *stream);

/*
 * acas2d_evaluate_policies_disturbed_f32 / _group_f32, acas2d_monte_carlo_disturbed_f32 / _group_f32,
 * acas2d_disturbance_draw_f32: the evaluation with statistics and the Monte Carlo campaign above under sensor noise and
 * actuator disturbance.  Additive to ABI 7, float32 only.  The arguments of acas2d_evaluate_policies_stats_* /
 * acas2d_monte_carlo_* with `disturbance` in front of `stream`; the same work shapes (thread-per-env n_traffic in
 * {1, 2, 3, 4, 8}, group {8, 16, 32, 64}) and the same rejections in the same words.  With all four standard deviations 0
 * the results equal the undisturbed entries' bit for bit.
 *   Per step, BEFORE the actor: entry 5 + 3 n + c of the observation the actor reads (traffic n; c = 0 normalised
 *   separation, 1 closest-point-of-approach distance, 2 closing speed) becomes  x + s_c * z  -- a float32 multiply and a
 *   float32 add, each rounded -- and is then held to the observation box by comparisons (y < lo ? lo : y > hi ? hi : y;
 *   [0, 1] for c = 0, [-1, 1] else; a NaN stays a NaN).  The five own-ship entries are never touched.  AFTER the actor:
 *   the clipped action becomes  a + s_action * z, held to [-1, 1] the same way; the move, a_lat and max_a_lat see that
 *   action.  A channel whose s is exactly 0 is neither added to nor clamped.  Only what the actor reads is disturbed:
 *   rewards, outcomes and statistics follow from the true state.
 *   The draws: one Philox4x32 block (the reset's generator and rounds) per (lane, episode, step, slot), counter
 *   (lane lo, lane hi, episode, step | slot << 20), key (noise_seed lo, noise_seed hi ^ 0x64697374).  lane = env_offset +
 *   the index within the policy's block (the RNG index of acas2d_monte_carlo_*: K policies meet the same noise); episode =
 *   the lane's current counter in a campaign, noise_episode for every episode of an evaluation; step = game.steps BEFORE
 *   the step's increment; slot 0 the actuator, slot n + 1 traffic n.  With u_i = ((w_i >> 8) + 0.5) / 2^24 and
 *   r(u) = sqrt(-2 ln u): z_sep = r(u1) cos(2 pi u2), z_cpa = r(u1) sin(2 pi u2), z_closing = r(u3) cos(2 pi u4); the
 *   actuator takes r(u1) cos(2 pi u2).  Log, sqrt, sin and cos are the hardware's approximations.  The noise depends on
 *   nothing else: not on K, not on how a campaign is cut into launches, not on the work shape.
 * acas2d_disturbance_draw_f32 writes those normals for lanes first_lane .. + n_lanes - 1, steps first_step .. + n_steps - 1
 * and slots 0 .. n_slots - 1 of one episode as float[n_steps][n_lanes][n_slots][3] = (z_sep, z_cpa, z_closing); slot 0
 * holds the actuator's normal and two zeros.  It calls the device function the two kernels call.
 * Rejected with ACAS2D_EINVAL before anything is launched: everything the undisturbed sibling rejects, a NULL disturbance,
 * a standard deviation that is negative or not finite, max_steps + 1 >= 2^20 (the step field); draw: a NULL out, a count
 * < 1, a negative first_lane or first_step, first_step + n_steps > 2^20, n_slots > 65.
 */
typedef struct Acas2dDisturbance {
    float s_sep, s_cpa, s_closing;     /* standard deviations in units of the NORMALISED observation */
    float s_action;                    /* ... and of the action */
    uint64_t noise_seed;
    uint32_t noise_episode;            /* evaluation: the episode counter of every episode; ignored by the campaign */
    uint32_t _pad;
} Acas2dDisturbance;
size_t acas2d_disturbance_size(void);  /* sizeof(Acas2dDisturbance), for bindings */
int acas2d_evaluate_policies_disturbed_f32(const Acas2dConfig *cfg, const Acas2dState *state, int64_t n_envs,
                                           const Acas2dPolicy *policies, int32_t n_policies, int32_t n_episodes,
                                           const void *obs_in, int32_t n_steps, uint64_t seed, int64_t env_offset,
                                           int32_t n_traffic, uint8_t *outcome, int32_t *steps, void *total_reward,
                                           const Acas2dEvalStats *stats, const Acas2dDisturbance *disturbance,
                                           void *stream);
int acas2d_evaluate_policies_disturbed_group_f32(const Acas2dConfig *cfg, const Acas2dState *state, int64_t n_envs,
                                                 const Acas2dPolicy *policies, int32_t n_policies, int32_t n_episodes,
                                                 const void *obs_in, int32_t n_steps, uint64_t seed, int64_t env_offset,
                                                 int32_t n_traffic, uint8_t *outcome, int32_t *steps, void *total_reward,
                                                 const Acas2dEvalStats *stats, const Acas2dDisturbance *disturbance,
                                                 void *stream);
int acas2d_monte_carlo_disturbed_f32(const Acas2dConfig *cfg, const Acas2dState *state, int64_t n_envs,
                                     const Acas2dPolicy *policies, int32_t n_policies, int32_t n_lanes, const void *obs_in,
                                     int32_t n_steps, uint64_t seed, int64_t env_offset, int32_t n_traffic,
                                     const Acas2dMonteCarlo *mc, const Acas2dDisturbance *disturbance, void *stream);
int acas2d_monte_carlo_disturbed_group_f32(const Acas2dConfig *cfg, const Acas2dState *state, int64_t n_envs,
                                           const Acas2dPolicy *policies, int32_t n_policies, int32_t n_lanes,
                                           const void *obs_in, int32_t n_steps, uint64_t seed, int64_t env_offset,
                                           int32_t n_traffic, const Acas2dMonteCarlo *mc,
                                           const Acas2dDisturbance *disturbance, void *stream);
int acas2d_disturbance_draw_f32(uint64_t noise_seed, int64_t first_lane, int32_t n_lanes, uint32_t episode,
                                int32_t first_step, int32_t n_steps, int32_t n_slots, float *out, void *stream);

/*
 * acas2d_evaluate_policies_correlated_f32 / _group_f32, acas2d_monte_carlo_correlated_f32 / _group_f32: the disturbed
 * entries above with an error that PERSISTS -- a first-order Gauss-Markov process per channel in place of the white
 * normals.  Additive to ABI 7, float32 only.  The arguments of the _disturbed sibling with `correlation` in front of
 * `stream`; the same work shapes, the same rejections in the same words.
 *   One coefficient rho in [0, 1] per channel (separation, closest-point-of-approach distance, closing speed, action),
 *   shared by all traffic aircraft, and one process per (traffic aircraft, channel) and one for the actuator: 3 N + 1
 *   values of state per env, local to the launch.  With z_t the sibling's normal of the step (the same block at the same
 *   counter: nothing about the draws changes) the error that takes z_t's place everywhere is
 *     e_t = z_t                                    at the first step a lane plays of an episode in this launch: its first
 *                                                  step of the launch, and the first step after an in-step reset;
 *     e_t = (rho * e_{t-1}) + (q * z_t)            otherwise: two float32 multiplies and a float32 add, each rounded, no fma,
 *   with the gain q = (float)sqrt(1.0 - (double)rho * (double)rho) formed on the host.  e has unit variance at every step,
 *   so s stays the standard deviation.  A channel whose rho is exactly 0 takes e_t = z_t and does no arithmetic: with all
 *   four 0 the results equal the _disturbed entries' bit for bit.  rho = 1 gives q = 0 and e_t = e_1: a constant offset
 *   s * z_1 per (lane, episode, channel, aircraft).  x + s * e, the box and "s == 0 leaves the channel alone" are the
 *   sibling's.  acas2d_disturbance_draw_f32 and a scan on the host reproduce any episode.
 * Rejected with ACAS2D_EINVAL before anything is launched: everything the _disturbed sibling rejects, in its words and its
 * order; then a NULL correlation; then a rho that is NaN, negative or above 1.
 */
typedef struct Acas2dCorrelation {
    float rho_sep, rho_cpa, rho_closing;   /* the step-to-step correlation of each observation channel's error */
    float rho_action;                      /* ... and of the actuator's */
} Acas2dCorrelation;
size_t acas2d_correlation_size(void);  /* sizeof(Acas2dCorrelation), for bindings */
int acas2d_evaluate_policies_correlated_f32(const Acas2dConfig *cfg, const Acas2dState *state, int64_t n_envs,
                                            const Acas2dPolicy *policies, int32_t n_policies, int32_t n_episodes,
                                            const void *obs_in, int32_t n_steps, uint64_t seed, int64_t env_offset,
                                            int32_t n_traffic, uint8_t *outcome, int32_t *steps, void *total_reward,
                                            const Acas2dEvalStats *stats, const Acas2dDisturbance *disturbance,
                                            const Acas2dCorrelation *correlation, void *stream);
int acas2d_evaluate_policies_correlated_group_f32(const Acas2dConfig *cfg, const Acas2dState *state, int64_t n_envs,
                                                  const Acas2dPolicy *policies, int32_t n_policies, int32_t n_episodes,
                                                  const void *obs_in, int32_t n_steps, uint64_t seed, int64_t env_offset,
                                                  int32_t n_traffic, uint8_t *outcome, int32_t *steps, void *total_reward,
                                                  const Acas2dEvalStats *stats, const Acas2dDisturbance *disturbance,
                                                  const Acas2dCorrelation *correlation, void *stream);
int acas2d_monte_carlo_correlated_f32(const Acas2dConfig *cfg, const Acas2dState *state, int64_t n_envs,
                                      const Acas2dPolicy *policies, int32_t n_policies, int32_t n_lanes, const void *obs_in,
                                      int32_t n_steps, uint64_t seed, int64_t env_offset, int32_t n_traffic,
                                      const Acas2dMonteCarlo *mc, const Acas2dDisturbance *disturbance,
                                      const Acas2dCorrelation *correlation, void *stream);
int acas2d_monte_carlo_correlated_group_f32(const Acas2dConfig *cfg, const Acas2dState *state, int64_t n_envs,
                                            const Acas2dPolicy *policies, int32_t n_policies, int32_t n_lanes,
                                            const void *obs_in, int32_t n_steps, uint64_t seed, int64_t env_offset,
                                            int32_t n_traffic, const Acas2dMonteCarlo *mc,
                                            const Acas2dDisturbance *disturbance, const Acas2dCorrelation *correlation,
                                            void *stream);

/*
 * acas2d_evaluate_policies_delayed_f32 / _group_f32, acas2d_monte_carlo_delayed_f32 / _group_f32: the correlated entries
 * above with a RESPONSE between the policy and the aircraft -- a dead time (the pilot's response delay) and a first-order
 * lag (the aircraft's).  Additive to ABI 7, float32 only.  The arguments of the _correlated sibling with `response` in
 * front of `stream`; the same work shapes, the same rejections in the same words.
 *   With a_s the actor's clipped action at a step (a NaN mean passes through), the step flies
 *     c_s = a_{s - delay_steps}                    the action the same lane's actor produced delay_steps steps earlier in the
 *                                                  same episode, played in the same launch; 0.0f while the episode is younger
 *                                                  than that (the aircraft flies straight until the first command arrives);
 *                                                  delay_steps == 0: c_s = a_s, and `ring` is not touched;
 *     u_s = clamp((lag * u_{s-1}) + (g * c_s))     to [-1, 1] by fminf(fmaxf(., -1), 1): two float32 multiplies and a float32
 *                                                  add, each rounded, no fma, with u = 0 in front of the episode's first step
 *                                                  and g = (float)(1.0 - (double)lag) formed on the host; lag == 0: u_s = c_s,
 *                                                  no arithmetic; lag == 1: the aircraft never responds;
 *   and the actuator's error acts on u_s as it acts on the clipped action in the sibling.  An episode's first step is the
 *   sibling's: the lane's first step of the launch, and the first step after an in-step reset.  Sensor noise is untouched.
 *   With delay_steps == 0 and lag == 0 the results equal the _correlated entries' bit for bit.
 *   ring       device float[delay_steps][ring_envs], scratch for the dead time: row steps % delay_steps holds the actions the
 *              envs of the launch (n_policies x n_episodes or n_lanes rounded up to 64) wrote delay_steps steps ago.  Its
 *              contents on entry mean nothing and need no clearing: no row is read before the episode at hand has written
 *              it.  An env's step costs one 4-byte load and one 4-byte store.  Launches that run at the same time need rings
 *              of their own.
 * Rejected with ACAS2D_EINVAL before anything is launched: everything the _correlated sibling rejects, in its words and its
 * order; then a NULL response; delay_steps below 0 or above 32767; a lag that is NaN, negative or above 1; delay_steps > 0
 * with a NULL ring, or with ring_envs below the launch's env count.
 */
typedef struct Acas2dResponse {
    int32_t delay_steps;                   /* dead time between the actor and the aircraft, in steps */
    float lag;                             /* the first-order lag's pole, in [0, 1] */
    float *ring;                           /* device float[delay_steps][ring_envs]; may be NULL when delay_steps == 0 */
    int64_t ring_envs;
} Acas2dResponse;
size_t acas2d_response_size(void);     /* sizeof(Acas2dResponse), for bindings */
int acas2d_evaluate_policies_delayed_f32(const Acas2dConfig *cfg, const Acas2dState *state, int64_t n_envs,
                                         const Acas2dPolicy *policies, int32_t n_policies, int32_t n_episodes,
                                         const void *obs_in, int32_t n_steps, uint64_t seed, int64_t env_offset,
                                         int32_t n_traffic, uint8_t *outcome, int32_t *steps, void *total_reward,
                                         const Acas2dEvalStats *stats, const Acas2dDisturbance *disturbance,
                                         const Acas2dCorrelation *correlation, const Acas2dResponse *response, void *stream);
int acas2d_evaluate_policies_delayed_group_f32(const Acas2dConfig *cfg, const Acas2dState *state, int64_t n_envs,
                                               const Acas2dPolicy *policies, int32_t n_policies, int32_t n_episodes,
                                               const void *obs_in, int32_t n_steps, uint64_t seed, int64_t env_offset,
                                               int32_t n_traffic, uint8_t *outcome, int32_t *steps, void *total_reward,
                                               const Acas2dEvalStats *stats, const Acas2dDisturbance *disturbance,
                                               const Acas2dCorrelation *correlation, const Acas2dResponse *response,
                                               void *stream);
int acas2d_monte_carlo_delayed_f32(const Acas2dConfig *cfg, const Acas2dState *state, int64_t n_envs,
                                   const Acas2dPolicy *policies, int32_t n_policies, int32_t n_lanes, const void *obs_in,
                                   int32_t n_steps, uint64_t seed, int64_t env_offset, int32_t n_traffic,
                                   const Acas2dMonteCarlo *mc, const Acas2dDisturbance *disturbance,
                                   const Acas2dCorrelation *correlation, const Acas2dResponse *response, void *stream);
int acas2d_monte_carlo_delayed_group_f32(const Acas2dConfig *cfg, const Acas2dState *state, int64_t n_envs,
                                         const Acas2dPolicy *policies, int32_t n_policies, int32_t n_lanes,
                                         const void *obs_in, int32_t n_steps, uint64_t seed, int64_t env_offset,
                                         int32_t n_traffic, const Acas2dMonteCarlo *mc,
                                         const Acas2dDisturbance *disturbance, const Acas2dCorrelation *correlation,
                                         const Acas2dResponse *response, void *stream);

/*
 * acas2d_collect_set_disturbed_f32 / acas2d_collect_set_disturbed_group_f32: acas2d_collect_set_f32 / _group_f32 under the
 * sensor noise and actuator disturbance above -- the collector of a PPO iteration that TRAINS under them.  Additive to
 * ABI 7, float32 only.  The siblings' arguments, then `sigmas`, `dist_seed` and `obs_read` in front of `stream`.
 *   sigmas     device float[n_members][4]: member k's (s_sep, s_cpa, s_closing, s_action), Acas2dDisturbance's units.  They
 *              live on the device, so the entry cannot look at them: the CALLER makes sure each is finite and at least 0
 *              (the Python host does).  A member whose four are 0 draws nothing; its columns of every output of the sibling
 *              equal the sibling's bit for bit and its rows of obs_read the true rows.
 *   dist_seed  Acas2dDisturbance.noise_seed, one for all members.
 *   obs_read   T[n_steps + 1][E][D], output: row t is the row BOTH networks read at step t -- the actor and the critic; the
 *              update must be given these rows.  Stored as disturbed (a NaN stays a NaN: the scrub to 0 is the networks').
 *              Row n_steps is the observation the last step left (fresh rows of envs that just reset included) under the
 *              draw the next launch's first step makes, so acas2d_gae_f32 with obs_last = obs_read[n_steps] returns as
 *              last_value_out the bits of the next collection's values[0].  io->obs keeps the TRUE observations.
 * Per step: slot n + 1 on traffic n's three entries in front of the two networks, slot 0 on clip(raw, -1, 1), clipped again.
 * actions keeps the RAW sampled action and logp its log-probability, as in the siblings: actuator noise belongs to the
 * environment, not to the policy's distribution.  Rewards, outcomes and the state follow from the true state.
 * The counter: lane = env_offset + the GLOBAL env index (the index of the sampler's noise stream), episode = the env's own
 * counter in `state` (the in-step reset advances it), step = game.steps before the increment.  The noise is a function of
 * (dist_seed, global env, episode, step, slot) only: not of n_members, of how training is cut into launches, or of the work
 * shape.  The key carries the tag above, so the blocks never meet the sampler's or the reset's.
 * With n_members == 1 the entries are the solo collector: any n_envs >= 1.
 * Rejected with ACAS2D_EINVAL before anything is launched: everything the sibling rejects (but n_members == 1 drops the
 * multiple-of-64 rule), a NULL sigmas or obs_read, obs_read overlapping io->obs or obs_in, max_steps + 1 >= 2^20.
 */
int acas2d_collect_set_disturbed_f32(const Acas2dConfig *cfg, const Acas2dState *state, const Acas2dStepIO *io,
                                     const Acas2dActorCritic *ac, int32_t n_members, const uint64_t *noise_seeds,
                                     const void *obs_in, int32_t n_steps, uint64_t seed, int64_t env_offset, int64_t n_envs,
                                     int32_t n_traffic, const float *sigmas, uint64_t dist_seed, void *obs_read,
                                     void *stream);
int acas2d_collect_set_disturbed_group_f32(const Acas2dConfig *cfg, const Acas2dState *state, const Acas2dStepIO *io,
                                           const Acas2dActorCritic *ac, int32_t n_members, const uint64_t *noise_seeds,
                                           const void *obs_in, int32_t n_steps, uint64_t seed, int64_t env_offset,
                                           int64_t n_envs, int32_t n_traffic, const float *sigmas, uint64_t dist_seed,
                                           void *obs_read, void *stream);

/*
 * acas2d_collect_set_correlated_f32 / acas2d_collect_set_correlated_group_f32: the disturbed collectors above under the
 * time-correlated and biased errors of Acas2dCorrelation -- the collector of a PPO iteration that TRAINS under them.  An
 * episode spans collection launches, so the error state lives in device memory between them.  Additive to ABI 7, float32
 * only.  The disturbed sibling's arguments, then `correlations` and `held` in front of `stream`.
 *   correlations  device float[n_members][8]: member k's rho_sep, rho_cpa, rho_closing, rho_action, then the four gains
 *                 q = (float)sqrt(1 - (double)rho * rho) in the same order.  Like sigmas it lives on the device, so the entry
 *                 cannot look at it: the CALLER makes sure each rho is in [0, 1] and each gain is the one that belongs to it
 *                 (the Python host does).
 *   held          device float[3 * n_traffic + 1][n_envs], in and out: row 3 n + c is traffic n's channel c (sep, cpa,
 *                 closing), row 3 * n_traffic the actuator's, column i env i of THIS launch.  The caller zeroes it once and
 *                 hands the same buffer to every launch on these envs.
 * With z_t the white model's normal of (dist_seed, global env, episode, step, slot), a channel's error is
 *   e_t = z_t                                  where the env's game.steps is 1 before the step's increment: the first step
 *                                              of an episode, after acas2d_reset_* and after an in-step reset alike;
 *   e_t = fadd(fmul(rho, e_{t-1}), fmul(q, z_t))  otherwise, three roundings, no fma, e_{t-1} the value the env held after the
 *                                              previous step it played -- in this launch or an earlier one.
 * A launch boundary is no episode boundary: the errors are a function of (dist_seed, global env, episode, step, slot, rho)
 * only, not of how training is cut into launches, of n_members or of the work shape.  A channel whose rho is 0 takes z_t
 * and leaves its held value alone; so does a channel where nothing is drawn (the member's three sensor sigmas all 0; its
 * action sigma 0).  A member whose four rho are 0 gives the disturbed sibling's outputs bit for bit.  rho == 1 is a
 * constant bias s z_1 per (env, episode, channel, aircraft).  A held value of 0 under steps > 1 -- a state set by hand, a
 * buffer zeroed in mid-episode -- gives e_t = q z_t.
 * obs_read[n_steps] is formed from the held e_{n_steps - 1} WITHOUT committing it: `held` returns as the last played step
 * left it, and the next launch's first step forms the same row again.
 * Rejected with ACAS2D_EINVAL before anything is launched: everything the disturbed sibling rejects, in its words and its
 * order; then a NULL correlations; then a NULL held; then held overlapping obs_read, io->obs or obs_in.
 */
int acas2d_collect_set_correlated_f32(const Acas2dConfig *cfg, const Acas2dState *state, const Acas2dStepIO *io,
                                      const Acas2dActorCritic *ac, int32_t n_members, const uint64_t *noise_seeds,
                                      const void *obs_in, int32_t n_steps, uint64_t seed, int64_t env_offset, int64_t n_envs,
                                      int32_t n_traffic, const float *sigmas, uint64_t dist_seed, void *obs_read,
                                      const float *correlations, float *held, void *stream);
int acas2d_collect_set_correlated_group_f32(const Acas2dConfig *cfg, const Acas2dState *state, const Acas2dStepIO *io,
                                            const Acas2dActorCritic *ac, int32_t n_members, const uint64_t *noise_seeds,
                                            const void *obs_in, int32_t n_steps, uint64_t seed, int64_t env_offset,
                                            int64_t n_envs, int32_t n_traffic, const float *sigmas, uint64_t dist_seed,
                                            void *obs_read, const float *correlations, float *held, void *stream);

/*
 * acas2d_encounter_sample_f32 / _f64, acas2d_encounter_select_f32 / _f64, acas2d_encounter_refit: a cross-entropy search
 * over encounters with importance sampling, around the unchanged acas2d_evaluate_policies_stats_* -- per generation:
 * sample, acas2d_reset_* with do_init = 0 (the first observation), the stats entry, select, refit, with no host decision
 * in between.  Additive to ABI 7.  K = n_policies searches run side by side on the blocks of EP = n_candidates rounded up
 * to 64 envs the stats entry plays; L = n_candidates, N = n_traffic, B = n_bins.
 *
 * An encounter is a point of the unit cube with n_coord = 4 (N + 1) coordinates: coordinate 4 e + j takes the place of
 * u01(word j) of the Philox block of entity e (0 = the player, n + 1 = traffic n) in the reset distribution.  The
 * proposal is one piecewise-constant density per coordinate on B equal bins, p[k][c][b]; coordinates with active[c] == 0
 * (they do not reach the state) keep their uniform, are never refit and add nothing to the likelihood ratio.
 *
 * sample.  Candidate i of block k draws reset's own blocks, counter (lane lo, lane hi, generation, e), key = seed, lane =
 * env_offset + i, and for every active coordinate, with u = u01(word):
 *   b = the largest bin with cdf[b] <= u (cdf[0] = 0, so at most B - 1);  t = (u - cdf[b]) / p[b], below 0 or NaN -> 0,
 *   above 1 - 2^-53 -> 1 - 2^-53;  c = (b + t) / B;  log_w += log_ratio[b]
 * (ascending coordinates, plain float64 adds from 0).  The state is reset's float64 formulas on c, with starts_down =
 * c_x >= 0.5 for traffic 0, rounded to the element type and stored into `state` (own_x .. trf_v, goal, steps = 0,
 * total_reward = 0) at env k EP + i; envs i >= L repeat candidate 0.  bins[k][c][i] is the bin (of an inactive
 * coordinate: min((int)(u B), B - 1)).  With a flat proposal c == u bit for bit: generation g of a float64 search is
 * episode counter g of acas2d_reset_f64.
 *
 * select.  One workgroup per k: score_i = min_sep[k][i] where outcome[k][i] != 0 and the value is not NaN, else +inf;
 * gamma_q = the n_quantile-th smallest score (radix select on the order-preserving integer key); gamma = max(gamma_q,
 * level rounded to the element type); elite: score <= gamma and finite; W_i = exp(log_w[k][i]) if weighted, else 1;
 * elite_w[k][i] = W_i for the elite, else 0.  history[k][0 .. 15], this generation's row of the log: finished,
 * unfinished, n_elite, gamma_q, gamma, n_event = #{score <= level}, the sums of W and W^2 over the event, the sums of W
 * and W^2 over all candidates, the smallest score, its candidate (the lowest index), the generation, three zeros.  The
 * archive: where that smallest score is strictly below best_score[k] (start it at +inf), best_score, best_generation
 * and best_candidate are replaced and the encounter itself, drawn again from this generation's tables, is stored:
 * best_own_psi[k] and best_traffic[k][n] = (x, y, psi, v).
 *
 * refit.  Per active coordinate c and policy k: S[b] = the sum of elite_w[k][i] over the candidates with bins[k][c][i]
 * == b, S_tot = the sum of S[b], ascending b; unless S_tot > 0 nothing changes; else
 *   p_new[b] = max((1 - alpha) p[b] + alpha (S[b] / S_tot), p_floor);  p[b] = p_new[b] / (the sum of p_new, ascending b)
 *   cdf[0] = 0, cdf[b + 1] = cdf[b] + p[b];  log_ratio[b] = -log(B p[b])
 * All sums over candidates are taken in one fixed order (thread-strided ascending, a fixed tree in the wave, the waves in
 * order) without floating atomics: the same inputs give the same bits.
 *
 * Rejected with ACAS2D_EINVAL before anything is launched: a NULL cfg, state (sample) or search, a NULL buffer of either;
 * n_bins not a power of two in 2 .. 64; n_coord != 4 (n_traffic + 1) (refit: not a multiple of 4 from 8 up); n_quantile
 * outside 1 .. n_candidates; alpha outside [0, 1]; p_floor outside [0, 1 / n_bins); generation >= 2^32; a NaN level;
 * n_candidates < 1; n_policies outside 1 .. 65535; a negative env_offset; a state of fewer than n_policies x EP envs.
 */
#define ACAS2D_SEARCH_HISTORY_WIDTH 16
typedef struct Acas2dEncounterSearch {
    double *p, *cdf, *log_ratio;     /* double[K][n_coord][B], [K][n_coord][B + 1], [K][n_coord][B] */
    const uint8_t *active;           /* u8[n_coord] */
    uint8_t *bins;                   /* u8[K][n_coord][L] */
    double *log_w, *elite_w;         /* double[K][L] */
    const uint8_t *outcome;          /* u8[K][L]: the stats entry's outcome */
    const void *min_sep;             /* T[K][L]: the stats entry's Acas2dEvalStats.min_sep */
    double *history;                 /* double[K][ACAS2D_SEARCH_HISTORY_WIDTH]: this generation's row */
    void *best_score;                /* T[K] */
    uint32_t *best_generation;       /* u32[K] */
    int32_t *best_candidate;         /* int32[K] */
    void *best_own_psi, *best_traffic;   /* T[K], T[K][N][4] */
    int32_t n_bins, n_coord, n_quantile, weighted;
    double alpha, p_floor, level;
    uint64_t generation;
} Acas2dEncounterSearch;
size_t acas2d_encounter_search_size(void);  /* sizeof(Acas2dEncounterSearch), for bindings */
int acas2d_encounter_sample_f32(const Acas2dConfig *cfg, const Acas2dState *state, int64_t n_envs, int32_t n_policies,
                                int32_t n_candidates, uint64_t seed, int64_t env_offset, int32_t n_traffic,
                                const Acas2dEncounterSearch *search, void *stream);
int acas2d_encounter_sample_f64(const Acas2dConfig *cfg, const Acas2dState *state, int64_t n_envs, int32_t n_policies,
                                int32_t n_candidates, uint64_t seed, int64_t env_offset, int32_t n_traffic,
                                const Acas2dEncounterSearch *search, void *stream);
int acas2d_encounter_select_f32(const Acas2dConfig *cfg, int32_t n_policies, int32_t n_candidates, uint64_t seed,
                                int64_t env_offset, int32_t n_traffic, const Acas2dEncounterSearch *search, void *stream);
int acas2d_encounter_select_f64(const Acas2dConfig *cfg, int32_t n_policies, int32_t n_candidates, uint64_t seed,
                                int64_t env_offset, int32_t n_traffic, const Acas2dEncounterSearch *search, void *stream);
int acas2d_encounter_refit(const Acas2dEncounterSearch *search, int32_t n_policies, int32_t n_candidates, void *stream);

/*
 * acas2d_collect_set_group_f32: acas2d_collect_set_f32 for n_traffic in {8, 16, 32, 64}, float32 -- the same arguments,
 * layouts and outputs.  Additive to ABI 7.  The launch is acas2d_collect_group_f32's (the env's G lanes of the packed work
 * shapes (4,2) (4,4) (4,8) (4,16) evaluate the two networks together) with the member found per wavefront: a wavefront
 * holds 64 / G envs, and the rule n_envs = K x a multiple of 64 is kept as it stands (64 / G would do for this kernel;
 * acas2d_gae_f32 and the trainers need 64 for K > 1, and one rule is easier to state).
 * The columns of member k equal acas2d_collect_group_f32 run alone on those envs -- policy k, noise_seed = noise_seeds[k],
 * env_offset + k EM, the same env seed -- bit for bit; at n_traffic = 8 they also equal acas2d_collect_set_f32's.
 * The stacks w1t, b1, w2t, b2, v1t, vb1, v2t, vb2 must be 16-byte aligned (a member's slice then is: the member strides are
 * multiples of 256 bytes).  Rejected with ACAS2D_EINVAL before anything is launched: what the sibling rejects, a misaligned
 * stack, and any n_traffic outside the four (n_traffic in {1, 2, 3, 4} belongs to acas2d_collect_set_f32).  There is no
 * float64 variant.
 */
int acas2d_collect_set_group_f32(const Acas2dConfig *cfg, const Acas2dState *state, const Acas2dStepIO *io,
                                 const Acas2dActorCritic *ac, int32_t n_members, const uint64_t *noise_seeds,
                                 const void *obs_in, int32_t n_steps, uint64_t seed, int64_t env_offset, int64_t n_envs,
                                 int32_t n_traffic, void *stream);

/*
 * acas2d_ppo_update_f32:ONE minibatch update of SB3 1.1.0's PPO.train() for the MlpPolicy actor-critic (the update
 * half of `PPO('MlpPolicy', env).learn()`, training_main.py:44-52) as two launches: forward + PPO loss + backward of
 * both 2 x 64 tanh networks on the rows idx[0 .. n_rows) of the rollout buffer (advantages normalised over the
 * minibatch, clipped surrogate, MSE value loss without clipping, entropy of the state-independent Gaussian), then
 * clip_grad_norm_ + Adam on the 13 parameter tensors IN PLACE.  Parameters in torch's own layouts ([out][in]), all
 * float32.  grad / adam_m / adam_v: acas2d_ppo_workspace_floats(obs_dim) floats each, zero before the first call
 * (grad is left zero by every call); adam_step: int32[1], 0 before the first call; stats: float[8], zero before
 * the first call -- [2] gradient norm, [4] policy loss, [5] value loss of the last minibatch.
 * obs_dim in {8, 11, 14, 17, 29} (n_traffic 1, 2, 3, 4, 8).  max_grad_norm < 0 (tests): only the gradient is
 * computed and left in `grad` (actor w1 b1 w2 b2 w3 b3, critic likewise, log_std), nothing is applied.
 * Run-to-run: the per-wave partial gradients are added to `grad` with float atomics, whose order is not fixed, so two
 * runs of the same update agree to float32 rounding of the sums (~1e-7 relative), not bit for bit -- unlike the env
 * kernels, which are bitwise deterministic.  The gradient kernel uses 70 - 75 KB of LDS per workgroup (gfx950 has 160 KB;
 * checked against each device at its first call, ACAS2D_EINVAL where it does not fit).
 */
typedef struct Acas2dPpoUpdate {
    void *actor_w1, *actor_b1, *actor_w2, *actor_b2, *actor_w3, *actor_b3;       /* mlp_extractor.policy_net.{0,2}, action_net */
    void *critic_w1, *critic_b1, *critic_w2, *critic_b2, *critic_w3, *critic_b3; /* mlp_extractor.value_net.{0,2}, value_net  */
    void *log_std;
    const void *obs;                 /* float[n][obs_dim]: the rollout buffer, flat */
    const void *act, *old_logp, *adv, *ret;   /* float[n] */
    const int64_t *idx;              /* int64[n_rows]: the minibatch */
    int32_t n_rows, obs_dim;
    float clip_range, vf_coef, ent_coef, max_grad_norm;
    float learning_rate, beta1, beta2, adam_eps;
    void *grad, *adam_m, *adam_v;
    int32_t *adam_step;
    void *stats;
} Acas2dPpoUpdate;

int acas2d_ppo_workspace_floats(int32_t obs_dim);
int acas2d_ppo_update_f32(const Acas2dPpoUpdate *u, void *stream);

/*
 * acas2d_ppo_update_wide_f32: acas2d_ppo_update_f32 for obs_dim in {53, 101, 197} (n_traffic 16, 32, 64), float32.
 * Additive to ABI 7.  The same struct, the same semantics (SB3 1.1.0's PPO.train() minibatch, advantages normalised over
 * the rows idx[0 .. n_rows), clip_grad_norm_ + Adam on the 13 parameter tensors IN PLACE), the same flat layout of
 * grad / adam_m / adam_v (acas2d_ppo_workspace_floats(obs_dim) floats each: actor w1 b1 w2 b2 w3 b3, critic likewise,
 * log_std; zero before the first call, grad left zero by every call), adam_step int32[1], stats float[8] ([2] gradient
 * norm, [4] policy loss, [5] value loss of the last minibatch), and the same probe mode: max_grad_norm < 0 leaves the raw
 * gradient in `grad` and applies nothing.  Every pointer is required and n_rows >= 2; any other obs_dim is rejected
 * (ACAS2D_EINVAL; {8, 11, 14, 17, 29} belong to the sibling), before anything is launched.
 * The gradient launch runs four waves per 64 samples and network, each wave a quarter of the hidden units, and tiles the
 * obs_dim-sized operands through LDS; no observation column >= obs_dim of any row is read.  The apply launch is the
 * sibling's.  Run-to-run: as for the sibling, the per-workgroup partial gradients are added to `grad` with float
 * atomics, whose order is not fixed, so two runs of the same update agree to float32 rounding of the sums (~1e-7
 * relative), not bit for bit.  The gradient kernel asks for acas2d_ppo_wide_lds_bytes(obs_dim) bytes of LDS per workgroup
 * (79 / 91 / 115 KB; gfx950 has 160 KB), checked against each device at its first call (ACAS2D_EINVAL where it does not
 * fit).  acas2d_ppo_wide_lds_bytes answers ACAS2D_EINVAL for an obs_dim outside the three.
 */
int acas2d_ppo_update_wide_f32(const Acas2dPpoUpdate *u, void *stream);
int acas2d_ppo_wide_lds_bytes(int32_t obs_dim);

/*
 * acas2d_ppo_update_set_f32: acas2d_ppo_update_f32 for K independent learners ("members") in TWO launches, whatever K
 * is.  Additive to ABI 7.  Every parameter pointer names a [K][...] stack of the sibling's tensor (torch layouts);
 * grad / adam_m / adam_v are float[K][acas2d_ppo_workspace_floats(obs_dim)], adam_step int32[K], stats float[K][8] (slots
 * as the sibling's), all zero before the first call.  The rollout buffer is ONE flat buffer shared by all members --
 * obs float[n_total][obs_dim], act / old_logp / adv / ret float[n_total] -- and idx int64[K][n_rows] holds member k's
 * minibatch as rows of that buffer, so the [T][K * EM] output of acas2d_collect_set_f32 feeds the update as it lies.
 * hyper is a DEVICE float[K][8]: clip_range, vf_coef, ent_coef, max_grad_norm, learning_rate, beta1, beta2, adam_eps of
 * member k, read by the kernels (the caller may rewrite it between calls).  apply == 0 (tests): only the gradients are
 * computed and left in grad[k]; nothing is applied and adam_step is untouched.
 * The gradient launch has the grid (ceil(n_rows / 64), 2, K) and runs the sibling's arithmetic per member; the apply
 * launch has one 1 024-thread workgroup per member.  Run-to-run: as for the sibling, the per-wave partial gradients are
 * added to grad[k] with float atomics, whose order is not fixed, so two runs agree to float32 rounding of the sums (~1e-7
 * relative), not bit for bit.  LDS as the sibling's (70 - 75 KB per gradient workgroup), checked against each device at
 * its first call.  Every pointer is required, n_members in [1, 65535], n_rows >= 2, obs_dim in {8, 11, 14, 17, 29}
 * (n_traffic 1, 2, 3, 4, 8); anything else is ACAS2D_EINVAL before a launch (the wide widths 53, 101, 197 are
 * acas2d_ppo_update_wide_set_f32, below).  Out of scope: float64, members with different n_rows.
 */
typedef struct Acas2dPpoUpdateSet {
    void *actor_w1, *actor_b1, *actor_w2, *actor_b2, *actor_w3, *actor_b3;       /* [K][...] stacks */
    void *critic_w1, *critic_b1, *critic_w2, *critic_b2, *critic_w3, *critic_b3;
    void *log_std;                      /* float[K] */
    const void *obs;                    /* float[n_total][obs_dim]: ONE shared flat rollout buffer */
    const void *act, *old_logp, *adv, *ret;   /* float[n_total] */
    const int64_t *idx;                 /* int64[K][n_rows]: member k's minibatch, rows of the shared buffer */
    int32_t n_members, n_rows, obs_dim, apply;  /* apply == 0: raw gradients only */
    const void *hyper;                  /* device float[K][8] */
    void *grad, *adam_m, *adam_v;       /* float[K][acas2d_ppo_workspace_floats(obs_dim)] */
    int32_t *adam_step;                 /* int32[K] */
    void *stats;                        /* float[K][8] */
} Acas2dPpoUpdateSet;

int acas2d_ppo_update_set_f32(const Acas2dPpoUpdateSet *u, void *stream);

/*
 * acas2d_ppo_update_wide_set_f32: acas2d_ppo_update_set_f32 for obs_dim in {53, 101, 197} (n_traffic 16, 32, 64), float32.
 * Additive to ABI 7.  The same struct and the same layouts: [K][...] parameter stacks in torch layouts, grad / adam_m /
 * adam_v float[K][acas2d_ppo_workspace_floats(obs_dim)], adam_step int32[K], stats float[K][8], hyper DEVICE float[K][8],
 * ONE flat rollout buffer shared by all members with idx int64[K][n_rows] naming member k's rows of it, apply == 0 for the
 * raw gradients.  The gradient launch has the grid (ceil(n_rows / 64), 2, K) with 256 threads and runs
 * acas2d_ppo_update_wide_f32's arithmetic per member (four waves per 64 samples and network); the apply launch is
 * acas2d_ppo_update_set_f32's, one 1 024-thread workgroup per member.  With one workgroup per network (n_rows <= 64) every
 * gradient entry receives one atomic add, and member k's result equals acas2d_ppo_update_wide_f32 on that member bit for bit.
 * Run-to-run: otherwise, as for the siblings, the per-workgroup partial gradients are added to grad[k] with float atomics,
 * whose order is not fixed, so two runs agree to float32 rounding of the sums (~1e-7 relative), not bit for bit.  The
 * gradient kernel asks for acas2d_ppo_wide_lds_bytes(obs_dim) bytes of LDS per workgroup (79 / 91 / 115 KB; gfx950 has
 * 160 KB), checked against each device at its first call (ACAS2D_EINVAL where it does not fit).
 * Every pointer is required, n_members in [1, 65535], n_rows >= 2; any other obs_dim is ACAS2D_EINVAL before a launch
 * ({8, 11, 14, 17, 29} belong to acas2d_ppo_update_set_f32, and the message says so).  Out of scope: float64, members with
 * different n_rows.
 */
int acas2d_ppo_update_wide_set_f32(const Acas2dPpoUpdateSet *u, void *stream);

/*
 * acas2d_ppo_update_guarded_set_f32: acas2d_ppo_update_set_f32 / acas2d_ppo_update_wide_set_f32 with SB3 1.1.0's target_kl
 * early stop and its train/approx_kl and train/clip_fraction, decided on the device.  Additive to ABI 7.  float32.
 * ONE entry for obs_dim in {8, 11, 14, 17, 29, 53, 101, 197}; `u` is the siblings' struct with the siblings' layouts, K =
 * 1 serves a single learner (its tensors are K = 1 stacks).  The same two launches, no read-back:
 *   gradient launch   the sibling's arithmetic; each live row of an actor workgroup also adds (ratio - 1) - log(ratio)
 *                     to diag[k][0] and (|ratio - 1| > clip_range ? 1 : 0) to diag[k][1], ratio being the one the
 *                     clipped surrogate is formed from.  A member with stopped[k] != 0 does nothing.
 *   apply launch      a member with stopped[k] != 0 does nothing.  Otherwise kl = diag[k][0] / n_rows and cf =
 *                     diag[k][1] / n_rows (SB3's approx_kl and clip_fraction of this minibatch), and
 *                       diag[k][2] = kl, diag[k][3] = cf              the last minibatch's
 *                       diag[k][4] += kl, diag[k][5] += cf, diag[k][6] += 1   sums and count over the update
 *                       diag[k][0] = diag[k][1] = 0
 *                     then, if target_kl[k] > 0 and kl > 1.5f * target_kl[k], the member STOPS: stopped[k] = 1, stats[k][0]
 *                     and [1] move to stats[k][4] and [5] (SB3 logs the stopping minibatch's losses), grad[k] is zeroed,
 *                     and nothing is applied -- the parameters, adam_m, adam_v, adam_step[k] and stats[k][2] stay as they
 *                     were, the entropy term is not added.  Otherwise the sibling's apply, and diag[k][7] += 1.
 * The caller zeroes `stopped` and `diag` where SB3 enters train() and keeps calling for every minibatch of the update;
 * afterwards diag[k][4] / diag[k][6] is SB3's train/approx_kl, diag[k][5] / diag[k][6] its train/clip_fraction and
 * diag[k][7] the number of minibatches applied (SB3 appends the stopping minibatch to both lists before it breaks, so it
 * counts in [4], [5], [6] and not in [7]).  target_kl[k] <= 0: no limit for member k, only the statistics.
 * With the limit off the parameters, moments and step counts are the siblings': bit for bit where n_rows <= 64 (one atomic
 * add per gradient entry), to the siblings' run-to-run rounding otherwise.  LDS as the siblings', checked against each
 * device at its first call.  ACAS2D_EINVAL before any launch: what the siblings reject, a NULL `g` or a NULL pointer in it,
 * an obs_dim outside the eight, and apply == 0 (the probe mode has no decision to make: the raw gradients are the
 * unguarded entries').  Out of scope: float64, members with different n_rows.
 */
typedef struct Acas2dPpoGuard {
    const void *target_kl;              /* device float[K]; <= 0: no limit */
    int32_t *stopped;                   /* device int32[K]; the caller zeroes it where SB3 enters train() */
    void *diag;                         /* device float[K][8], slots as above; zeroed with `stopped` */
} Acas2dPpoGuard;

int acas2d_ppo_update_guarded_set_f32(const Acas2dPpoUpdateSet *u, const Acas2dPpoGuard *g, void *stream);
size_t acas2d_ppo_guard_size(void);     /* sizeof(Acas2dPpoGuard): layout check for bindings */

/*
 * acas2d_ppo_update_sb3_set_f32: acas2d_ppo_update_guarded_set_f32 with the rest of SB3 1.1.0's PPO.__init__ -- clip_range_vf
 * (the value-function clipping) and per-update factors on learning_rate, clip_range and clip_range_vf, which is what a
 * schedule of progress_remaining evaluates to.  Additive to ABI 7.  float32.  ONE entry for obs_dim in {8, 11, 14, 17, 29,
 * 53, 101, 197}; `u` and `g` are the sibling's structs with the sibling's layouts and meaning (target_kl[k] <= 0: only the
 * statistics), K = 1 serves a single learner.  The same two launches, no read-back:
 *   gradient launch   a member with stopped[k] != 0 does nothing.  An actor workgroup uses clip_range = hyper[k][0] *
 *                     scale[k][1], ONE float32 product, for the clipped surrogate and for diag[k][1]'s clipped count
 *                     alike.  A critic workgroup forms c = clip_range_vf[k] * scale[k][2], one float32 product; if c > 0 a
 *                     live row s with critic output `out` takes SB3's clipped value loss,
 *                       d = out - old_val[s];  vp = old_val[s] + fminf(fmaxf(d, -c), c);  e = vp - ret[s]
 *                       value loss += e * e / n_rows;  d loss / d out = (-c <= d && d <= c) ? vf_coef * 2 e / n_rows : 0
 *                     (values_pred = old_values + clamp(values - old_values, -c, c), F.mse_loss(returns, values_pred): no
 *                     max with the unclipped loss, and torch's clamp passes the gradient on the closed interval).
 *                     Otherwise (c <= 0 or NaN) the row takes the sibling's plain MSE branch and old_val is NOT READ for
 *                     member k.
 *   apply launch      the sibling's statistics, stop decision and stats moves, then the sibling's apply with learning
 *                     rate hyper[k][4] * scale[k][0], one float32 product.
 * The factors multiply whatever hyper[k] holds when the kernels run, so they compose with acas2d_population_exploit_f32
 * rewriting those rows on the device.  The caller writes scale (and zeroes `stopped` / `diag`) where SB3 enters train().
 * Neutral options: scale rows of ones and clip_range_vf of zeros give acas2d_ppo_update_guarded_set_f32's parameters,
 * adam_m, adam_v, adam_step, stats and diag -- bit for bit where n_rows <= 64 (x * 1.0f is exact, one atomic add per
 * gradient entry), to the siblings' run-to-run rounding otherwise.  LDS as the siblings'.
 * ACAS2D_EINVAL before any HIP call: what the guarded entry rejects, a NULL `o`, and a NULL pointer in `o` (the message
 * names the field).  Out of scope: float64, members with different n_rows.
 */
typedef struct Acas2dPpoOptions {
    const void *old_val;                /* float[n_total]: the rollout's values, rows as obs / act / ... */
    const void *clip_range_vf;          /* device float[K]; <= 0: plain MSE for member k, old_val not read */
    const void *scale;                  /* device float[K][4]: factors on learning_rate, clip_range, clip_range_vf of
                                           this update; [3] reserved, not read */
} Acas2dPpoOptions;

int acas2d_ppo_update_sb3_set_f32(const Acas2dPpoUpdateSet *u, const Acas2dPpoGuard *g, const Acas2dPpoOptions *o,
                                  void *stream);
size_t acas2d_ppo_options_size(void);   /* sizeof(Acas2dPpoOptions): layout check for bindings */

/*
 * acas2d_gae_f32: what lies between acas2d_collect_* and acas2d_ppo_update_* in a PPO iteration, in ONE launch -- the
 * critic's value of the last observation (optional) and SB3 1.1.0's RolloutBuffer.compute_returns_and_advantage (GAE)
 * over the collector's [T][E] buffers (`PPO.learn()`, training_main.py:44-52).  Additive to ABI 7.  float32.
 * One lane per env sweeps t = T-1 ... 0; per (t, e), every operation its own float32 rounding, in this order:
 *     r     = reward[t][e], NaN -> 0, +inf -> FLT_MAX, -inf -> -FLT_MAX          (torch.nan_to_num(x, nan=0.0))
 *     nt    = done[t][e] ? 0.0f : 1.0f
 *     nv    = (t == T-1) ? last_value[e] : value[t+1][e]
 *     delta = ((r + ((gamma_k * nv) * nt)) - value[t][e])
 *     last  = delta + ((gl_k * nt) * last)                                       last starts at 0
 *     adv[t][e] = last;  ret[t][e] = last + value[t][e]
 * which is the sequence of torch operations of the Python host's compute_gae(): the outputs are equal to its bit for bit.
 * The sweep keeps acas2d_gae_pipeline_depth() rows of loads in flight below the row it computes on.
 *   gamma, gamma_lambda   DEVICE float[K]: member k's gamma_k and gl_k.  The CALLER forms gl_k, so both conventions exist:
 *                         (float)(gamma * lambda) with the product taken in double (scalar hyper-parameters), or
 *                         (float)gamma * (float)lambda rounded in float32 (float32 tensors of hyper-parameters)
 *   n_members             K >= 1: member k owns the envs [k EM, (k + 1) EM), EM = n_envs / K -- for K > 1 a multiple of 64,
 *                         so that a wavefront's envs belong to one member and its constants and critic stay scalar
 *                         operands, as for acas2d_collect_set_f32; K == 1 takes any n_envs >= 1 (< 2^31)
 *   last_value            float[E], or NULL: the kernel then evaluates the critic on obs_last float[E][obs_dim] itself, with
 *                         the value-net stacks v1t .. vb3 in Acas2dActorCritic's layout ([K][D][64], [K][64], [K][64][64],
 *                         [K][64], [K][64], [K][1]).  A non-finite observation entry is fed as 0, and the arithmetic is the
 *                         collector's, so the value has the bits `values` of a collection started on that observation
 *                         holds.  The in-kernel critic exists for obs_dim in {8, 11, 14, 17, 29} (n_traffic 1, 2, 3, 4, 8)
 *                         only: the wide widths (53, 101, 197) must pass last_value.  obs_dim and v1t .. vb3 are ignored
 *                         when last_value is given
 *   last_value_out        optional float[E]: the bootstrap value used
 *   nan_count             optional int32[K]: the number of NaN rewards of member k is ADDED to nan_count[k] (one integer
 *                         atomic per wavefront that saw one; zero it before the call)
 * Rejected with ACAS2D_EINVAL before any HIP call: a NULL reward, value, done, adv, ret, gamma or gamma_lambda; n_steps,
 * n_envs or n_members < 1; K > 1 with n_envs not K x a multiple of 64; last_value and obs_last both NULL; without
 * last_value an obs_dim outside the five or a NULL critic stack; adv or ret equal to any other buffer of the struct or to
 * each other.
 */
typedef struct Acas2dGae {
    const void *reward, *value;      /* float[n_steps][n_envs]: the collector's reward / values */
    const uint8_t *done;             /* u8[n_steps][n_envs] */
    const void *last_value;          /* float[n_envs] or NULL */
    const void *obs_last;            /* float[n_envs][obs_dim]; read only when last_value is NULL */
    const void *v1t, *vb1;           /* the critic, as Acas2dActorCritic's: read only when last_value is NULL */
    const void *v2t, *vb2;
    const void *v3, *vb3;
    const void *gamma, *gamma_lambda;   /* device float[n_members] */
    void *adv, *ret;                 /* float[n_steps][n_envs] outputs */
    void *last_value_out;            /* float[n_envs] or NULL */
    int32_t *nan_count;              /* int32[n_members] or NULL */
    int64_t n_envs;
    int32_t n_steps, n_members, obs_dim, _pad;
} Acas2dGae;

int acas2d_gae_f32(const Acas2dGae *g, void *stream);
size_t acas2d_gae_size(void);         /* sizeof(Acas2dGae): layout check for bindings */
int acas2d_gae_pipeline_depth(void);  /* rows of loads in flight per lane (16) */

/*
 * acas2d_reward_normalize_f32: SB3 1.1.0's VecNormalize(norm_obs=False, norm_reward=True) over the collector's [T][E]
 * reward buffer, between acas2d_collect_* and acas2d_gae_f32 -- every reward divided by the running standard deviation of
 * the discounted return (VecNormalize.step_wait + RunningMeanStd.update_from_moments).  Additive to ABI 7.  float32 rewards;
 * the state and all arithmetic are float64, every operation its own rounding.
 * State: per member k `stats[k]` = mean, var, count (start it at 0, 1, 1e-4); per env e the discounted return
 * `returns[e]` = G_e (start it at 0).  Member k owns the envs [k EM, (k + 1) EM), EM = n_envs / K.  For t = 0 .. T-1, in
 * this order:
 *     r       = reward[t][e], NaN -> 0, +-inf -> +-FLT_MAX (acas2d_gae_f32's scrub), widened to double
 *     G_e     = G_e * gamma_k + r
 *     bm      = sum_e(G_e) / EM;  bv = sum_e((G_e - bm)^2) / EM                    two passes over member k's envs
 *     delta   = bm - mean;  tot = count + EM
 *     mean'   = mean + delta * EM / tot
 *     m2      = var * count + bv * EM + delta * delta * count * EM / tot
 *     var     = m2 / tot;  mean = mean';  count = tot
 *     out[t][e] = (float)min(max(r / sqrt(var + epsilon), -clip), clip)            double division, one rounding to float32
 *     if done[t][e]: G_e = 0
 * The two sums over e are taken in a fixed order that depends on EM alone (lane l of one wavefront adds the columns l,
 * l + 64, ... ascending, the wavefront adds along the xor tree 32 .. 1); there are no floating-point atomics and the merges
 * over t are sequential.  So the same inputs give the same bits on every run; a call over T rows equals a call over the
 * first T1 rows followed by one over the rest (the state carries everything), bit for bit in out, returns and stats; and a
 * call with K members equals K calls with K = 1 on the column slices.
 * The call is four launches on `stream` (per-env sweep, per-row moments, per-member merges, element-wise division) with no
 * host synchronisation and no read-back; the sweep keeps acas2d_reward_norm_pipeline_depth() rows of loads in flight.
 *   reward, done          the collector's float[T][E] / u8[T][E]
 *   out                   float[T][E]; out == reward is allowed (in place: the same element by the same lane)
 *   returns               DEVICE double[E], read and written
 *   stats                 DEVICE double[K][3], read and written
 *   gamma                 DEVICE double[K]: member k's discount
 *   workspace             DEVICE scratch of acas2d_reward_norm_workspace_bytes(n_envs, n_steps, n_members) bytes (8 per
 *                         sample and 24 per (t, k)), 8-byte aligned; holds nothing between calls
 *   epsilon, clip         SB3's defaults are 1e-8 and 10
 *   n_members             K >= 1; for K > 1, EM must be a multiple of 64 (a wavefront's envs belong to one member, as for
 *                         acas2d_gae_f32); K == 1 takes any n_envs >= 1 (< 2^31)
 * Rejected with ACAS2D_EINVAL before any HIP call: a NULL pointer; n_steps, n_envs or n_members < 1; n_envs >= 2^31; K > 1
 * with n_envs not K x a multiple of 64; epsilon or clip not finite and positive; out, returns, stats or workspace equal to
 * another buffer of the struct, other than out == reward; returns, stats, gamma or workspace not 8-byte aligned.
 */
typedef struct Acas2dRewardNorm {
    const void *reward;              /* float[n_steps][n_envs]: the collector's reward */
    const uint8_t *done;             /* u8[n_steps][n_envs] */
    void *out;                       /* float[n_steps][n_envs]; may be `reward` */
    double *returns;                 /* device double[n_envs]: read and written */
    double *stats;                   /* device double[n_members][3]: mean, var, count; read and written */
    const double *gamma;             /* device double[n_members] */
    void *workspace;                 /* acas2d_reward_norm_workspace_bytes() of device scratch */
    double epsilon, clip;
    int64_t n_envs;
    int32_t n_steps, n_members;
} Acas2dRewardNorm;

int acas2d_reward_normalize_f32(const Acas2dRewardNorm *n, void *stream);
size_t acas2d_reward_norm_size(void);             /* sizeof(Acas2dRewardNorm): layout check for bindings */
/* bytes of `workspace` for a call of this shape; 0 for a shape the entry rejects */
size_t acas2d_reward_norm_workspace_bytes(int64_t n_envs, int32_t n_steps, int32_t n_members);
int acas2d_reward_norm_pipeline_depth(void);      /* rows of loads in flight per lane of the sweep (16) */

/*
 * acas2d_member_episodes_f32: the episodes that ended during a collection of K members, summed per member in ONE launch
 * -- the score of population-based training (Jaderberg et al. 2017).  Additive to ABI 7.  Inputs are the [T][E] outputs of
 * acas2d_collect_* as they lie, member k owning the columns [k EM, (k + 1) EM), EM = n_envs / K.  ep_return and ep_steps
 * are defined only where done != 0; whatever lies at the other positions (NaN, inf, INT32_MIN) reaches no result.
 * The launch ADDS to the accumulators (device memory; zero them to start a new window):
 *   ep_count       int64[K]      episodes ended
 *   ep_outcomes    int64[K][4]   of these, by outcome code 0 .. 3
 *   ep_steps_sum   int64[K]      the sum of ep_steps - 1 (ep_steps counts step() calls + 1)
 *   ep_return_sum  double[K]     the sum of the float returns, each widened to double and added as it is (a NaN return
 *                                at a done position propagates, to that member's sum only)
 * and OVERWRITES score float[K] = (float)(ep_return_sum[k] / ep_count[k]) from the totals after adding: the mean return of
 * the window, NaN where no episode has ended.
 * One 1 024-thread workgroup per member adds in a fixed order (in the lane, in the wave, across the waves) without
 * atomics: the same inputs and shapes give the same bits on every run.
 * Rejected with ACAS2D_EINVAL before any HIP call: a NULL pointer; n_steps or n_envs < 1; n_members outside [1, 65535];
 * K > 1 with n_envs not K x a multiple of 64 (K == 1 takes any n_envs >= 1); n_envs >= 2^31.
 */
typedef struct Acas2dMemberEpisodes {
    const uint8_t *done, *outcome;   /* u8[n_steps][n_envs] */
    const void *ep_return;           /* float[n_steps][n_envs] */
    const int32_t *ep_steps;         /* int32[n_steps][n_envs] */
    int64_t *ep_count, *ep_outcomes, *ep_steps_sum;   /* int64[K], int64[K][4], int64[K]: added to */
    double *ep_return_sum;           /* double[K]: added to */
    void *score;                     /* float[K]: overwritten */
    int64_t n_envs;
    int32_t n_steps, n_members;
} Acas2dMemberEpisodes;

int acas2d_member_episodes_f32(const Acas2dMemberEpisodes *m, void *stream);
size_t acas2d_member_episodes_size(void);     /* sizeof(Acas2dMemberEpisodes): layout check for bindings */

/*
 * acas2d_population_exploit_f32: the exploit / explore step of population-based training for the K stacked learners of
 * acas2d_ppo_update_set_f32 / acas2d_ppo_update_wide_set_f32, in ONE launch with no host decision: truncation selection on
 * `score`, a bit copy of a better member into each of the worst, and the perturbation of the copied hyper row.  Additive
 * to ABI 7.  The layouts are Acas2dPpoUpdateSet's at every width: obs_dim in {8, 11, 14, 17, 29, 53, 101, 197}.
 * With K = n_members and R = n_replace (0 <= 2R <= K):
 *   key_j   = -inf where score[j] is NaN, else score[j]
 *   rank_k  = #{j : key_j > key_k} + #{j < k : key_j == key_k}       (a total order: ties go to the smaller index, +0 == -0)
 *   member k is a recipient iff rank_k >= K - R; every other member gets donor[k] = k and is not touched
 *   w       = the seven-round philox4x32 of the reset stream on counter (k, generation, 0, 0x70627431), key (seed lo, seed hi)
 *   d       = the member with rank_d == (uint64(w.x) * R) >> 32                         (one of the R best, uniformly)
 *   if not key_d > key_k: donor[k] = k and nothing of member k changes                  (a NaN score never donates)
 *   else    the 13 parameter tensors, adam_m[k], adam_v[k] and adam_step[k] become member d's, bit for bit;
 *           hyper[k][s] = hyper[d][s], and where bit s of perturb_mask is set instead
 *           fminf(fmaxf(hyper[d][s] * f, lo[s]), hi[s]) with f = ((w.y >> s) & 1) ? factor_hi : factor_lo (one float32
 *           multiplication; slots in the order of the hyper row: clip_range, vf_coef, ent_coef, max_grad_norm,
 *           learning_rate, beta1, beta2, adam_eps; bits 8 .. 31 are ignored); donor[k] = d
 * grad and stats of the update are not touched.  Donors are only read and a recipient is written by its own workgroups
 * only, so the launch (grid 16 x K, every workgroup ranking the K scores in LDS) is race-free in place.  A member's row
 * of adam_m / adam_v is an odd number of floats: rows are copied as 16-byte words where source and destination allow,
 * as dwords otherwise, and nothing beyond 4-byte alignment is assumed.
 * Rejected with ACAS2D_EINVAL before any HIP call: a NULL pointer; obs_dim outside the eight widths; n_members outside
 * [1, 1024]; n_replace < 0 or 2 x n_replace > n_members; a factor that is not finite and positive; lo[s] > hi[s] (or a
 * NaN bound) on a slot of perturb_mask; donor or score equal to another buffer of the struct.  n_replace == 0 launches
 * and writes donor[k] = k only.
 */
typedef struct Acas2dPopulationExploit {
    void *actor_w1, *actor_b1, *actor_w2, *actor_b2, *actor_w3, *actor_b3;       /* [K][...] stacks, as Acas2dPpoUpdateSet's */
    void *critic_w1, *critic_b1, *critic_w2, *critic_b2, *critic_w3, *critic_b3;
    void *log_std;                      /* float[K] */
    void *adam_m, *adam_v;              /* float[K][acas2d_ppo_workspace_floats(obs_dim)] */
    int32_t *adam_step;                 /* int32[K] */
    void *hyper;                        /* device float[K][8] */
    const void *score;                  /* float[K]: greater is better, NaN is worst */
    int32_t *donor;                     /* int32[K] output: whom member k was copied from, k where it was not */
    int32_t n_members, obs_dim, n_replace;
    uint32_t generation;
    uint64_t seed;
    uint32_t perturb_mask;
    float factor_lo, factor_hi;
    float lo[8], hi[8];
    uint32_t _pad;
} Acas2dPopulationExploit;

int acas2d_population_exploit_f32(const Acas2dPopulationExploit *x, void *stream);
size_t acas2d_population_exploit_size(void);  /* sizeof(Acas2dPopulationExploit): layout check for bindings */

/*
 * acas2d_reset_*: replaces ACAS2DEnv.reset() (environment.py:44-48 -> ACAS2DGame.__init__,
 * game.py:28-41,80-116, then observe()).  For every env with mask[e] != 0 (mask == NULL: all):
 *   do_init != 0: draw a fresh episode from the Philox stream described above
 *                 (episode[e] is read, not modified), steps = 0, total_reward = 0, status = 0;
 *   do_init == 0: keep the state the caller wrote into the buffers (oracle-state injection /
 *                 host-side MT19937 "parity reset"), only zero total_reward and status;
 * then, if obs != NULL, run observe(): steps += 1 and the first observation into obs[e].
 */
int acas2d_reset_f32(const Acas2dConfig *cfg, const Acas2dState *state, const uint8_t *mask,
                     void *obs, int32_t do_init, uint64_t seed, int64_t env_offset,
                     int64_t n_envs, int32_t n_traffic, void *stream);
int acas2d_reset_f64(const Acas2dConfig *cfg, const Acas2dState *state, const uint8_t *mask,
                     void *obs, int32_t do_init, uint64_t seed, int64_t env_offset,
                     int64_t n_envs, int32_t n_traffic, void *stream);

/* 1 if acas2d_step_* with ACAS2D_AUTO_RESET takes the consecutive-layout kernel for this state (see acas2d_step_*),
 * else 0.  Informational (bench / tests); never an error. */
int acas2d_state_is_consecutive(const Acas2dState *state, int64_t n_envs, int32_t n_traffic, int32_t elem_size);

/*
 * Launch geometry chosen for (n_envs, n_traffic, elem_size = 4 | 8): lanes per env (power of two
 * <= 64), traffic aircraft per lane (-1: generic strided walk), threads per workgroup and number
 * of workgroups.  Informational (bench / DESIGN.md); output pointers may be NULL.
 */
int acas2d_launch_geometry(int64_t n_envs, int32_t n_traffic, int32_t elem_size,
                           int32_t *lanes_per_env, int32_t *traffic_per_lane,
                           int32_t *block_threads, int64_t *grid_blocks);

#ifdef __cplusplus
}
#endif
#endif /* ACAS2D_H */
