"""ctypes binding of libacas2d_hip.so (include/acas2d.h).  There is NO fallback: if the HIP
library is missing or fails to load, importing the engine raises."""
import ctypes as C
import os
import subprocess

from .config import CConfig

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB_PATH = os.path.join(_CSRC, "libacas2d_hip.so")
ABI_VERSION = 7

AUTO_RESET = 1


class CState(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "own_x", "own_y", "own_psi", "own_v", "goal_x", "goal_y", "trf_x", "trf_y", "trf_psi",
        "trf_v", "steps", "total_reward", "status", "episode", "trace")]


class CStepIO(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "actions", "obs", "reward", "done", "outcome", "term_obs", "ep_return", "ep_steps")]


class CPolicy(C.Structure):
    """struct Acas2dPolicy: the SB3 MlpPolicy actor, float32, first two weights transposed."""
    _fields_ = [(n, C.c_void_p) for n in ("w1t", "b1", "w2t", "b2", "w3", "b3")] + \
               [("hidden", C.c_int32), ("_pad", C.c_int32)]


class CActorCritic(C.Structure):
    """struct Acas2dActorCritic: actor + value net + log-std, the per-step value / log-prob outputs, the noise stream."""
    _fields_ = [("actor", CPolicy)] + [(n, C.c_void_p) for n in ("v1t", "vb1", "v2t", "vb2", "v3", "vb3", "log_std",
                                                                 "values", "logp")] + \
               [("noise_seed", C.c_uint64), ("noise_step", C.c_uint32), ("_pad", C.c_uint32)]


class CPpoUpdate(C.Structure):
    """struct Acas2dPpoUpdate: one PPO minibatch update (include/acas2d.h)."""
    _fields_ = [(n, C.c_void_p) for n in (
        "actor_w1", "actor_b1", "actor_w2", "actor_b2", "actor_w3", "actor_b3", "critic_w1", "critic_b1", "critic_w2",
        "critic_b2", "critic_w3", "critic_b3", "log_std", "obs", "act", "old_logp", "adv", "ret", "idx")] + \
        [("n_rows", C.c_int32), ("obs_dim", C.c_int32)] + \
        [(n, C.c_float) for n in ("clip_range", "vf_coef", "ent_coef", "max_grad_norm", "learning_rate", "beta1", "beta2",
                                  "adam_eps")] + \
        [(n, C.c_void_p) for n in ("grad", "adam_m", "adam_v", "adam_step", "stats")]


class CPpoUpdateSet(C.Structure):
    """struct Acas2dPpoUpdateSet: one PPO minibatch update of K stacked learners (include/acas2d.h)."""
    _fields_ = [(n, C.c_void_p) for n in (
        "actor_w1", "actor_b1", "actor_w2", "actor_b2", "actor_w3", "actor_b3", "critic_w1", "critic_b1", "critic_w2",
        "critic_b2", "critic_w3", "critic_b3", "log_std", "obs", "act", "old_logp", "adv", "ret", "idx")] + \
        [(n, C.c_int32) for n in ("n_members", "n_rows", "obs_dim", "apply")] + \
        [(n, C.c_void_p) for n in ("hyper", "grad", "adam_m", "adam_v", "adam_step", "stats")]


class CPpoGuard(C.Structure):
    """struct Acas2dPpoGuard: the target_kl limits, stop flags and KL / clip statistics of K stacked learners
    (include/acas2d.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("target_kl", "stopped", "diag")]


class CPpoOptions(C.Structure):
    """struct Acas2dPpoOptions: the rollout's values, the value clips [K] and the per-update factors [K][4] of
    acas2d_ppo_update_sb3_set_f32 (include/acas2d.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("old_val", "clip_range_vf", "scale")]


class CEvalStats(C.Structure):
    """struct Acas2dEvalStats: the six per-episode safety statistics [K][n_episodes] of acas2d_evaluate_policies_stats_*
    (include/acas2d.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("min_sep", "min_sep_step", "los_steps", "max_a_lat", "max_dev", "sum_dev")]


class CMonteCarlo(C.Structure):
    """struct Acas2dMonteCarlo: the accumulators of a Monte Carlo campaign, the histogram's bin rule and the launch's episode
    counters (acas2d_monte_carlo_*, include/acas2d.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("outcome_count", "sum_steps", "los_episodes", "sum_los_steps", "sep_hist",
                                          "lane_return_sum", "lane_return_sq", "lane_worst_sep", "lane_worst_episode")] + \
        [("n_bins", C.c_int32), ("episodes_per_lane", C.c_int32), ("inv_bin_width", C.c_double),
         ("first_episode", C.c_uint32), ("_pad", C.c_uint32)]


class CDisturbance(C.Structure):
    """struct Acas2dDisturbance: the four standard deviations (normalised observation units / action units), the noise
    seed and the evaluator's episode counter (acas2d_evaluate_policies_disturbed_*, acas2d_monte_carlo_disturbed_*,
    include/acas2d.h)."""
    _fields_ = [(n, C.c_float) for n in ("s_sep", "s_cpa", "s_closing", "s_action")] + \
        [("noise_seed", C.c_uint64), ("noise_episode", C.c_uint32), ("_pad", C.c_uint32)]


class CCorrelation(C.Structure):
    """struct Acas2dCorrelation: the four channels' step-to-step correlation coefficients, each in [0, 1]
    (acas2d_evaluate_policies_correlated_*, acas2d_monte_carlo_correlated_*, include/acas2d.h)."""
    _fields_ = [(n, C.c_float) for n in ("rho_sep", "rho_cpa", "rho_closing", "rho_action")]


class CResponse(C.Structure):
    """struct Acas2dResponse: the dead time in steps, the lag's pole in [0, 1], and the dead time's device scratch
    float[delay_steps][ring_envs] (acas2d_evaluate_policies_delayed_*, acas2d_monte_carlo_delayed_*, include/acas2d.h)."""
    _fields_ = [("delay_steps", C.c_int32), ("lag", C.c_float), ("ring", C.c_void_p), ("ring_envs", C.c_int64)]


class CEncounterSearch(C.Structure):
    """struct Acas2dEncounterSearch: the proposal's tables, the per-candidate buffers, the stats entry's outputs, the log row,
    the archive and the settings of one generation of an encounter search (acas2d_encounter_*, include/acas2d.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("p", "cdf", "log_ratio", "active", "bins", "log_w", "elite_w", "outcome", "min_sep",
                                          "history", "best_score", "best_generation", "best_candidate", "best_own_psi",
                                          "best_traffic")] + \
        [(n, C.c_int32) for n in ("n_bins", "n_coord", "n_quantile", "weighted")] + \
        [(n, C.c_double) for n in ("alpha", "p_floor", "level")] + [("generation", C.c_uint64)]


SEARCH_HISTORY_WIDTH = 16


class CGae(C.Structure):
    """struct Acas2dGae: the bootstrap value and GAE over the collector's [T][E] buffers (include/acas2d.h)."""
    _fields_ = [(n, C.c_void_p) for n in (
        "reward", "value", "done", "last_value", "obs_last", "v1t", "vb1", "v2t", "vb2", "v3", "vb3", "gamma",
        "gamma_lambda", "adv", "ret", "last_value_out", "nan_count")] + \
        [("n_envs", C.c_int64)] + [(n, C.c_int32) for n in ("n_steps", "n_members", "obs_dim", "_pad")]


class CRewardNorm(C.Structure):
    """struct Acas2dRewardNorm: VecNormalize's reward normalisation over the collector's [T][E] rewards (include/acas2d.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("reward", "done", "out", "returns", "stats", "gamma", "workspace")] + \
        [("epsilon", C.c_double), ("clip", C.c_double), ("n_envs", C.c_int64), ("n_steps", C.c_int32),
         ("n_members", C.c_int32)]


class CMemberEpisodes(C.Structure):
    """struct Acas2dMemberEpisodes: per-member episode statistics of a collection (include/acas2d.h)."""
    _fields_ = [(n, C.c_void_p) for n in (
        "done", "outcome", "ep_return", "ep_steps", "ep_count", "ep_outcomes", "ep_steps_sum", "ep_return_sum", "score")] + \
        [("n_envs", C.c_int64), ("n_steps", C.c_int32), ("n_members", C.c_int32)]


class CPopulationExploit(C.Structure):
    """struct Acas2dPopulationExploit: truncation selection, copy and perturbation among K stacked learners
    (include/acas2d.h)."""
    _fields_ = [(n, C.c_void_p) for n in (
        "actor_w1", "actor_b1", "actor_w2", "actor_b2", "actor_w3", "actor_b3", "critic_w1", "critic_b1", "critic_w2",
        "critic_b2", "critic_w3", "critic_b3", "log_std", "adam_m", "adam_v", "adam_step", "hyper", "score", "donor")] + \
        [(n, C.c_int32) for n in ("n_members", "obs_dim", "n_replace")] + \
        [("generation", C.c_uint32), ("seed", C.c_uint64), ("perturb_mask", C.c_uint32), ("factor_lo", C.c_float),
         ("factor_hi", C.c_float), ("lo", C.c_float * 8), ("hi", C.c_float * 8), ("_pad", C.c_uint32)]


EXPORTS = ("acas2d_abi_version", "acas2d_config_size", "acas2d_state_size", "acas2d_last_error", "acas2d_step_f32",
           "acas2d_step_f64", "acas2d_rollout_f32", "acas2d_rollout_f64", "acas2d_rollout_policy_f32",
           "acas2d_rollout_policy_f64", "acas2d_collect_f32", "acas2d_collect_f64", "acas2d_ppo_workspace_floats",
           "acas2d_ppo_update_f32", "acas2d_reset_f32", "acas2d_reset_f64", "acas2d_launch_geometry",
           "acas2d_state_is_consecutive", "acas2d_evaluate_policies_f32", "acas2d_evaluate_policies_f64",
           "acas2d_rollout_policy_group_f32", "acas2d_collect_group_f32", "acas2d_evaluate_policies_group_f32",
           "acas2d_ppo_update_wide_f32", "acas2d_ppo_wide_lds_bytes", "acas2d_collect_set_f32", "acas2d_ppo_update_set_f32",
           "acas2d_gae_f32", "acas2d_gae_size", "acas2d_gae_pipeline_depth", "acas2d_collect_set_group_f32",
           "acas2d_ppo_update_wide_set_f32", "acas2d_member_episodes_f32", "acas2d_member_episodes_size",
           "acas2d_population_exploit_f32", "acas2d_population_exploit_size", "acas2d_ppo_update_guarded_set_f32",
           "acas2d_ppo_guard_size", "acas2d_ppo_update_sb3_set_f32", "acas2d_ppo_options_size",
           "acas2d_reward_normalize_f32", "acas2d_reward_norm_size", "acas2d_reward_norm_workspace_bytes",
           "acas2d_reward_norm_pipeline_depth", "acas2d_evaluate_policies_stats_f32", "acas2d_evaluate_policies_stats_f64",
           "acas2d_evaluate_policies_stats_group_f32", "acas2d_monte_carlo_f32", "acas2d_monte_carlo_f64",
           "acas2d_monte_carlo_group_f32", "acas2d_monte_carlo_size", "acas2d_encounter_sample_f32",
           "acas2d_encounter_sample_f64", "acas2d_encounter_select_f32", "acas2d_encounter_select_f64", "acas2d_encounter_refit",
           "acas2d_encounter_search_size", "acas2d_disturbance_size", "acas2d_evaluate_policies_disturbed_f32",
           "acas2d_evaluate_policies_disturbed_group_f32", "acas2d_monte_carlo_disturbed_f32",
           "acas2d_monte_carlo_disturbed_group_f32", "acas2d_disturbance_draw_f32", "acas2d_collect_set_disturbed_f32",
           "acas2d_collect_set_disturbed_group_f32", "acas2d_correlation_size", "acas2d_evaluate_policies_correlated_f32",
           "acas2d_evaluate_policies_correlated_group_f32", "acas2d_monte_carlo_correlated_f32",
           "acas2d_monte_carlo_correlated_group_f32", "acas2d_collect_set_correlated_f32",
           "acas2d_collect_set_correlated_group_f32", "acas2d_response_size", "acas2d_evaluate_policies_delayed_f32",
           "acas2d_evaluate_policies_delayed_group_f32", "acas2d_monte_carlo_delayed_f32", "acas2d_monte_carlo_delayed_group_f32")


class NativeLibraryError(RuntimeError):
    pass


def build(verbose=False):
    """Compile the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    r = subprocess.run(["make", "-C", _CSRC, "-j4"], capture_output=True, text=True)
    if verbose or r.returncode:
        print(r.stdout + r.stderr)
    if r.returncode:
        raise NativeLibraryError("building libacas2d_hip.so failed:\n" + r.stderr[-2000:])
    return LIB_PATH


_lib = None


def lib():
    """Load the library once.  torch must be imported first so that the HIP runtime the kernels
    register with (DT_NEEDED libamdhip64.so.7) is the one torch already loaded."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  (loads torch's libamdhip64 before ours resolves its DT_NEEDED)
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryError(
            "%s not found -- run `python -c 'import __graft_entry__ as g; g.build()'` or "
            "`make -C %s`.  The ACAS2D engine has no CPU fallback." % (LIB_PATH, _CSRC))
    try:
        L = C.CDLL(LIB_PATH)
    except OSError as e:
        raise NativeLibraryError("cannot load %s: %s" % (LIB_PATH, e)) from e
    missing = [n for n in EXPORTS if not hasattr(L, n)]
    if missing:
        raise NativeLibraryError("libacas2d_hip.so lacks symbols: %s" % missing)
    L.acas2d_abi_version.restype = C.c_int
    L.acas2d_config_size.restype = C.c_size_t
    L.acas2d_state_size.restype = C.c_size_t
    L.acas2d_last_error.restype = C.c_char_p
    for name in ("acas2d_step_f32", "acas2d_step_f64"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [C.POINTER(CConfig), C.POINTER(CState), C.POINTER(CState), C.POINTER(CStepIO), C.c_uint32,
                      C.c_uint64, C.c_int64, C.c_int64, C.c_int32, C.c_void_p]      # state_out may be None
    for name in ("acas2d_rollout_f32", "acas2d_rollout_f64"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [C.POINTER(CConfig), C.POINTER(CState), C.POINTER(CStepIO), C.c_int32,
                      C.c_uint64, C.c_int64, C.c_int64, C.c_int32, C.c_void_p]
    for name in ("acas2d_rollout_policy_f32", "acas2d_rollout_policy_f64", "acas2d_rollout_policy_group_f32"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [C.POINTER(CConfig), C.POINTER(CState), C.POINTER(CStepIO), C.POINTER(CPolicy), C.c_void_p,
                      C.c_int32, C.c_uint64, C.c_int64, C.c_int64, C.c_int32, C.c_void_p]
    for name in ("acas2d_collect_f32", "acas2d_collect_f64", "acas2d_collect_group_f32"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [C.POINTER(CConfig), C.POINTER(CState), C.POINTER(CStepIO), C.POINTER(CActorCritic), C.c_void_p,
                      C.c_int32, C.c_uint64, C.c_int64, C.c_int64, C.c_int32, C.c_void_p]
    # the policy-scoring family (acas2d_evaluate_policies_*, acas2d_monte_carlo_*): cfg, state, n_envs, policies, n_policies,
    # n_episodes / n_lanes, obs_in, n_steps, seed, env_offset, n_traffic -- then each entry's own outputs, then the stream
    head = [C.POINTER(CConfig), C.POINTER(CState), C.c_int64, C.POINTER(CPolicy), C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
            C.c_uint64, C.c_int64, C.c_int32]
    results = [C.c_void_p, C.c_void_p, C.c_void_p]          # outcome, steps, total_reward
    for stem, tail in (("evaluate_policies", results), ("evaluate_policies_stats", results + [C.POINTER(CEvalStats)]),
                       ("evaluate_policies_disturbed", results + [C.POINTER(CEvalStats), C.POINTER(CDisturbance)]),
                       ("monte_carlo", [C.POINTER(CMonteCarlo)]),
                       ("monte_carlo_disturbed", [C.POINTER(CMonteCarlo), C.POINTER(CDisturbance)]),
                       ("evaluate_policies_correlated", results + [C.POINTER(CEvalStats), C.POINTER(CDisturbance),
                                                                   C.POINTER(CCorrelation)]),
                       ("monte_carlo_correlated", [C.POINTER(CMonteCarlo), C.POINTER(CDisturbance), C.POINTER(CCorrelation)]),
                       ("evaluate_policies_delayed", results + [C.POINTER(CEvalStats), C.POINTER(CDisturbance),
                                                                C.POINTER(CCorrelation), C.POINTER(CResponse)]),
                       ("monte_carlo_delayed", [C.POINTER(CMonteCarlo), C.POINTER(CDisturbance), C.POINTER(CCorrelation),
                                                C.POINTER(CResponse)])):
        for sfx in ("f32", "group_f32") + (() if stem.endswith(("disturbed", "correlated", "delayed")) else ("f64",)):     # (those: float32 only)
            f = getattr(L, "acas2d_%s_%s" % (stem, sfx))
            f.restype = C.c_int
            f.argtypes = head + tail + [C.c_void_p]
    L.acas2d_monte_carlo_size.restype = C.c_size_t
    L.acas2d_disturbance_draw_f32.restype = C.c_int
    L.acas2d_disturbance_draw_f32.argtypes = [C.c_uint64, C.c_int64, C.c_int32, C.c_uint32, C.c_int32, C.c_int32, C.c_int32,
                                              C.c_void_p, C.c_void_p]
    L.acas2d_disturbance_size.restype = C.c_size_t
    L.acas2d_correlation_size.restype = C.c_size_t
    L.acas2d_response_size.restype = C.c_size_t
    for name in ("acas2d_encounter_sample_f32", "acas2d_encounter_sample_f64"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [C.POINTER(CConfig), C.POINTER(CState), C.c_int64, C.c_int32, C.c_int32, C.c_uint64, C.c_int64, C.c_int32,
                      C.POINTER(CEncounterSearch), C.c_void_p]
    for name in ("acas2d_encounter_select_f32", "acas2d_encounter_select_f64"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [C.POINTER(CConfig), C.c_int32, C.c_int32, C.c_uint64, C.c_int64, C.c_int32, C.POINTER(CEncounterSearch),
                      C.c_void_p]
    L.acas2d_encounter_refit.restype = C.c_int
    L.acas2d_encounter_refit.argtypes = [C.POINTER(CEncounterSearch), C.c_int32, C.c_int32, C.c_void_p]
    L.acas2d_encounter_search_size.restype = C.c_size_t
    for name in ("acas2d_collect_set_f32", "acas2d_collect_set_group_f32"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [C.POINTER(CConfig), C.POINTER(CState), C.POINTER(CStepIO), C.POINTER(CActorCritic), C.c_int32,
                      C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_int64, C.c_int64, C.c_int32, C.c_void_p]
    # ... under sensor noise and actuator disturbance: then sigmas (device float[K][4]), dist_seed, obs_read, the stream
    for name in ("acas2d_collect_set_disturbed_f32", "acas2d_collect_set_disturbed_group_f32"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [C.POINTER(CConfig), C.POINTER(CState), C.POINTER(CStepIO), C.POINTER(CActorCritic), C.c_int32,
                      C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_uint64,
                      C.c_void_p, C.c_void_p]
    # ... under time-correlated errors: then correlations (device float[K][8]) and held (device float[3 N + 1][E]) in front of it
    for name in ("acas2d_collect_set_correlated_f32", "acas2d_collect_set_correlated_group_f32"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [C.POINTER(CConfig), C.POINTER(CState), C.POINTER(CStepIO), C.POINTER(CActorCritic), C.c_int32,
                      C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_uint64,
                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    for name in ("acas2d_ppo_update_set_f32", "acas2d_ppo_update_wide_set_f32"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [C.POINTER(CPpoUpdateSet), C.c_void_p]
    L.acas2d_ppo_update_guarded_set_f32.restype = C.c_int
    L.acas2d_ppo_update_guarded_set_f32.argtypes = [C.POINTER(CPpoUpdateSet), C.POINTER(CPpoGuard), C.c_void_p]
    L.acas2d_ppo_guard_size.restype = C.c_size_t
    L.acas2d_ppo_update_sb3_set_f32.restype = C.c_int
    L.acas2d_ppo_update_sb3_set_f32.argtypes = [C.POINTER(CPpoUpdateSet), C.POINTER(CPpoGuard), C.POINTER(CPpoOptions),
                                                C.c_void_p]
    L.acas2d_ppo_options_size.restype = C.c_size_t
    L.acas2d_gae_f32.restype = C.c_int
    L.acas2d_gae_f32.argtypes = [C.POINTER(CGae), C.c_void_p]
    L.acas2d_gae_size.restype = C.c_size_t
    L.acas2d_gae_pipeline_depth.restype = C.c_int
    L.acas2d_reward_normalize_f32.restype = C.c_int
    L.acas2d_reward_normalize_f32.argtypes = [C.POINTER(CRewardNorm), C.c_void_p]
    L.acas2d_reward_norm_size.restype = C.c_size_t
    L.acas2d_reward_norm_workspace_bytes.restype = C.c_size_t
    L.acas2d_reward_norm_workspace_bytes.argtypes = [C.c_int64, C.c_int32, C.c_int32]
    L.acas2d_reward_norm_pipeline_depth.restype = C.c_int
    L.acas2d_member_episodes_f32.restype = C.c_int
    L.acas2d_member_episodes_f32.argtypes = [C.POINTER(CMemberEpisodes), C.c_void_p]
    L.acas2d_member_episodes_size.restype = C.c_size_t
    L.acas2d_population_exploit_f32.restype = C.c_int
    L.acas2d_population_exploit_f32.argtypes = [C.POINTER(CPopulationExploit), C.c_void_p]
    L.acas2d_population_exploit_size.restype = C.c_size_t
    L.acas2d_ppo_workspace_floats.restype = C.c_int
    L.acas2d_ppo_workspace_floats.argtypes = [C.c_int32]
    for name in ("acas2d_ppo_update_f32", "acas2d_ppo_update_wide_f32"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [C.POINTER(CPpoUpdate), C.c_void_p]
    L.acas2d_ppo_wide_lds_bytes.restype = C.c_int
    L.acas2d_ppo_wide_lds_bytes.argtypes = [C.c_int32]
    for name in ("acas2d_reset_f32", "acas2d_reset_f64"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [C.POINTER(CConfig), C.POINTER(CState), C.c_void_p, C.c_void_p, C.c_int32,
                      C.c_uint64, C.c_int64, C.c_int64, C.c_int32, C.c_void_p]
    L.acas2d_state_is_consecutive.restype = C.c_int
    L.acas2d_state_is_consecutive.argtypes = [C.POINTER(CState), C.c_int64, C.c_int32, C.c_int32]
    L.acas2d_launch_geometry.restype = C.c_int
    L.acas2d_launch_geometry.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int32),
                                         C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    if L.acas2d_abi_version() != ABI_VERSION:
        raise NativeLibraryError("ABI version %d != %d" % (L.acas2d_abi_version(), ABI_VERSION))
    if L.acas2d_config_size() != C.sizeof(CConfig):
        raise NativeLibraryError("Acas2dConfig layout mismatch: %d != %d" %
                                 (L.acas2d_config_size(), C.sizeof(CConfig)))
    if L.acas2d_state_size() != C.sizeof(CState):
        raise NativeLibraryError("Acas2dState layout mismatch: %d != %d" % (L.acas2d_state_size(), C.sizeof(CState)))
    if L.acas2d_gae_size() != C.sizeof(CGae):
        raise NativeLibraryError("Acas2dGae layout mismatch: %d != %d" % (L.acas2d_gae_size(), C.sizeof(CGae)))
    for name, twin in (("member_episodes", CMemberEpisodes), ("population_exploit", CPopulationExploit),
                       ("ppo_guard", CPpoGuard), ("ppo_options", CPpoOptions), ("reward_norm", CRewardNorm),
                       ("monte_carlo", CMonteCarlo), ("encounter_search", CEncounterSearch),
                       ("disturbance", CDisturbance), ("correlation", CCorrelation), ("response", CResponse)):
        size = getattr(L, "acas2d_%s_size" % name)()
        if size != C.sizeof(twin):
            raise NativeLibraryError("%s layout mismatch: %d != %d" % (twin.__name__, size, C.sizeof(twin)))
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise RuntimeError("acas2d: error %d: %s" % (rc, lib().acas2d_last_error().decode()))


def launch_geometry(n_envs, n_traffic, elem_size=4):
    g, c, b, n = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    check(lib().acas2d_launch_geometry(n_envs, n_traffic, elem_size, C.byref(g), C.byref(c), C.byref(b),
                                       C.byref(n)))
    return {"lanes_per_env": g.value, "traffic_per_lane": c.value, "block_threads": b.value,
            "grid_blocks": n.value}
