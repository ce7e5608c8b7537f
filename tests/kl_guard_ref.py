"""Float64 restatement of what acas2d_ppo_update_guarded_set_f32 adds to the set update (test code only; the package never
imports it): SB3 1.1.0's approx_kl and clip_fraction of a minibatch and its target_kl stop rule, on top of
learner_ref.logp64.  Only the float64 mathematics: the rollout buffer the guarded tests run on is
learner_support.RolloutBatch.  Only numpy and learner_ref."""
import numpy as np

import learner_ref as R

EDGE = 1e-4          # no ratio closer than this to a clip edge: float32 and float64 would take different branches there


def log_ratio64(ac_cls, D, theta, obs, act, old_logp):
    """log pi(act | obs) - old_logp in float64 for the rows given, parameters `theta` (flat, PARAM_NAMES order)."""
    return R.logp64(ac_cls, D, theta, obs, act) - np.asarray(old_logp, np.float64)


def approx_kl64(log_ratio):
    """SB3 1.1.0: mean((ratio - 1) - log ratio)."""
    return float(np.mean((np.exp(log_ratio) - 1.0) - log_ratio))


def clip_fraction64(log_ratio, clip_range):
    """(count, fraction) of |ratio - 1| > clip_range."""
    count = int((np.abs(np.exp(log_ratio) - 1.0) > clip_range).sum())
    return count, count / len(log_ratio)


def edge_distance(log_ratio, clip_range):
    """min over rows of | |ratio - 1| - clip_range |: how far the nearest row is from changing its clipped bit."""
    return float(np.abs(np.abs(np.exp(log_ratio) - 1.0) - clip_range).min())


def stops(kl, target_kl):
    """SB3's rule, as the apply launch decides it: a limit is set and this minibatch's approx_kl exceeds 1.5 x it."""
    return target_kl > 0.0 and kl > 1.5 * target_kl
