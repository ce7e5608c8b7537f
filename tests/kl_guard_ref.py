"""Float64 restatement of what acas2d_ppo_update_guarded_set_f32 adds to the set update (test code only; the package never
imports it): SB3 1.1.0's approx_kl and clip_fraction of a minibatch and its target_kl stop rule, on top of
learner_ref.logp64 / grad64 / adam64 -- and the shared rollout buffer the guarded tests run on, the recipe of
tests/test_learner_kernels.py's _Batch with a member dimension ("mixed" old log-probs so that ratios spread, ratios
nudged 1e-4 off the clip edges), restated here so that no test module is imported.
Only numpy, torch and learner_ref."""
import numpy as np
import torch

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


def members(g, D, K, seed, device):
    """K actor-critics away from SB3's near-zero head (ratios spread, some clip), with different log-stds."""
    out = []
    for k in range(K):
        torch.manual_seed(seed + 17 * k)
        pol = g.ActorCritic(D).to(device)
        with torch.no_grad():
            pol.action_net.weight.mul_(40.0)
            pol.log_std.fill_(-0.7 + 0.2 * k)
        out.append(pol)
    return out


class SharedBatch:
    """One flat rollout buffer of n rows on `device`, shared by K members with different parameters."""

    def __init__(self, g, D, K, n, seed, device):
        rng = np.random.default_rng(seed)
        self.g, self.rng, self.D, self.K, self.n, self.device = g, rng, D, K, n, device
        f = lambda a: torch.as_tensor(np.asarray(a, np.float32), device=device).contiguous()  # noqa: E731
        self.obs = f(rng.uniform(-1, 1, (n, D)))
        self.act = f(rng.normal(0, 0.7, n))
        self.adv, self.ret = f(rng.normal(0, 2, n)), f(rng.normal(2, 3, n))     # (value offset: gradient norm > 0.5 at any B)
        self.old_logp = torch.zeros(n, dtype=torch.float32, device=device)
        self.pols = members(g, D, K, seed, device)
        self.bufs = (self.obs, self.act, self.old_logp, self.adv, self.ret)

    def policy_set(self):
        """A fresh ActorCriticSet holding copies of the members as constructed (twins start from the same bits)."""
        return self.g.ActorCriticSet.from_members(self.pols)

    @staticmethod
    def theta(pset, k):
        return torch.cat([pset.params[n][k].reshape(-1) for n in R.PARAM_NAMES]).double().cpu().numpy()

    def host(self, rows):
        i = rows.cpu().numpy()
        return [t.cpu().numpy().astype(np.float64)[i] for t in self.bufs]

    def set_old_logp(self, theta, rows, mode, clip):
        """old_logp of `rows` for the member with parameters `theta`: "mixed" its float64 log-prob plus N(0, 0.5) noise,
        "first" the log-prob itself (ratio ~ 1); ratios within EDGE of a clip edge are moved off it."""
        i = rows.cpu().numpy()
        lp = R.logp64(self.g.ActorCritic, self.D, theta, self.obs.cpu().numpy()[i], self.act.cpu().numpy()[i])
        old = lp + (self.rng.normal(0, 0.5, len(i)) if mode == "mixed" else 0.0)
        old = old.astype(np.float32).astype(np.float64)
        r = np.exp(lp - old)
        edge = (np.abs(r - (1 - clip)) < EDGE) | (np.abs(r - (1 + clip)) < EDGE)
        old[edge] -= 1e-3
        self.old_logp[rows] = torch.as_tensor(old.astype(np.float32), device=self.device)

    def log_ratio(self, theta, rows):
        obs, act, old, _, _ = self.host(rows)
        return log_ratio64(self.g.ActorCritic, self.D, theta, obs, act, old)
