"""Float64 restatement of what acas2d_ppo_update_sb3_set_f32 adds to the guarded set update (test code only; the package
never imports it): SB3 1.1.0's clipped value loss, and the update of one member under effective (scaled) numbers.  The
loss below is a LOCAL copy -- it does not call ppo.ppo_loss, which the tests hold to it -- over learner_ref's float64
policy, with float64 torch autograd; the step is learner_ref.adam64.
Only numpy, torch and learner_ref."""
import math

import numpy as np
import torch

import learner_ref as R

LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)
EDGE = 1e-4          # no row closer than this to +-c (or a ratio to a clip edge): float32 and float64 would part there


def f32(x):
    """A Python number as the float32 the kernels read, back in float64."""
    return float(np.float32(x))


def product32(a, b):
    """float32(a) * float32(b) rounded to float32 -- the ONE product the kernels form -- as a float64 number."""
    return float(np.float32(a) * np.float32(b))


def value_loss64(value, old_val, ret, c):
    """NumPy: SB3's value loss of one minibatch.  c None or <= 0: F.mse_loss(returns, values); otherwise on values_pred =
    old_values + clamp(values - old_values, -c, c), with no max against the unclipped loss.  Returns (loss, values_pred)."""
    value, old_val, ret = (np.asarray(a, np.float64) for a in (value, old_val, ret))
    vp = value if c is None or not c > 0 else old_val + np.clip(value - old_val, -c, c)
    return float(np.mean((ret - vp) ** 2)), vp


def dvalue64(value, old_val, ret, c, vf_coef):
    """Closed form of d loss / d value: vf_coef * 2 (vp - ret) / B on the rows with |value - old_val| <= c (torch's clamp
    passes the gradient on the CLOSED interval), 0 elsewhere; every row with c None or <= 0."""
    value, old_val, ret = (np.asarray(a, np.float64) for a in (value, old_val, ret))
    _, vp = value_loss64(value, old_val, ret, c)
    g = vf_coef * 2.0 * (vp - ret) / len(ret)
    if c is None or not c > 0:
        return g
    d = value - old_val
    return np.where((d >= -c) & (d <= c), g, 0.0)


def loss64(pol, obs, act, old_logp, adv, ret, old_val, clip_range, clip_vf, vf_coef, ent_coef):
    """The local copy of SB3's minibatch loss on a float64 policy (torch float64 tensors in): (loss, pg, vf, value)."""
    mean, value = pol.forward(obs)
    ls = pol.log_std
    logp = (-((act - mean) ** 2) / (2.0 * (2.0 * ls).exp()) - ls - LOG_SQRT_2PI).sum(-1)
    a = (adv - adv.mean()) / (adv.std() + 1e-8)
    ratio = (logp - old_logp).exp()
    pg = -torch.min(a * ratio, a * torch.clamp(ratio, 1.0 - clip_range, 1.0 + clip_range)).mean()
    if clip_vf is None or not clip_vf > 0:
        vf = ((ret - value) ** 2).mean()
    else:
        vf = ((ret - (old_val + torch.clamp(value - old_val, -clip_vf, clip_vf))) ** 2).mean()
    ent = -(0.5 + LOG_SQRT_2PI + ls).sum()
    return pg + ent_coef * ent + vf_coef * vf, pg, vf, value


def grad64(ac_cls, cfg, D, theta, obs, act, old_logp, adv, ret, old_val=None, clip_range=None, clip_vf=None):
    """loss64 of one minibatch (the rows given) with float64 autograd; clip_range defaults to cfg's, clip_vf to None (plain
    MSE).  Returns (flat gradient, pg, vf, ratio, value): learner_ref.grad64's tuple plus the critic's float64 output."""
    pol = R.policy64(ac_cls, D, theta)
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))  # noqa: E731
    x = t(R.obs32(obs))
    ov = None if old_val is None else t(old_val)
    loss, pg, vf, value = loss64(pol, x, t(act).reshape(-1, 1), t(old_logp), t(adv), t(ret), ov,
                                 cfg.clip_range if clip_range is None else clip_range, clip_vf, cfg.vf_coef, cfg.ent_coef)
    loss.backward()
    g = torch.cat([pol.get_parameter(n).grad.reshape(-1) for n in R.PARAM_NAMES]).numpy()
    with torch.no_grad():
        mean, _ = pol.forward(x)
        ls = pol.log_std
        logp = (-((t(act).reshape(-1, 1) - mean) ** 2) / (2.0 * (2.0 * ls).exp()) - ls - LOG_SQRT_2PI).sum(-1)
        ratio = (logp - t(old_logp)).exp().numpy()
    return g, float(pg.detach()), float(vf.detach()), ratio, value.detach().numpy()


def value64(ac_cls, D, theta, obs):
    """The critic's float64 output on float32-rounded observations."""
    pol = R.policy64(ac_cls, D, theta)
    with torch.no_grad():
        return pol.forward(torch.as_tensor(R.obs32(obs)))[1].numpy()


def place_old_val(rng, value, c, sigma=0.8):
    """float32 old values = value + N(0, sigma) with every row's | |value - old| - c | >= EDGE: rows closer are moved off,
    as RolloutBatch.set_old_logp does for ratios.  c None or <= 0: no edge to keep away from."""
    old = (np.asarray(value, np.float64) + rng.normal(0, sigma, len(value))).astype(np.float32).astype(np.float64)
    if c is not None and c > 0:
        for _ in range(4):
            near = np.abs(np.abs(value - old) - c) < 2 * EDGE
            if not near.any():
                break
            old[near] = (old[near] - 1e-2).astype(np.float32).astype(np.float64)
    return old
