"""The reward normalisation of acas2d_reward_normalize_f32 (include/acas2d.h: SB3 1.1.0's VecNormalize.step_wait with
RunningMeanStd.update_from_moments) restated in float64 NumPy, with the order of the two sums over a member's envs as a
parameter: NumPy's own (pairwise) or sequential, ascending.  The referee of tests/test_reward_norm.py."""
import numpy as np

FLT_MAX = np.finfo(np.float32).max
ORDERS = ("numpy", "sequential")


def fresh_state(n_envs, n_members=1):
    """(returns [E], stats [K, 3]) as SB3 starts them: G = 0; mean, var, count = 0, 1, 1e-4."""
    return np.zeros(n_envs, np.float64), np.tile(np.array([0.0, 1.0, 1e-4]), (n_members, 1))


def _sum(x, order):
    """Sum over the last axis of [K, EM]."""
    if order == "numpy":
        return x.sum(-1)
    assert order == "sequential", order
    return np.cumsum(x, axis=-1)[..., -1]                 # (cumsum adds one element after the other, ascending)


def normalize(reward, done, returns, stats, gamma, epsilon=1e-8, clip=10.0, n_members=1, order="numpy"):
    """reward float32 [T, E], done [T, E], returns float64 [E], stats float64 [K, 3], gamma: a number or [K].
    Returns (out float32 [T, E], returns, stats) -- new arrays, the inputs are left alone."""
    reward = np.asarray(reward, np.float32)
    T, E = reward.shape
    K = int(n_members)
    EM = E // K
    assert EM * K == E
    gam = np.broadcast_to(np.asarray(gamma, np.float64).reshape(-1, 1), (K, 1))
    r_all = np.where(np.isnan(reward), np.float32(0), np.clip(reward, -FLT_MAX, FLT_MAX)).astype(np.float32)
    G = np.array(returns, np.float64).reshape(K, EM)
    stats = np.array(stats, np.float64)
    mean, var, count = stats[:, 0].copy(), stats[:, 1].copy(), stats[:, 2].copy()
    out = np.empty((T, E), np.float32)
    with np.errstate(over="ignore"):
        for t in range(T):
            r = r_all[t].astype(np.float64).reshape(K, EM)
            G = G * gam + r
            bm = _sum(G, order) / EM
            d = G - bm[:, None]
            bv = _sum(d * d, order) / EM
            delta = bm - mean
            tot = count + EM
            mean_new = mean + delta * EM / tot
            m2 = var * count + bv * EM + delta * delta * count * EM / tot
            var, mean, count = m2 / tot, mean_new, tot
            out[t] = np.minimum(np.maximum(r / np.sqrt(var + epsilon)[:, None], -clip), clip).reshape(E).astype(np.float32)
            G = np.where(np.asarray(done[t]).astype(bool).reshape(K, EM), 0.0, G)
    return out, G.reshape(E), np.stack((mean, var, count), 1)
