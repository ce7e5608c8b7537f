"""NumPy restatement of the two launches of population-based training (csrc/acas2d_pbt.hip), for tests/test_pbt.py.

`exploit` restates the normative rules of acas2d_population_exploit_f32 (include/acas2d.h) -- key, rank, recipients, the
random donor, the copy condition, the perturbation -- on top of oracle.philox4x32, the seven-round generator that
Random123's vectors pin.  `episodes` restates acas2d_member_episodes_f32's sums: integers exactly, the return sum as the
correctly rounded double of the exact sum (math.fsum).  Only numpy and oracle.philox4x32."""
import math

import numpy as np

DOMAIN = 0x70627431                  # the counter word that separates these draws from every other stream of the project
HYPER_SLOTS = ("clip_range", "vf_coef", "ent_coef", "max_grad_norm", "learning_rate", "beta1", "beta2", "adam_eps")


def keys(score):
    s = np.asarray(score, np.float32)
    return np.where(np.isnan(s), np.float32(-np.inf), s).astype(np.float32)


def ranks(score):
    """rank_k = #{j : key_j > key_k} + #{j < k : key_j == key_k}: a permutation of 0 .. K - 1, 0 the best."""
    key = keys(score)
    j = np.arange(len(key))
    greater = key[None, :] > key[:, None]
    tie_before = (key[None, :] == key[:, None]) & (j[None, :] < j[:, None])
    return (greater.sum(1) + tie_before.sum(1)).astype(np.int64)


def words(k, generation, seed):
    from oracle import oracle as O
    seed = int(seed) & (2 ** 64 - 1)
    return O.philox4x32([k, int(generation) & 0xffffffff, 0, DOMAIN], [seed & 0xffffffff, seed >> 32])


def target_rank(wx, R):
    return (int(wx) * int(R)) >> 32


def perturbed(h, bit, factor_lo, factor_hi, lo, hi):
    """fminf(fmaxf(h * f, lo), hi) with one float32 multiplication."""
    f = np.float32(factor_hi if bit else factor_lo)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.fmin(np.fmax(np.float32(h) * f, np.float32(lo)), np.float32(hi)).astype(np.float32)


def exploit(score, hyper, n_replace, generation, seed, perturb_mask, factor_lo, factor_hi, lo, hi):
    """-> (donor int32 [K], hyper float32 [K, 8] after the step).  Everything else a recipient k with donor[k] != k takes
    is a bit copy of member donor[k]'s row (`gather`)."""
    hyper = np.array(hyper, np.float32)
    K, R = len(hyper), int(n_replace)
    assert 0 <= 2 * R <= K
    key, rank = keys(score), ranks(score)
    by_rank = np.argsort(rank)
    donor = np.arange(K, dtype=np.int32)
    out = hyper.copy()
    for k in range(K):
        if rank[k] < K - R:
            continue
        w = words(k, generation, seed)
        d = int(by_rank[target_rank(w[0], R)])
        if not key[d] > key[k]:
            continue
        donor[k] = d
        for s in range(8):
            if (perturb_mask >> s) & 1:
                out[k, s] = perturbed(hyper[d, s], (int(w[1]) >> s) & 1, factor_lo, factor_hi, lo[s], hi[s])
            else:
                out[k].view(np.uint32)[s] = hyper[d].view(np.uint32)[s]
    return donor, out


def gather(rows, donor):
    """Member k's row becomes member donor[k]'s, bit for bit: rows [K, ...] of any 4-byte dtype."""
    rows = np.ascontiguousarray(rows)
    return rows.view(np.uint32)[np.asarray(donor, np.int64)].view(rows.dtype)


def episodes(done, outcome, ep_return, ep_steps, n_members):
    """-> dict of count int64 [K], outcomes int64 [K, 4], steps int64 [K], return_sum float64 [K] (the exact sum, rounded
    once), abs_sum float64 [K] (the sum of |return|, for the error bound of a double summation in any order)."""
    done = np.asarray(done).astype(bool)
    T, E = done.shape
    K = int(n_members)
    EM = E // K
    out = {"count": np.zeros(K, np.int64), "outcomes": np.zeros((K, 4), np.int64), "steps": np.zeros(K, np.int64),
           "return_sum": np.zeros(K, np.float64), "abs_sum": np.zeros(K, np.float64)}
    for k in range(K):
        sel = done[:, k * EM:(k + 1) * EM]
        r = np.asarray(ep_return)[:, k * EM:(k + 1) * EM][sel].astype(np.float64)
        s = np.asarray(ep_steps)[:, k * EM:(k + 1) * EM][sel].astype(np.int64)
        o = np.asarray(outcome)[:, k * EM:(k + 1) * EM][sel]
        out["count"][k] = sel.sum()
        out["outcomes"][k] = [(o == c).sum() for c in range(4)]
        out["steps"][k] = (s - 1).sum()
        out["return_sum"][k] = math.fsum(r) if np.isfinite(r).all() else r.sum()
        out["abs_sum"][k] = math.fsum(np.abs(r)) if np.isfinite(r).all() else np.inf
    return out
