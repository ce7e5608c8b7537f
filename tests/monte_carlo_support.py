"""Shared by tests/test_monte_carlo.py and tests/noise_scoring_support.py: the campaign's shapes and its reference -- the
existing entries, folded on the host.

Reference (no new arithmetic, no tolerance): for every episode counter c, ACAS2DVecEnv.reset_to_episode(c) on an n_lanes-env
engine of the campaign's seed, dtype and config draws the encounters, their state is read back, and
evaluate_policies_fused(safety=True) -- the stats evaluator, one episode per lane -- plays them with the K policies;
records.monte_carlo_reduce() folds the per-counter results in counter order.  One reference per shape, computed once for
the most counters any test asks for, and left unchanged."""
from collections import namedtuple

import fractions

import numpy as np
import pytest
import torch

import helpers as H
from eval_stats_support import DEV, bits_equal, two_policies      # noqa: F401  (bits_equal: for the tests)

LANES = 70                   # one full wave and a partial one (thread per env); 18 waves of four envs at the (4,16) shape
EPISODES = 3
N_BINS = 16
SEED = 13
COUNTERS = 7                 # the first_episode test continues to counter 6

# ---- wide keys ---------------------------------------------------------------------------------------------------------------------------
# The campaign forms its own RNG lane (env_offset + the index within the policy's block, 64 bits) and counts its own episodes
# (32 bits); the noisy kernels form the noise lane the same way.  At seed 13, offset 0 and counters 0 .. 6 the high word of
# the lane, the high word of the seed and the top of the counter are all 0 or trivial.  These keys make every one of them
# matter: a seed whose halves are non-zero and distinct (helpers.WIDE_SEED), an env_offset that puts the 2^32 crossing of the
# lane at local lane 37 of the 70 -- neither the first nor the last env of its wave at 64, 32, 16, 8 or 4 envs per wave
# (tests/test_monte_carlo_host.py holds every shape used to that) --, and a first counter whose launch ends at 2^32 - 1.
WIDE_CROSSING = 37
WIDE_LANE_OFFSET = 2 ** 32 - WIDE_CROSSING
WIDE_SEED = H.WIDE_SEED
WIDE_FIRST_EPISODE = 2 ** 32 - EPISODES
WIDE = dict(seed=WIDE_SEED, env_offset=WIDE_LANE_OFFSET, first_episode=WIDE_FIRST_EPISODE)
# the same seed and counters at the lane a kernel that dropped the high word would form for the local lanes >= 37: lane
# l - 37 of env_offset 0
TRUNCATED = dict(WIDE, env_offset=0)

Shape = namedtuple("Shape", "dtype fast N group max_steps")
F32, F64 = torch.float32, torch.float64
_BASE = ([(F32, True, n, False) for n in (1, 3, 8)] + [(F64, False, 1, False), (F64, True, 1, False), (F64, False, 4, False)] +
         [(F32, True, n, True) for n in (8, 16, 64)])
# every shape under the default config (max_steps 1000) and under one whose episodes also end by timeout
SHAPES = [Shape(*b, max_steps) for max_steps in (1000, 150) for b in _BASE]
# the float32 work shapes _BASE leaves out -- (2,1), (4,1) and (4,8) -- for the equality with the reference alone, under the
# short config (_BASE feeds every property test twice)
MORE_SHAPES = [Shape(F32, True, n, grp, 150) for n, grp in ((2, False), (4, False), (32, True))]


def shape_id(s):
    return "%s%s-N%d%s%s" % ("f32" if s.dtype == F32 else "f64", "" if s.dtype == F32 else ("-fast" if s.fast else "-exact"), s.N,
                             "-group" if s.group else "", "" if s.max_steps == 1000 else "-T%d" % s.max_steps)


def config(g, s):
    return g.ACAS2DConfig(n_traffic=s.N, max_steps=s.max_steps, fast_math=s.fast)


def npdt(s):
    return np.float32 if s.dtype == F32 else np.float64


def zero_policy(N):
    """baseline_main.py's constant action [0] as a policy: all-zero weights (w1, b1, w2, b2, w3, b3 in torch's layout)."""
    D = 5 + 3 * N
    return (torch.zeros(64, D), torch.zeros(64), torch.zeros(64, 64), torch.zeros(64), torch.zeros(1, 64), torch.zeros(1))


def policies(g, s):
    """[a, b, zero]: eval_stats_support's two policies and the unequipped aircraft."""
    return two_policies(g, s.N) + [zero_policy(s.N)]


def campaign(g, s, pols=None, lanes=LANES, seed=SEED, env_offset=0, first_episode=0, n_bins=N_BINS, **kw):
    """A fresh campaign at shape s.  first_episode: moved to that counter through the public route, a state_dict()."""
    mc = g.MonteCarlo(policies(g, s) if pols is None else pols, lanes, seed=seed, dtype=s.dtype, group=s.group,
                      config=config(g, s), n_bins=n_bins, device=DEV, env_offset=env_offset, **kw)
    if first_episode:
        sd = mc.state_dict()
        sd["first_episode"] = first_episode
        mc.load_state_dict(sd)
        assert mc.first_episode == first_episode
    return mc


def inv_bin_width(g, s, n_bins=N_BINS, hist_max=None):
    """n_bins / hist_max as policy.MonteCarlo forms it (default hist_max: 4 x the safe distance)."""
    return n_bins / float(4.0 * config(g, s).safe_distance if hist_max is None else hist_max)


_RESULTS = {}


def per_counter(g, s, fl=None, seed=SEED, env_offset=0, first_episode=0, lanes=LANES):
    """The stats evaluator's result dicts of [a, b, zero] for counters 0 .. COUNTERS - 1 at shape s.  fl (a
    noise_scoring_support.Flavour): the noisy evaluator's under fl.disturbance(g), counter c with the noise of episode c,
    for counters 0 .. EPISODES - 1.  At other keys or lane counts: counters first_episode .. first_episode + EPISODES - 1
    of the lanes env_offset .. env_offset + lanes - 1 under `seed`."""
    key = (fl and fl.name, s) + (() if (seed, env_offset, first_episode, lanes) == (SEED, 0, 0, LANES) else
                                 (seed, env_offset, first_episode, lanes))
    if key not in _RESULTS:
        cfg = config(g, s)
        v = g.ACAS2DVecEnv(lanes, s.N, device=DEV, dtype=s.dtype, seed=seed, env_offset=env_offset, config=cfg)
        out = []
        for c in range(first_episode, first_episode + (EPISODES if fl or len(key) > 2 else COUNTERS)):
            v.reset_to_episode(c)
            own, trf, goal = g.policy.read_state(v)
            res = g.evaluate_policies_fused(policies(g, s), own, trf, goal, dtype=s.dtype, device=DEV, config=cfg, group=s.group,
                                            safety=True, disturbance=fl and fl.disturbance(g), noise_episode=c, env_offset=env_offset)
            for a in res.values():
                a.setflags(write=False)
            out.append(res)
        _RESULTS[key] = out
    return _RESULTS[key]


def reference(g, s, counters=EPISODES, rows=None, fl=None, n_bins=N_BINS, hist_max=None, seed=SEED, env_offset=0, first_episode=0,
              lanes=LANES):
    """The accumulators of counters first_episode .. first_episode + counters - 1, for all three policies or the rows named,
    under the histogram (n_bins, hist_max)."""
    res = per_counter(g, s, fl, seed, env_offset, first_episode, lanes)[:counters]
    if rows is not None:
        res = [{k: v[list(rows)] for k, v in r.items() if np.ndim(v) == 2} for r in res]
    return g.records.monte_carlo_reduce(res, n_bins, inv_bin_width(g, s, n_bins, hist_max), npdt(s), first_episode=first_episode)


def mismatches(g, got, want):
    """The accumulators that differ: integers exactly, the four per-lane arrays by bit pattern."""
    return [k for k in g.records.MONTE_CARLO_KEYS if not bits_equal(got[k], want[k])]


def same(g, got, want):
    bad = mismatches(g, got, want)
    assert not bad, {k: (np.asarray(got[k]).ravel()[:6], np.asarray(want[k]).ravel()[:6]) for k in bad}


# ---- the histogram rule ------------------------------------------------------------------------------------------------------------------
def edge_hist_max(min_sep, n_bins, dtype):
    """A hist_max (a double) at which the bin of `min_sep` depends on the precision of the product: with
    inv = dtype(n_bins / hist_max) -- what the kernel multiplies by -- min_sep * inv evaluated in `dtype` is exactly a bin
    edge j (1 <= j < n_bins) while the exact product lies below it, and min_sep < hist_max.  Searched over the bins and the
    few representable values around dtype(j) / min_sep; raises if there is none."""
    dt = np.dtype(dtype).type
    m = dt(min_sep)
    exact = fractions.Fraction(float(m))
    for j in range(1, n_bins):
        c = dt(j) / m
        cands = [c]
        for _ in range(4):
            cands = [np.nextafter(cands[0], dt(-np.inf))] + cands + [np.nextafter(cands[-1], dt(np.inf))]
        for inv in cands:
            hist_max = n_bins / float(inv)
            if dt(n_bins / hist_max) == inv and float(m) < hist_max and m * inv == dt(j) and exact * fractions.Fraction(float(inv)) < j:
                return hist_max
    raise ValueError("no bin width of %d bins puts %r on a rounded edge in %s" % (n_bins, min_sep, np.dtype(dtype).name))


def exact_bins(min_sep, n_bins, inv_bin_width, dtype):
    """records.separation_bin() of finite separations with the product in exact arithmetic: inv_bin_width rounded to
    `dtype`, as the kernel reads it, and then no rounding."""
    inv = fractions.Fraction(float(np.dtype(dtype).type(inv_bin_width)))
    flat = [min(max(int(fractions.Fraction(float(x)) * inv), 0), n_bins - 1) for x in np.asarray(min_sep, dtype).ravel()]
    return np.asarray(flat, np.int64).reshape(np.shape(min_sep))


def edge_separation(g, s, n_bins):
    """(m, edge_hist_max(m, n_bins)): m the median finite min_separation (an element, not a mean of two) of policy row 0 over
    counters 0 .. EPISODES - 1.  Not every value has such a width (of 1 000 random values in [50, 1500], 30 in float32 and 38 in float64 have none at 16 bins): then its nearest
    neighbours in the sorted separations are tried, below first -- edge_hist_max() itself never falls back."""
    m = np.sort(np.concatenate([r["min_separation"][0] for r in per_counter(g, s)[:EPISODES]]))
    m = m[np.isfinite(m)]
    mid = len(m) // 2
    for i in sorted(range(len(m)), key=lambda i: (abs(i - mid), i)):
        try:
            return m[i], edge_hist_max(m[i], n_bins, npdt(s))
        except ValueError:
            pass
    raise ValueError("no separation of %s has a bin width with a rounding edge" % shape_id(s))


# ---- a campaign at the wide keys ---------------------------------------------------------------------------------------------------------
FLOAT_LANE_KEYS = ("lane_return_sum", "lane_return_sq", "lane_worst_sep")


def envs_per_wave(s):
    """Envs (campaign lanes, episodes) a wave of the policy kernels holds at (n_traffic, group): thread per env 64; the group
    shapes are (4, N / 4) -- four aircraft per lane, N / 4 lanes per env."""
    N, group = (s.N, s.group) if hasattr(s, "group") else s
    return 64 // (N // 4) if group else 64


def campaign_at_wide_keys(g, s, fl=None, default=None):
    """The campaign of [a, b, zero] at WIDE against reference() at WIDE, and what a campaign is used for there.  fl: the
    noisy campaign under fl.disturbance(g) (a flavour at WIDE_SEED), `default` the flavour of the default-key reference.
    Teeth first, on the reference alone: the float per-lane arrays are not those of the default keys, and in the lanes >= 37
    not those of the lane a truncated index names (TRUNCATED's lane l - 37)."""
    kw = {} if fl is None else {"disturbance": fl.disturbance(g)}
    ref = reference(g, s, fl=fl, **WIDE)
    assert ref["outcome_count"].sum(1).tolist() == ref["sep_hist"].sum(1).tolist() == [LANES * EPISODES] * 3
    plain, cut = reference(g, s, fl=default), reference(g, s, fl=fl, **TRUNCATED)
    for k in FLOAT_LANE_KEYS:
        assert not bits_equal(ref[k], plain[k]), k
        assert not bits_equal(ref[k][:, WIDE_CROSSING:], cut[k][:, :LANES - WIDE_CROSSING]), k
        assert not bits_equal(ref[k][:, :WIDE_CROSSING], cut[k][:, :WIDE_CROSSING]), k           # (nor is the offset ignored)
    # the campaign
    mc = campaign(g, s, **WIDE, **kw).run(EPISODES)
    acc = mc.accumulators()
    same(g, acc, ref)
    finite = np.isfinite(acc["lane_worst_sep"])
    assert finite.any() and acc["lane_worst_episode"].dtype == np.uint32
    assert (acc["lane_worst_episode"][finite] >= 2 ** 32 - EPISODES).all()
    same(g, campaign(g, s, **WIDE, **kw).run(2).run(1).accumulators(), acc)
    # the closest encounter of every policy, and the lanes on both sides of the crossing, regenerated and replayed
    for k, top in enumerate(mc.worst(1)):
        for lane in (top[0][0], WIDE_CROSSING - 1, WIDE_CROSSING):
            counter, sep = int(acc["lane_worst_episode"][k, lane]), acc["lane_worst_sep"][k, lane]
            if lane == top[0][0]:
                assert (lane, counter, sep) == top[0] and sep == acc["lane_worst_sep"][k].min()
            enc = mc.encounter(lane, counter)
            replay = {} if fl is None else enc[3]
            if fl is not None:
                assert replay == {"disturbance": fl.disturbance(g), "noise_episode": counter, "env_offset": WIDE_LANE_OFFSET + lane}
            res = g.evaluate_policies_fused(policies(g, s), *enc[:3], dtype=s.dtype, device=DEV, config=config(g, s), group=s.group,
                                            safety=True, **replay)
            assert bits_equal(res["min_separation"][k, :1], np.asarray([sep], npdt(s))), (k, lane)
    # the counter is spent: 2^32 names no episode, and the refusal leaves the campaign alone
    assert mc.first_episode == 2 ** 32
    with pytest.raises((ValueError, RuntimeError)):
        mc.run(1)
    assert mc.first_episode == 2 ** 32
    same(g, mc.accumulators(), acc)
