"""Shared by tests/test_monte_carlo.py and tests/noise_scoring_support.py: the campaign's shapes and its reference -- the
existing entries, folded on the host.

Reference (no new arithmetic, no tolerance): for every episode counter c, ACAS2DVecEnv.reset_to_episode(c) on an n_lanes-env
engine of the campaign's seed, dtype and config draws the encounters, their state is read back, and
evaluate_policies_fused(safety=True) -- the stats evaluator, one episode per lane -- plays them with the K policies;
records.monte_carlo_reduce() folds the per-counter results in counter order.  One reference per shape, computed once for
the most counters any test asks for, and left unchanged."""
from collections import namedtuple

import numpy as np
import torch

from eval_stats_support import DEV, bits_equal, two_policies      # noqa: F401  (bits_equal: for the tests)

LANES = 70                   # one full wave and a partial one (thread per env); 18 waves of four envs at the (4,16) shape
EPISODES = 3
N_BINS = 16
SEED = 13
COUNTERS = 7                 # the first_episode test continues to counter 6

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


def campaign(g, s, pols=None, lanes=LANES, **kw):
    return g.MonteCarlo(policies(g, s) if pols is None else pols, lanes, seed=SEED, dtype=s.dtype, group=s.group,
                        config=config(g, s), n_bins=N_BINS, device=DEV, **kw)


def inv_bin_width(g, s):
    return N_BINS / (4.0 * config(g, s).safe_distance)


_RESULTS = {}


def per_counter(g, s, fl=None):
    """The stats evaluator's result dicts of [a, b, zero] for counters 0 .. COUNTERS - 1 at shape s.  fl (a
    noise_scoring_support.Flavour): the noisy evaluator's under fl.disturbance(g), counter c with the noise of episode c,
    for counters 0 .. EPISODES - 1."""
    key = (fl and fl.name, s)
    if key not in _RESULTS:
        cfg = config(g, s)
        v = g.ACAS2DVecEnv(LANES, s.N, device=DEV, dtype=s.dtype, seed=SEED, config=cfg)
        out = []
        for c in range(EPISODES if fl else COUNTERS):
            v.reset_to_episode(c)
            own, trf, goal = g.policy.read_state(v)
            res = g.evaluate_policies_fused(policies(g, s), own, trf, goal, dtype=s.dtype, device=DEV, config=cfg, group=s.group,
                                            safety=True, disturbance=fl and fl.disturbance(g), noise_episode=c)
            for a in res.values():
                a.setflags(write=False)
            out.append(res)
        _RESULTS[key] = out
    return _RESULTS[key]


def reference(g, s, counters=EPISODES, rows=None):
    """The accumulators of counters 0 .. counters - 1, for all three policies or the rows named."""
    res = per_counter(g, s)[:counters]
    if rows is not None:
        res = [{k: v[list(rows)] for k, v in r.items() if np.ndim(v) == 2} for r in res]
    return g.records.monte_carlo_reduce(res, N_BINS, inv_bin_width(g, s), npdt(s))


def mismatches(g, got, want):
    """The accumulators that differ: integers exactly, the four per-lane arrays by bit pattern."""
    return [k for k in g.records.MONTE_CARLO_KEYS if not bits_equal(got[k], want[k])]
