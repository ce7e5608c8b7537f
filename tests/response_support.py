"""Shared by tests/test_response.py: the flavours of the response model (policy.DelayedDisturbance) and the host loop its
evaluator is held to.

The flavours carry noise_scoring_support's sigmas and rho, so the correlated campaign is theirs at delay 0 and lag 0 and the
shared cache's run serves both files; NOMINAL has zero sigmas, the response alone.

Reference (no new arithmetic, no tolerance): noise_scoring_support.host_loop() itself, handed a view of the package whose
records.disturb_action() first passes the actor's action through a per-env delay queue and records.response_lag_step() -- the
step records.response_lag() scans with -- and then does what it has always done.  host_loop() calls it once per step with the
actions of all envs, every episode starts at the loop's first step, and a latched env's entries are never read, so one queue
of per-step arrays is the per-env queues side by side.  One reference per (flavour, shape), computed once and left unchanged."""
import collections

import numpy as np

import eval_stats_support as ES
import noise_scoring_support as NS
from noise_scoring_support import RHO, SIGMAS, Flavour, correlated_series

ZERO_SIGMAS = dict(sep=0.0, cpa=0.0, closing=0.0, action=0.0, seed=7)


def flavour(name, sigmas=SIGMAS, **response):
    return Flavour(name, lambda g: g.DelayedDisturbance.normalised(**sigmas, **RHO, **response), correlated_series)


DELAY = flavour("delay", delay=3)
LAG = flavour("lag", lag=0.5)
BOTH = flavour("delay-and-lag", delay=5, lag=0.75)
NOMINAL = flavour("nominal-delay", ZERO_SIGMAS, delay=7)
NEUTRAL = flavour("neutral-response")                      # delay 0, lag 0: the correlated entries' results


class _Records:
    """records, with the response in front of disturb_action()."""

    def __init__(self, records, dist):
        self._records, self._dist = records, dist
        self._queue, self._held, self._step = collections.deque(), None, 0

    def __getattr__(self, name):
        return getattr(self._records, name)

    def disturb_action(self, action, s_action, normal):
        action = np.asarray(action, np.float32)
        command = action
        if self._dist.delay > 0:                           # what went in `delay` steps ago comes out; nothing yet: 0
            self._queue.append(action.copy())
            command = self._queue.popleft() if len(self._queue) > self._dist.delay else np.zeros_like(action)
        held = np.zeros_like(action) if self._held is None else self._held
        self._held = self._records.response_lag_step(held, command, self._dist.lag, self._step == 0)
        self._step += 1
        return self._records.disturb_action(self._held, s_action, normal)


class Responding:
    """The package as host_loop() sees it for ONE episode batch under `dist`: everything the package's, but `records`."""

    def __init__(self, g, dist):
        self._g, self.records = g, _Records(g.records, dist)

    def __getattr__(self, name):
        return getattr(self._g, name)


_LOOP = {}


def loop_reference(g, fl, N, group):
    """host_loop()'s rows of eval_stats_support's two policies under the flavour's response at NOISE_EPISODE."""
    key = (fl.name, N, group)
    if key not in _LOOP:
        cfg = ES.config(g, N)
        eps = ES.episodes(cfg)
        dist = fl.disturbance(g)
        _LOOP[key] = [NS.host_loop(Responding(g, dist), cfg, eps, pol, dist, NS.NOISE_EPISODE, group, fl.errors(g, dist, N))
                      for pol in ES.two_policies(g, N)]
    return _LOOP[key]


def without_response(g, fl):
    """The flavour's disturbance with delay 0 and lag 0."""
    d = fl.disturbance(g)
    return type(d).from_dict(dict(d.to_dict(), delay=0, lag=0.0))


def evaluator_equals_the_host_loop(g, fl, shape):
    """Teeth first, on the reference alone: every episode finished, and against the same flavour without delay and lag a float
    statistic moves in at least half of the episodes.  Then the fused evaluator's rows against the loop's, bit for bit."""
    N, group = shape
    rows = loop_reference(g, fl, N, group)
    plain = NS.fused(g, N, group, disturbance=without_response(g, fl), noise_episode=NS.NOISE_EPISODE)
    floats = [k for k in g.records.SAFETY_KEYS if k not in ("min_separation_step", "los_steps")]
    for k, row in enumerate(rows):
        assert (row[0] != 0).all(), "an episode of the reference did not finish"
        moved = np.zeros(ES.E, bool)
        for key in floats:
            moved |= ES.bits(row[4][key]) != ES.bits(plain[key][k])
        print("\n%s %s policy %d: the response moves a float statistic of %d of %d episodes" % (fl.name, NS.shape_id(shape), k,
                                                                                                int(moved.sum()), ES.E))
        assert 2 * int(moved.sum()) >= ES.E, (k, int(moved.sum()))
    got = NS.fused(g, N, group, disturbance=fl.disturbance(g), noise_episode=NS.NOISE_EPISODE)
    for k, (outcome, steps, ret, stats, summary) in enumerate(rows):
        assert np.array_equal(got["outcome"][k], outcome) and np.array_equal(got["steps"][k], steps), k
        assert ES.bits_equal(got["total_reward"][k].astype(np.float32), ret), k
        for key in g.records.SAFETY_KEYS:
            assert ES.bits_equal(got[key][k], summary[key]), (k, key)
