"""Shared by tests/test_eval_stats.py: the hand-placed episodes of the safety-statistics tests and their reference --
the existing per-step path, reduced on the host.

Reference (no new arithmetic, no tolerance): ACAS2DVecEnv.rollout_policy() plays the episodes with the policy (bit-equal
per step to the fused evaluator) and keeps the action of every step; those actions are replayed through the latching
per-step kernel with record_trace=True from the same set_state, the trace columns d_sep / a_lat / d_dev are read after
every step up to each env's first done, and records.episode_safety(dtype=T) reduces them.  One reference per
(dtype, formulation, N), computed once and left unchanged.
"""
import math
from collections import namedtuple

import numpy as np
import torch

DEV = "cuda:0"
E = 70                       # one full wave and a partial one (thread per env); 18 waves of four envs at the (4,16) shape
MAX_STEPS = 120
FAMILIES = ("goal", "collision", "timeout", "goal_receding", "loss_of_separation")

Episodes = namedtuple("Episodes", "own trf goal family")
Reference = namedtuple("Reference", "outcome steps total_reward stats summary")    # [K, E] arrays; stats / summary: dicts of them


def config(g, N, fast=False):
    return g.ACAS2DConfig(n_traffic=N, max_steps=MAX_STEPS, fast_math=fast)


def episodes(cfg, seed=0):
    """E episodes, family i % 5, placed so that the outcome does not depend on what the policy does (the heading changes
    by less than one degree per step):
      goal                10 .. 60 px outside the goal radius, flying at the goal: done within ~30 steps
      collision           one aircraft (slot i % N) head-on, 6 .. 40 px outside the collision distance: done within ~10
      timeout             1 200 px from the goal with max_steps = 120 steps of 2 px
      goal_receding       a goal episode whose traffic all flies away: the minimum separation is its first step row's
      loss_of_separation  a goal episode with one aircraft alongside, between collision and safe distance, never closer
    Everything not placed on purpose lies 500 .. 900 px away, flying radially away, never parallel to the player."""
    rng = np.random.default_rng(seed)
    N = cfg.n_traffic
    gx, gy = cfg.goal
    v, step = float(cfg.airspeed), float(cfg.airspeed) * cfg.dt
    cd, R = 2.0 * cfg.collision_radius, float(cfg.goal_radius)
    own, trf, goal, family = np.zeros((E, 4)), np.zeros((E, N, 4)), np.tile([gx, gy], (E, 1)), []

    def far(x, y):
        out = []
        for _ in range(N):
            th, r = rng.uniform(30.0, 330.0), rng.uniform(500.0, 900.0)
            out.append([x + r * math.cos(math.radians(th)), y + r * math.sin(math.radians(th)),
                        (th + rng.uniform(-10.0, 10.0)) % 360.0, v])
        return out

    for i in range(E):
        fam = FAMILIES[i % len(FAMILIES)]
        family.append(fam)
        y = gy + rng.uniform(-20.0, 20.0)
        if fam == "timeout":
            x = gx - 1200.0 - rng.uniform(0.0, 50.0)
        elif fam == "collision":
            x = gx - 600.0 - rng.uniform(0.0, 50.0)          # the goal is out of reach before the intruder arrives
        elif fam == "loss_of_separation":
            x = gx - R - rng.uniform(10.0, 40.0)
        else:
            x = gx - R - rng.uniform(10.0, 60.0)
        own[i] = [x - step, y, rng.uniform(-2.0, 2.0) % 360.0, v]
        t = far(x, y)
        if fam == "collision":
            t[i % N] = [x + cd + rng.uniform(6.0, 40.0), y + rng.uniform(-5.0, 5.0), 180.0 + rng.uniform(-3.0, 3.0), v]
        elif fam == "loss_of_separation":
            side = 1.0 if i % 2 else -1.0
            t[i % N] = [x + rng.uniform(-10.0, 10.0), y + side * rng.uniform(125.0, 135.0), (side * 3.0) % 360.0, v]
        trf[i] = t
    return Episodes(own, trf, goal, np.array(family))


def two_policies(g, N):
    """Two randomly initialised ActorCritics whose heads are scaled up so that the actions differ and move."""
    pols = []
    for seed in (1, 2):
        torch.manual_seed(seed)
        pol = g.ActorCritic(5 + 3 * N)
        with torch.no_grad():
            pol.action_net.weight.mul_(40.0)
        pols.append(pol)
    return pols


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def trace_reduction(g, cfg, eps, policy, dtype, n_steps, group=False):
    """One policy's reference rows [E]: (outcome, steps, total_reward, stats dict, summary dict), zeros where the episode
    is not done within n_steps."""
    N = cfg.n_traffic
    npdt = np.float32 if dtype == torch.float32 else np.float64
    zero = np.zeros(E, np.int32)
    v = g.ACAS2DVecEnv(E, N, device=DEV, dtype=dtype, auto_reset=True, config=cfg)
    v.set_state(eps.own, eps.trf, eps.goal, zero, observe=True)
    out = v.rollout_policy(policy, n_steps, group=group)
    done = out["done"].cpu().numpy()
    fin, t0, e = done.any(0), done.argmax(0), np.arange(E)
    outcome = np.where(fin, out["outcome"].cpu().numpy()[t0, e], 0).astype(np.uint8)
    steps = np.where(fin, out["episode_steps"].cpu().numpy()[t0, e], 0).astype(np.int32)
    ret = np.where(fin, out["episode_return"].cpu().numpy()[t0, e], 0).astype(npdt)
    # the latching replay with traces: row 0 is the record row of the reset, row t + 1 that of step t
    r = g.ACAS2DVecEnv(E, N, device=DEV, dtype=dtype, auto_reset=False, record_trace=True, config=cfg)
    r.set_state(eps.own, eps.trf, eps.goal, zero, observe=True)
    cols = [r.trace.clone()]
    last = int(t0[fin].max()) if fin.any() else -1
    for t in range(last + 1):
        r.step(out["actions"][t])
        cols.append(r.trace.clone())
    trace = torch.stack(cols).cpu().numpy()                           # [rows, E, 16]
    names = list(g.vec_env.TRACE_COLUMNS)
    c_sep, c_lat, c_dev = names.index("d_sep"), names.index("a_lat"), names.index("d_dev")
    keys = ("min_sep", "min_sep_step", "los_steps", "max_a_lat", "max_dev", "sum_dev")
    ints = ("min_sep_step", "los_steps")
    stats = {k: np.zeros(E, np.int32 if k in ints else npdt) for k in keys}
    summary = {k: np.zeros(E, np.int32 if k in ("min_separation_step", "los_steps") else npdt) for k in g.records.SAFETY_KEYS}
    for i in np.nonzero(fin)[0]:
        n = t0[i] + 2                                                 # row 0 and t0 + 1 step rows
        assert n == steps[i]
        one = g.records.episode_safety(trace[:n, i, c_sep], trace[:n, i, c_lat], trace[:n, i, c_dev], cfg.safe_distance, npdt)
        for k in keys:
            stats[k][i] = one[k]
        for k, val in g.records.safety_summary(one, int(steps[i])).items():
            summary[k][i] = val
    return outcome, steps, ret, stats, summary


_CACHE = {}


def reference(g, dtype, fast, N, n_steps=MAX_STEPS + 1):
    """The reference of K = 2 policies on the E episodes at (dtype, formulation, N), as [2, E] arrays."""
    key = (dtype, fast, N, n_steps)
    if key not in _CACHE:
        cfg = config(g, N, fast)
        eps = episodes(cfg)
        rows = [trace_reduction(g, cfg, eps, pol, dtype, n_steps, group=N > 8) for pol in two_policies(g, N)]
        stack = lambda i: np.stack([r[i] for r in rows])  # noqa: E731
        ref = Reference(stack(0), stack(1), stack(2), {k: np.stack([r[3][k] for r in rows]) for k in rows[0][3]},
                        {k: np.stack([r[4][k] for r in rows]) for k in rows[0][4]})
        for a in (ref.outcome, ref.steps, ref.total_reward, *ref.stats.values(), *ref.summary.values()):
            a.setflags(write=False)
        _CACHE[key] = ref
    return _CACHE[key]
