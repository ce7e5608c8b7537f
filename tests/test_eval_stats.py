"""Per-episode safety statistics from the fused evaluator (acas2d_evaluate_policies_stats_*,
evaluate_policies_fused(safety=True)) on the GPU: all six outputs equal, bit for bit, the reduction of the latching
kernel's trace rows over the same actions (tests/eval_stats_support.py: no new arithmetic, no tolerance), and outcome /
steps / total_reward equal the plain entry point's.  K = 2 policies (the wave-uniform policy switch), E = 70 hand-placed
episodes (a full wave, a partial one and padding lanes), ~120 steps, every kind of work shape of the new kernels."""
import numpy as np
import pytest
import torch

import eval_stats_support as S

pytestmark = pytest.mark.gpu

# (dtype, fast formulation, N, group): thread-per-env float32, the group shapes (4,2) (4,4) (4,16), float64 in both formulations
SHAPES = (("float32", True, 1, False), ("float32", True, 3, False), ("float32", True, 8, False),
          ("float32", True, 8, True), ("float32", True, 16, True), ("float32", True, 64, True),
          ("float64", False, 1, False), ("float64", False, 3, False), ("float64", True, 3, False))
IDS = ["%s%s-N%d%s" % (d, "fast" if (f and d == "float64") else "", n, "-group" if grp else "") for d, f, n, grp in SHAPES]
STATS = {"min_separation": "min_sep", "min_separation_step": "min_sep_step", "los_steps": "los_steps",
         "max_abs_a_lat": "max_a_lat", "max_abs_deviation": "max_dev"}


@pytest.fixture(scope="module")
def g():
    import gym_acas2d_amd as g
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    g.native.lib()
    return g


_RUNS = {}


def _fused(g, shape, safety=True, max_steps=None, policies=slice(None)):
    """evaluate_policies_fused on the support module's episodes and policies (the full two-policy safety run is kept)."""
    dtype, fast, N, group = shape
    key = (shape, safety, max_steps, (policies.start, policies.stop))
    if key not in _RUNS:
        cfg = S.config(g, N, fast)
        eps = S.episodes(cfg)
        _RUNS[key] = g.evaluate_policies_fused(S.two_policies(g, N)[policies], eps.own, eps.trf, eps.goal,
                                               dtype=getattr(torch, dtype), config=cfg, group=group, safety=safety,
                                               max_steps=max_steps)
    return _RUNS[key]


def _assert_equal_reference(got, ref, rows=slice(None)):
    assert np.array_equal(got["outcome"], ref.outcome[rows]) and np.array_equal(got["steps"], ref.steps[rows])
    assert S.bits_equal(got["total_reward"], ref.total_reward[rows].astype(np.float64))
    for key, name in STATS.items():
        assert S.bits_equal(got[key], ref.stats[name][rows]), key
        assert S.bits_equal(got[key], ref.summary[key][rows]), key
    assert S.bits_equal(got["mean_abs_deviation"], ref.summary["mean_abs_deviation"][rows])
    # the sum itself, from the mean's two operands: sum / (steps - 1) in T is what both sides computed
    rows_f = np.maximum(ref.steps[rows] - 1, 1).astype(ref.stats["sum_dev"].dtype)
    assert S.bits_equal(got["mean_abs_deviation"], np.where(ref.steps[rows] > 1, ref.stats["sum_dev"][rows] / rows_f, 0)
                        .astype(rows_f.dtype))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_safety_statistics_equal_the_trace_reduction(g, shape):
    dtype, fast, N, group = shape
    ref = S.reference(g, getattr(torch, dtype), fast, N)
    got = _fused(g, shape)
    npdt = np.dtype(dtype)
    for key in g.records.SAFETY_KEYS:
        assert got[key].shape == (2, S.E), key
        assert got[key].dtype == (np.int32 if key in ("min_separation_step", "los_steps") else npdt), key
    _assert_equal_reference(got, ref)
    # outcome / steps / total_reward: the plain entry point's, bit for bit
    plain = _fused(g, shape, safety=False)
    assert set(got) - set(plain) == set(g.records.SAFETY_KEYS)
    for key in ("outcome", "steps", "unfinished", "path_length"):
        assert np.array_equal(got[key], plain[key]), key
    assert S.bits_equal(got["total_reward"], plain["total_reward"])
    # the episodes hold what they were placed for, for both policies, and the two policies do play differently
    fam = S.episodes(S.config(g, N, fast)).family
    assert (got["unfinished"] == 0).all()
    for k in range(2):
        oc, st = got["outcome"][k], got["steps"][k]
        assert (oc[fam == "collision"] == 2).all() and (oc[fam == "timeout"] == 3).all()
        assert (oc[fam == "goal"] == 1).any() and (st[fam == "timeout"] == S.MAX_STEPS + 1).all()
        assert (got["min_separation_step"][k][fam == "goal_receding"] == 1).any()
        los = got["los_steps"][k]
        assert ((los > 0) & (oc != 2) & (fam == "loss_of_separation")).any()
        assert (los[fam == "loss_of_separation"] == st[fam == "loss_of_separation"] - 1).any()   # every step row inside
        assert (los[fam == "timeout"] == 0).all()
        coll = fam == "collision"                                       # a collision's closest row is its last one
        assert (got["min_separation_step"][k][coll] == st[coll] - 1).all()
        # d_sep is taken before the traffic moves, the collision found after: one traffic step (2 px) above the threshold at most
        cfg = S.config(g, N)
        assert (got["min_separation"][k][coll] < 2 * cfg.collision_radius + cfg.airspeed * cfg.dt).all()
        assert (got["max_abs_a_lat"][k] <= np.float64(S.config(g, N).acc_lat_limit) * (1 + 1e-6)).all()
        assert (got["max_abs_a_lat"][k] > 0).all() and (got["max_abs_deviation"][k] > 0).all()
        assert (got["mean_abs_deviation"][k] <= got["max_abs_deviation"][k]).all()
    assert not np.array_equal(S.bits(got["max_abs_a_lat"][0]), S.bits(got["max_abs_a_lat"][1]))
    print("%s: %d episodes x 2 policies equal the trace reduction; steps %d..%d, min separation %.3f..%.3f"
          % (IDS[SHAPES.index(shape)], S.E, got["steps"].min(), got["steps"].max(), got["min_separation"].min(),
             got["min_separation"].max()))


def test_thread_per_env_and_group_agree_at_eight_aircraft(g):
    a, b = _fused(g, SHAPES[2]), _fused(g, SHAPES[3])
    assert SHAPES[2][2:] == (8, False) and SHAPES[3][2:] == (8, True)
    for key in ("outcome", "steps", "total_reward") + tuple(g.records.SAFETY_KEYS):
        assert S.bits_equal(a[key], b[key]), key


SHORT = (SHAPES[1], SHAPES[4], SHAPES[7])                   # float32 N = 3, group N = 16, float64 N = 3


@pytest.mark.parametrize("shape", SHORT, ids=[IDS[SHAPES.index(s)] for s in SHORT])
def test_unfinished_episodes_get_zeros(g, shape):
    """A budget of 40 steps: all-zero rows for the episodes not done by then, unchanged rows for the others."""
    dtype, fast, N, group = shape
    full = _fused(g, shape)
    short = _fused(g, shape, max_steps=39)                   # n_steps = max_steps + 1 = 40
    late = full["steps"] > 41                                # done at step t (0-based) has steps = t + 2
    assert np.array_equal(short["outcome"] == 0, late) and late.any() and (~late).any()
    assert np.array_equal(short["unfinished"], late.sum(1))
    for key in ("outcome", "steps", "total_reward") + tuple(g.records.SAFETY_KEYS):
        assert short[key].dtype == full[key].dtype, key
        assert not S.bits(short[key][late]).any(), key       # zeros, +0.0 in the float outputs
        assert S.bits_equal(short[key][~late], full[key][~late]), key
    _assert_equal_reference(short, S.reference(g, getattr(torch, dtype), fast, N, n_steps=40))


@pytest.mark.parametrize("shape", SHORT[:2], ids=[IDS[SHAPES.index(s)] for s in SHORT[:2]])
def test_repeatable_and_independent_of_the_policy_count(g, shape):
    """The same launch twice gives the same bits, and a policy's rows do not depend on K: each policy alone (K = 1)
    against its row of the K = 2 launch."""
    dtype, fast, N, group = shape
    both = _fused(g, shape)
    cfg = S.config(g, N, fast)
    eps = S.episodes(cfg)
    again = g.evaluate_policies_fused(S.two_policies(g, N), eps.own, eps.trf, eps.goal, dtype=getattr(torch, dtype),
                                      config=cfg, group=group, safety=True)
    keys = ("outcome", "steps", "total_reward") + tuple(g.records.SAFETY_KEYS)
    for key in keys:
        assert S.bits_equal(again[key], both[key]), key
    for k in range(2):
        alone = _fused(g, shape, policies=slice(k, k + 1))
        for key in keys:
            assert alone[key].shape == (1, S.E) and S.bits_equal(alone[key][0], both[key][k]), (k, key)
