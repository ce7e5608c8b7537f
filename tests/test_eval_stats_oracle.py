"""Per-episode safety statistics of the fused evaluator (evaluate_policies_fused(safety=True)) on the GPU against a
reference with no project kernel in it: the float64 CPU oracle stepped over the same scenes and actions, its rows reduced
by records.episode_safety (tests/safety_ref.py; the scenes are held to their labels by tests/test_safety_scenes.py).
tests/test_eval_stats.py stays the bit-for-bit check of the reduction; this file is the check of the arithmetic: which
aircraft, which lane, which vector element, which moment of the step and which threshold the kernels take.

Every shape the entry points ship, K = 4 policies per launch (three constant-action ones, known without any kernel, and a
random one whose actions ACAS2DVecEnv.rollout_policy() supplies at the dtype under test), E = 89 scenes.  outcome / steps
equal the oracle's, max_abs_a_lat is bit-equal to max |T(action) * T(acc_lat_limit)|, min_separation / max_abs_deviation /
mean_abs_deviation lie within B, min_separation_step is a row within 2 B of the reference minimum, los_steps lies between
the reference counts at safe_distance -+ B; the tie / threshold / NaN scenes are asserted exactly.  B per build: see
tests/safety_ref.py, which also quotes what an MI355X measured."""
import numpy as np
import pytest
import torch

import helpers as H
import safety_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (dtype, FAST formulation, N, group, config)
SHAPES = tuple(("float32", True, N, False, "default") for N in (1, 2, 3, 4, 8)) + \
    tuple(("float32", True, N, True, "default") for N in (8, 16, 32, 64)) + \
    tuple(("float64", False, N, False, "default") for N in (1, 2, 3, 4)) + \
    tuple(("float64", True, N, False, "default") for N in (1, 4)) + \
    (("float32", True, 3, False, "small"), ("float32", True, 16, True, "small"), ("float64", False, 3, False, "small"))


def _build(shape):
    return "float64fast" if (shape[0] == "float64" and shape[1]) else shape[0]


def _id(shape):
    return "%s-N%d%s%s" % (_build(shape), shape[2], "-group" if shape[3] else "", "" if shape[4] == "default" else "-" + shape[4])


@pytest.fixture(scope="module")
def g():
    import gym_acas2d_amd as g
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    g.native.lib()
    return g


@pytest.fixture(autouse=True)
def _default_work_shape(monkeypatch):
    monkeypatch.delenv("ACAS2D_SHAPE", raising=False)


_RUNS = {}


def _run(g, O, shape):
    """One launch per shape and its reference: (cfg, scenes, reference, B, D, evaluate_policies_fused's dict)."""
    if shape not in _RUNS:
        dtype, fast, N, group, name = shape
        tdt, npdt = getattr(torch, dtype), np.dtype(dtype).type
        cfg = S.config(g, N, name, fast)
        sc = S.scenes(S.config(g, N, name), O)
        E, T = len(sc.family), cfg.max_steps + 1
        pols = S.policies(g, N)
        # the random policy's actions, from the per-step path at the dtype under test
        v = g.ACAS2DVecEnv(E, N, device=DEV, dtype=tdt, auto_reset=True, config=cfg)
        v.set_state(sc.own.copy(), sc.trf.copy(), sc.goal.copy(), np.zeros(E, np.int32), observe=True)
        played = v.rollout_policy(pols[-1], T, group=group)["actions"].cpu().numpy().astype(np.float64)
        assert ((np.abs(played) <= 1) | np.isnan(played)).all() and np.isnan(played[:cfg.max_steps, sc.family == "nan"]).all()
        actions = np.stack([S.constant_actions(sc, b, T) for b in S.CONST_BIAS] + [played])
        ref = S.reference(O, H, g, cfg, sc, actions)
        D = S.drift(O, H, cfg, sc, actions, ref) if dtype == "float32" else None
        B = S.bound(H, _build(shape), cfg.max_steps, ref.extent, D)
        got = g.evaluate_policies_fused(pols, sc.own, sc.trf, sc.goal, dtype=tdt, device=DEV, config=cfg, group=group,
                                        safety=True)
        _RUNS[shape] = (cfg, sc, ref, B, D, got, npdt)
    return _RUNS[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=[_id(s) for s in SHAPES])
def test_safety_statistics_against_the_oracle(g, oracle_mod, shape):
    cfg, sc, ref, B, D, got, npdt = _run(g, oracle_mod, shape)
    for key in g.records.SAFETY_KEYS:
        assert got[key].shape == (S.K, len(sc.family)), key
    # the random policy does play: its actions move, and differ between episodes
    moving = ref.actions[3][:5, sc.family == "nearest"]
    assert len(np.unique(moving)) > 5
    err = S.compare(got, ref, cfg, B, npdt)
    print("%s: worst error min_separation %.3e, max_abs_deviation %.3e, mean_abs_deviation %.3e px; B = %.4e px%s; "
          "max_abs_a_lat bit-equal; of %d episodes %d have one candidate row, %d one loss-of-separation count; least "
          "threshold margin under the random policy %.3f px"
          % (_id(shape), err["min_separation"], err["max_abs_deviation"], err["mean_abs_deviation"], B,
             "" if D is None else " (D = %.3e px, extent %.0f px)" % (D, ref.extent), err["episodes"], err["unique"],
             err["same_los"], np.nanmin(ref.margin[3])))
    S.assert_exact_scenes(got, sc, cfg, npdt)
    # what the scenes were placed for did happen on the device
    fam = sc.family
    for k in range(S.K):
        near = fam == "nearest"
        assert (got["los_steps"][k][near] == got["steps"][k][near] - 1).all()
        assert (got["min_separation_step"][k][fam == "receding"] == 1).all()
        coll = fam == "collision"
        assert (got["min_separation_step"][k][coll] == got["steps"][k][coll] - 1).all()
        assert (got["steps"][k][np.isin(fam, ("first_goal", "first_collision"))] == 2).all()
    assert (got["max_abs_a_lat"][0][fam != "nan"] == 0).all()                   # b = 0: a zero maximum


TRACED = (SHAPES[4], SHAPES[8], SHAPES[12])       # float32 N = 8 thread per env, float32 group N = 64, float64 exact N = 4


@pytest.mark.parametrize("shape", TRACED, ids=[_id(s) for s in TRACED])
def test_trace_columns_against_the_oracle(g, oracle_mod, monkeypatch, shape):
    """The d_sep / a_lat / d_dev trace columns of the latching per-step kernel -- what tests/test_eval_stats.py reduces as
    its reference -- row by row up to each env's first done, under the b = 0.375 policy's actions: within the same B of the
    reference's rows, a_lat exactly.  A failure above that does not show here lies in the reduction, not in the step."""
    dtype, fast, N, group, name = shape
    assert (dtype, N, group) in (("float32", 8, False), ("float32", 64, True), ("float64", 4, False))
    cfg, sc, ref, B, D, got, npdt = _run(g, oracle_mod, shape)
    tdt, E = getattr(torch, dtype), len(sc.family)
    if N == 8:                                     # one lane per env, eight aircraft per lane -- read at every launch
        monkeypatch.setenv("ACAS2D_SHAPE", "8,1")
    geo = g.native.launch_geometry(E, N, np.dtype(dtype).itemsize)
    assert (geo["traffic_per_lane"], geo["lanes_per_env"]) == {8: (8, 1), 64: (4, 16), 4: (4, 1)}[N]
    k = S.SMOOTH
    r = g.ACAS2DVecEnv(E, N, device=DEV, dtype=tdt, auto_reset=False, record_trace=True, config=cfg)
    r.set_state(sc.own.copy(), sc.trf.copy(), sc.goal.copy(), np.zeros(E, np.int32), observe=True)
    acts = torch.as_tensor(np.array(ref.actions[k]), dtype=tdt, device=DEV)
    rows = [r.trace.clone()]
    for t in range(int(ref.steps[k].max()) - 1):
        r.step(acts[t])
        rows.append(r.trace.clone())
    trace = torch.stack(rows).cpu().numpy().astype(np.float64)                 # [rows, E, 16]: row t + 1 is step t's
    names = list(g.vec_env.TRACE_COLUMNS)
    valid = S.step_rows(ref)[k][:len(rows)]
    worst = {}
    for col, want in (("d_sep", ref.d_sep[k]), ("d_dev", ref.d_dev[k])):
        x, y = trace[:, :, names.index(col)], want[:len(rows)]
        fin = valid & np.isfinite(y)
        assert fin.sum() > 1000 and np.isfinite(x[fin]).all()
        assert not np.isfinite(x[valid & ~fin]).any()                          # the nan scenes: +inf or NaN, never a number
        worst[col] = float(np.abs(x[fin] - y[fin]).max())
        assert worst[col] <= B, (col, worst[col], B)
    a = trace[:, :, names.index("a_lat")]
    want = (ref.actions[k].astype(npdt) * npdt(cfg.acc_lat_limit)).astype(np.float64)[:len(rows) - 1]
    fin = valid[1:] & np.isfinite(want)
    assert np.array_equal(a[1:][fin], want[fin]) and np.isnan(a[1:][valid[1:] & ~fin]).all()
    print("%s trace rows: worst error d_sep %.3e, d_dev %.3e px (B = %.4e px), a_lat exact, %d rows"
          % (_id(shape), worst["d_sep"], worst["d_dev"], B, int(valid.sum())))
