"""GPU parity tests (-m gpu): the HIP path, called through the C ABI (ctypes ->
libacas2d_hip.so), against the CPU oracle and the committed golden vectors.

Tolerances (north star: masks bit-exact, 1e-5 abs on float positions / rewards):
  float64 instantiation -- the parity gate.  Asserted far tighter than required: 1e-9 abs on
      positions, observations, rewards and returns over full episodes; done / outcome / step
      masks bit-exact (cases placed within 1e-9 of a threshold excepted and counted).
  float32 instantiation -- throughput mode.  float32 cannot REPRESENT 1600-px positions or
      +-1000 rewards to 1e-5 (ulp(1024..2048) = 1.2e-4, ulp(1000) = 6.1e-5), so single steps from
      identical (float32-representable) states are held to: observations 1e-5 abs (2e-5 for the
      signed d_cpa entry), non-terminal rewards 1e-5 abs, positions / terminal rewards 1 float32
      ulp (1.3e-4); masks exact outside a 1e-3 band around the thresholds.
  float32 under a non-default configuration (helpers.NONDEFAULT_CONFIGS: "wide", "small") -- the same criteria with the
      bounds derived from the configuration (helpers.f32_bounds): positions 1 ulp of the largest coordinate (2.44e-4
      beyond 2048 px: worst 1.22e-4), fresh speeds (max - min) airspeed 2^-24 + 2 ulp (worst 2.2e-5 of 3.6e-5 under
      "wide", 3.4e-5 of 6.8e-5 under "small"), and the d_cpa entry 2e-5 plus, where speeds differ, the reference's own
      conditioning d (max airspeed 2^-20) / (|v12| d_cpa_max) (worst 2.8e-5, 0.35 of its bound).
"""
import os
import types

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def g():
    import gym_acas2d_amd as g
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    g.native.lib()          # fails loudly if the HIP extension is missing
    return g


@pytest.fixture(scope="module")
def O(oracle_mod):
    return oracle_mod


@pytest.fixture(params=("exact", "fast"))
def math(request):
    """The two formulations of the float64 build (include/acas2d.h, ACAS2D_MATH_*): the reference's operation
    order with libm, and the float32 build's algebraic formulation in float64 arithmetic.  Both are held to the
    same fixtures at the same 1e-9 (the contract asks 1e-5)."""
    return request.param


def bits_equal(x, y):
    """torch.equal on the BIT patterns: the engine reproduces the reference's NaN d_cpa in exact parallel flight
    (kinematics.py:48), which float32 headings hit about once per 4e6 env-steps at N = 8 -- and NaN != NaN."""
    if x.is_floating_point():
        bits = torch.int32 if x.dtype == torch.float32 else torch.int64
        return x.shape == y.shape and torch.equal(x.contiguous().view(bits), y.contiguous().view(bits))
    return torch.equal(x, y)


class GpuEngine:
    """The HIP path behind the OracleEnvs interface (numpy float64 views), see helpers.py."""

    def __init__(self, g, E, N, dtype=None, auto_reset=False, seed=13, env_offset=0, math="exact"):
        self.v = g.ACAS2DVecEnv(E, N, device="cuda:0", dtype=dtype or torch.float64,
                                auto_reset=auto_reset, seed=seed, env_offset=env_offset,
                                config=g.ACAS2DConfig(n_traffic=N, fast_math=(math == "fast")))
        self.E, self.N = E, N

    @staticmethod
    def _np(t):
        return t.detach().cpu().numpy().astype(np.float64) if t.is_floating_point() else t.detach().cpu().numpy()

    def __getattr__(self, name):
        if name in ("own_x", "own_y", "own_psi", "own_v", "goal_x", "goal_y", "trf_x", "trf_y",
                    "trf_psi", "trf_v", "steps", "total_reward", "status"):
            return self._np(getattr(self.v, name))
        if name == "episode":
            return self.v.episode.cpu().numpy().view(np.uint32)
        if name in ("term_obs", "ep_return", "ep_steps"):
            key = {"term_obs": "terminal_observation", "ep_return": "episode_return",
                   "ep_steps": "episode_steps"}[name]
            return self._np(self.v.outputs[key])
        raise AttributeError(name)

    def set_state(self, own, trf, goal=None, steps=None):
        self.v.set_state(own, trf, goal, steps, observe=False)

    def observe(self):
        # observe() on the state as it stands: re-inject it with observe=True
        st = np.stack([self.own_x, self.own_y, self.own_psi, self.own_v], 1)
        tr = np.stack([self.trf_x, self.trf_y, self.trf_psi, self.trf_v], -1)
        go = np.stack([self.goal_x, self.goal_y], 1)
        return self._np(self.v.set_state(st, tr, go, self.steps, observe=True))

    def reset(self):
        return self._np(self.v.reset())

    def step(self, actions):
        obs, rew, done, _ = self.v.step(np.asarray(actions, np.float64))
        out = self.v.outputs
        d = done.cpu().numpy().astype(np.uint8)
        return self._np(obs), self._np(rew), d, out["outcome"].cpu().numpy(), int(d.sum())


def grazing(fx_obs, N, cfg, band):
    """Rows whose post-step geometry lies within `band` of a collision / goal threshold."""
    d_sep = fx_obs[:, 5::3][:, :N] * cfg.d_sep_max
    d_goal = fx_obs[:, 3] * cfg.d_goal_max
    with np.errstate(invalid="ignore"):
        return (np.abs(d_sep - cfg.collision_dist) < band).any(1) | (np.abs(d_goal - cfg.goal_radius) < band)


def _fixture_shapes(dtype):
    """(N, shape) of every work shape with an edge fixture (N in 1, 3, 8, 64); the default shape keeps the id "N".  The
    float64 rows are the same in both formulations: the `math` fixture picks one."""
    rows = [s for s in H.SHAPES if s.dtype == dtype and s.math == ("fast" if dtype == "float32" else "exact")
            and s.n_traffic in (1, 3, 8, 64)]
    return [pytest.param(s.n_traffic, s, id=str(s.n_traffic) if s.override is None else "%d-%s" % (s.n_traffic, s.override))
            for s in rows]


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,shape", _fixture_shapes("float64"))
def test_f64_edge_vectors(g, O, monkeypatch, N, shape, math):
    _use_shape(g, monkeypatch, shape)
    fx = H.load("ref_edge_n%d.npz" % N)
    E = len(fx["action"])
    env = GpuEngine(g, E, N, math=math)
    env.set_state(fx["own"], fx["trf"], fx["goal"], fx["steps"])
    obs, reward, done, outcome, _ = env.step(fx["action"])
    assert np.array_equal(np.isnan(obs), np.isnan(fx["obs"]))
    want = fx["obs"].copy()
    if math == "fast":
        # kinematics.py:47 takes arctan(v12y / v12x): d_cpa changes SIGN with the sign of v12x.  The hand-placed
        # mirror-image headings make the reference's v12x an exact 0 (or +-1 ulp) -- a coin toss of libm's cos that
        # no other sincos reproduces (the float32 tests exclude |v12x| < 0.02 for the same reason); the magnitude
        # still has to match.
        rad = lambda d: d / 360.0 * 2 * np.pi  # noqa: E731
        op, ov = fx["own_out"][:, 2][:, None], fx["own_out"][:, 3][:, None]
        tp, tv = fx["trf_out"][..., 2], fx["trf_out"][..., 3]
        v12x = ov * np.cos(rad(op)) - tv * np.cos(rad(tp))
        coin = np.abs(v12x) < 1e-9
        # The exempt set is pinned by the fixture's own geometry, not by a bound: exactly the hand-placed entries with
        # equal airspeeds whose headings are parallel (psi_t == psi) or mirror images (psi_t + psi == 360) -- 9 entries
        # at N = 1, 16 at N = 3 / 8 / 64 -- and nothing else has |v12x| < 1e-9.
        assert np.array_equal(coin, (tv == ov) & ((tp == op) | (tp + op == 360.0)))
        assert int(coin.sum()) == {1: 9}.get(N, 16)
        flip = coin & (np.sign(obs[:, 6::3][:, :N]) != np.sign(want[:, 6::3][:, :N]))
        want[:, 6::3][:, :N][flip] *= -1.0
    np.testing.assert_allclose(obs, want, rtol=0, atol=1e-9, equal_nan=True)
    np.testing.assert_allclose(reward, fx["reward"], rtol=0, atol=1e-9, equal_nan=True)
    np.testing.assert_allclose(np.stack([env.own_x, env.own_y, env.own_psi, env.own_v], 1),
                               fx["own_out"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(np.stack([env.trf_x, env.trf_y, env.trf_psi, env.trf_v], -1),
                               fx["trf_out"], rtol=0, atol=1e-9)
    assert np.array_equal(env.steps, fx["steps_out"])
    cfgc = O.default_config()
    ok = ~grazing(fx["obs"], N, cfgc, 1e-9)
    assert ok.sum() >= E - 12
    assert np.array_equal(done[ok], fx["done"][ok]) and np.array_equal(outcome[ok], fx["outcome"][ok])
    assert np.array_equal(env.status[ok], fx["outcome"][ok])        # latched (auto_reset off)


@pytest.mark.parametrize("N", (1, 3, 8, 64))
def test_f64_reference_rollouts(g, N, math):
    fx = H.load("ref_rollout_n%d.npz" % N)
    n_ep = len(fx["ep_own"])
    env = GpuEngine(g, n_ep, N, math=math)
    env.set_state(fx["ep_own"], fx["ep_trf"], fx["ep_goal"], np.zeros(n_ep, np.int32))
    np.testing.assert_allclose(env.observe(), fx["ep_obs0"], rtol=0, atol=1e-9)
    res = H.replay_rollout(env, fx)
    assert res["n"] == len(fx["action"])
    assert res["done_mismatch"] == 0 and res["outcome_mismatch"] == 0 and res["steps_mismatch"] == 0
    assert res["pos"] < 1e-9 and res["psi"] < 1e-9 and res["obs"] < 1e-9
    assert res["reward"] < 1e-9 and res["total_reward"] < 1e-8


def test_f64_reference_csv_baseline(g, math):
    """The reference's own golden CSV replayed on the GPU (100 constant-action episodes)."""
    dg = H.load("csv_baseline_digest.npz")
    cfg = g.ACAS2DConfig(n_traffic=1)
    own, trf, goal = H.parity_reset_states(cfg, 13, 2, 100)
    env = GpuEngine(g, 100, 1, math=math)
    env.set_state(own, trf, goal, np.zeros(100, np.int32))
    env.observe()
    out = H.replay_baseline(env, dg, own, trf)
    assert out["unfinished"] == 0
    assert np.array_equal(out["outcome"], dg["outcome"]) and np.array_equal(out["steps"], dg["steps"])
    for k in ("own_sub", "trf_sub", "own_first2", "own_last"):
        np.testing.assert_allclose(out[k], dg[k], rtol=0, atol=1e-9, equal_nan=True)
    assert np.abs(out["total_reward"] - dg["total_reward"]).max() < 1e-8


def test_single_env_adapter_reference_surface(g):
    """ACAS2DEnv: random.seed(13) names the reference's episodes, old gym
    4-tuple API, numpy float64, env.game.* attributes, CSV episode 1 end to end."""
    import random
    random.seed(13)
    env = g.ACAS2DEnv()
    obs = env.reset()
    assert obs.dtype == np.float64 and obs.shape == (8,) and env.observation_space.shape == (8,)
    assert env.action_space.shape == (1,)
    p, t = env.game.player, env.game.traffic[0]
    assert (p.x, p.y, p.v_air) == (48, 500.0, 200) and p.psi == 358.1242450086868
    assert (t.x, t.y, t.v_air) == (1552, 48, 200.0) and t.psi == 136.41722591475224
    want = [0.001, 0.99478957, 0., 0.41314554, 0., 0.26677536, 0.08703283, -0.92934645]
    np.testing.assert_allclose(obs, want, atol=1e-8)
    env.reset()                                 # third game after the seed = CSV episode 1
    total, n = 0.0, 0
    for _ in range(1000):
        o, r, d, info = env.step(np.array([0]))
        assert isinstance(r, float) and isinstance(d, bool) and info == {}
        total += r
        n += 1
        if n == 1:
            assert abs(env.game.path[-1][0] - 49.998468716044925) < 1e-11
            assert abs(env.game.path[-1][1] - 499.92175173490904) < 1e-11
        if d:
            break
    assert env.game.outcome == 2 and g.OUTCOME_NAMES[env.game.outcome] == "Collision"
    assert env.game.steps == 390
    assert abs(env.game.total_reward - (-988.6418379569138)) < 1e-8 and abs(total - env.game.total_reward) < 1e-9
    assert len(env.game.path) == 390 and len(env.game.traffic_paths[0]) == 390
    assert env.game.traffic_paths[0][1] == env.game.traffic_paths[0][0]      # appendix A quirk
    # stepping a finished env: player moves, traffic frozen (game.py:243-245)
    t_before = (env.game.traffic[0].x, env.game.traffic[0].y)
    env.step(np.array([0.0]))
    assert (env.game.traffic[0].x, env.game.traffic[0].y) == t_before


def test_records_in_the_reference_csv_layout(g, tmp_path):
    """baseline_main.simulate() on the adapter: same columns as the reference's CSV, and the first
    episodes agree with it (outcome, steps, return, path)."""
    import csv
    import random
    dg = H.load("csv_baseline_digest.npz")
    random.seed(13)
    env = g.ACAS2DEnv()
    env.reset()                                  # the game check_env consumed (baseline_main.py:22)
    cols = g.records.simulate(env, episodes=3)
    assert tuple(cols) == g.records.BASELINE_COLUMNS and cols["Episode"] == [1, 2, 3]
    for i in range(3):
        assert cols["Outcome"][i] == {1: "Goal", 2: "Collision", 3: "Timeout"}[int(dg["outcome"][i])]
        assert cols["Time Steps"][i] == dg["steps"][i] and len(cols["Path"][i]) == dg["n_points"][i]
        assert abs(cols["Total Reward"][i] - dg["total_reward"][i]) < 1e-8
        np.testing.assert_allclose(cols["Path"][i][:2], dg["own_first2"][i], atol=1e-9)
        np.testing.assert_allclose(cols["Path"][i][-1], dg["own_last"][i], atol=1e-9)
        np.testing.assert_allclose(cols["Traffic Paths"][i][0][:3], dg["trf_first3"][i], atol=1e-9)
    out = tmp_path / "baseline.csv"
    g.records.to_csv(cols, out)
    rows = list(csv.DictReader(open(out)))
    assert list(rows[0]) == list(g.records.BASELINE_COLUMNS) and rows[0]["Outcome"] == "Collision"
    import ast
    assert rows[0]["Path"].startswith("[(48.0, 500.0), (49.99846871604")      # the reference's file: "[(48, 500.0), (49.998468716044925, ..."
    assert len(ast.literal_eval(rows[0]["Path"])) == 390 and len(ast.literal_eval(rows[0]["Traffic Paths"])[0]) == 390


@pytest.mark.parametrize("N", (1, 3))
def test_testing_main_record_columns_vs_reference(g, N, tmp_path):
    """every column testing_main.py:114-138 writes -- Path Length and the thirteen per-step
    record lists ACAS2DGame keeps (game.py:132-160, :231-241, :266-276) -- from the engine's trace rows
    (include/acas2d.h, Acas2dState.trace), against the lists captured from the unmodified reference
    (tests/golden/ref_records_n{N}.npz, oracle/refharness/capture_golden.py capture_records): random-action
    episodes replayed from the captured initial states.  d_sep is the separation AFTER the player moved and
    BEFORE the traffic did (:236-237 vs :243-245), r_step the step reward before the terminal bonuses."""
    fx = H.load("ref_records_n%d.npz" % N)
    env = g.ACAS2DEnv(n_traffic=N)
    n_ep = len(fx["outcome"])
    acts = iter(fx["actions"])
    states = [(fx["own0"][i], fx["trf0"][i], fx["goal0"][i]) for i in range(n_ep)]
    cols = g.records.simulate(env, episodes=n_ep, policy=lambda obs: np.array([next(acts)]), columns="testing",
                              initial_states=states)
    assert tuple(cols) == g.records.TESTING_COLUMNS
    off = fx["off_records"]
    worst = {}
    for i in range(n_ep):
        lo, hi = off[i], off[i + 1]
        assert cols["Outcome"][i] == {1: "Goal", 2: "Collision", 3: "Timeout"}[int(fx["outcome"][i])]
        assert cols["Time Steps"][i] == fx["steps"][i]
        assert abs(cols["Total Reward"][i] - fx["total_reward"][i]) < 1e-8
        assert abs(cols["Path Length"][i] - fx["d_path"][i]) < 1e-9
        np.testing.assert_allclose(np.array(cols["Path"][i]), fx["path"][lo:hi], atol=1e-9, rtol=0)
        np.testing.assert_allclose(np.array(cols["Traffic Paths"][i]).transpose(1, 0, 2), fx["traffic_paths"][lo:hi],
                                   atol=1e-9, rtol=0)
        for col, attr in g.records.TESTING_RECORDS:
            got, want = np.array(cols[col][i]), fx[attr][lo:hi]
            assert got.shape == want.shape, (col, got.shape, want.shape)
            assert np.array_equal(np.isnan(got), np.isnan(want)), col
            err = float(np.nanmax(np.abs(got - want)))
            worst[col] = max(worst.get(col, 0.0), err)
            assert err < 1e-9, (i, col, err)
    assert next(acts, None) is None                              # every recorded action was consumed
    assert worst["a_lat"] == 0.0 and worst["psi"] < 1e-11
    out = tmp_path / "testing.csv"
    g.records.to_csv(cols, out)
    import csv
    csv.field_size_limit(1 << 30)
    rows = list(csv.DictReader(open(out)))
    assert list(rows[0]) == list(g.records.TESTING_COLUMNS) and len(rows) == n_ep


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,shape", _fixture_shapes("float32"))
def test_f32_single_step_vs_f64_oracle(g, O, monkeypatch, N, shape):
    _use_shape(g, monkeypatch, shape)
    fx = H.load("ref_edge_n%d.npz" % N)
    sel = ~np.isnan(fx["obs"]).any(1)
    own = fx["own"][sel].astype(np.float32).astype(np.float64)        # float32-representable inputs
    trf = fx["trf"][sel].astype(np.float32).astype(np.float64)
    act = fx["action"][sel].astype(np.float32).astype(np.float64)
    E = len(act)
    ref = O.OracleEnvs(E, N)
    ref.set_state(own, trf, fx["goal"], fx["steps"][sel])
    o, r, d, oc, _ = ref.step(act)
    env = GpuEngine(g, E, N, dtype=torch.float32)
    env.set_state(own, trf, fx["goal"], fx["steps"][sel])
    obs, rew, done, outcome, _ = env.step(act)
    cfgc = O.default_config()
    ok = ~grazing(o, N, cfgc, 1e-3)
    assert ok.sum() >= E - 30
    assert np.array_equal(done[ok], d[ok]) and np.array_equal(outcome[ok], oc[ok])
    col = np.arange(o.shape[1])
    cpa = (col >= 5) & ((col - 5) % 3 == 1)
    assert np.abs(obs[:, ~cpa] - o[:, ~cpa]).max() < 1e-5
    # d_cpa = d * sin(a_rel - arctan(v12y / v12x)) (kinematics.py:48-49) is ill-conditioned in the
    # reference itself where the relative velocity v12 is tiny (near-parallel flight: float32
    # rounding of 200*cos(psi), ~1.2e-5, turns into an angle error 2.4e-5 / |v12|) and jumps by
    # +-2 d where v12x changes sign.  Entries with |v12| < 2 px/s or |v12x| < 0.02 px/s (of 200)
    # are excluded -- counted: a handful.
    rad = np.deg2rad
    v12x = (ref.own_v * np.cos(rad(ref.own_psi)))[:, None] - ref.trf_v * np.cos(rad(ref.trf_psi))
    v12y = (ref.own_v * np.sin(rad(ref.own_psi)))[:, None] - ref.trf_v * np.sin(rad(ref.trf_psi))
    well = (np.abs(v12x) > 0.02) & (np.hypot(v12x, v12y) > 2.0)
    assert (~well).mean() < 0.01 or (~well).sum() <= 4
    assert np.abs(obs[:, cpa] - o[:, cpa])[well].max() < 2e-5
    ok &= well[:, 0]                                  # the reward reads traffic[0]'s d_cpa
    term = d.astype(bool)
    assert np.abs(rew[ok & ~term] - r[ok & ~term]).max() < 1e-5
    assert np.abs(rew[ok & term] - r[ok & term]).max() <= 1.3e-4          # 1 ulp of float32(1000)
    pos_err = max(np.abs(env.own_x - ref.own_x).max(), np.abs(env.own_y - ref.own_y).max(),
                  np.abs(env.trf_x - ref.trf_x).max(), np.abs(env.trf_y - ref.trf_y).max())
    assert pos_err <= 1.3e-4                                             # 1 ulp of float32(1600)
    assert np.abs(env.own_psi - ref.own_psi).max() <= 3.1e-5             # 1 ulp of float32(360)


@pytest.mark.parametrize("N,shape", _fixture_shapes("float32"))
def test_f32_reproduces_the_reference_nan_pattern(g, monkeypatch, N, shape):
    """Parallel flight (identical heading and speed) makes the reference's relative velocity 0/0:
    d_cpa is NaN (kinematics.py:48) and so is the reward whenever it reads traffic[0]'s d_cpa.  The
    algebraic float32 formulation (0 * inf) must put NaN in exactly the same places."""
    _use_shape(g, monkeypatch, shape)
    fx = H.load("ref_edge_n%d.npz" % N)
    rows = np.isnan(fx["obs"]).any(1)
    assert rows.sum() >= 8
    f32 = lambda a: a.astype(np.float32).astype(np.float64)  # noqa: E731
    env = GpuEngine(g, int(rows.sum()), N, dtype=torch.float32)
    env.set_state(f32(fx["own"][rows]), f32(fx["trf"][rows]), fx["goal"], fx["steps"][rows])
    obs, rew, done, outcome, _ = env.step(f32(fx["action"][rows]))
    assert np.array_equal(np.isnan(obs), np.isnan(fx["obs"][rows]))
    assert np.array_equal(np.isnan(rew), np.isnan(fx["reward"][rows]))
    ok = ~np.isnan(fx["obs"][rows])
    assert np.abs(obs[ok] - fx["obs"][rows][ok]).max() < 2e-5
    # masks: the fixture's boundary rows sit within an ulp of float64 of the 96 px / 144 px
    # thresholds (game.py:291,299) -- float32 inputs cannot represent that, so they are compared
    # only where the reference's own distances clear the threshold by a float32 rounding margin
    clear = ~grazing(fx["obs"][rows], N, g.ACAS2DConfig(n_traffic=N).to_c(), 1e-3)
    assert clear.sum() >= 4
    assert np.array_equal(done[clear], fx["done"][rows][clear])
    assert np.array_equal(outcome[clear], fx["outcome"][rows][clear])


@pytest.mark.parametrize("N", (1, 8))
def test_f32_full_episodes_vs_f64_oracle(g, O, N):
    """Whole episodes in float32 against the float64 oracle on the same actions: rounding
    accumulates (<= ~0.1 px over 1000 steps), so outcomes / lengths may differ only for episodes
    that cross a threshold within that margin.  Reported, and bounded at 2 %."""
    E, T = 512, 1001
    cfg = g.ACAS2DConfig(n_traffic=N)
    own, trf, goal = H.parity_reset_states(cfg, 4242, 0, E)
    rng = np.random.default_rng(5)
    ref = O.OracleEnvs(E, N)
    ref.set_state(own, trf, goal, np.zeros(E, np.int32))
    ref.observe()
    env = GpuEngine(g, E, N, dtype=torch.float32)
    env.set_state(own, trf, goal, np.zeros(E, np.int32))
    env.observe()
    fin_r, fin_g = np.zeros(E, np.int32), np.zeros(E, np.int32)
    oc_r, oc_g = np.zeros(E, np.uint8), np.zeros(E, np.uint8)
    max_pos = 0.0
    for k in range(T):
        a = rng.uniform(-1, 1, E).astype(np.float32).astype(np.float64)
        _, _, d1, o1, _ = ref.step(a)
        _, _, d2, o2, _ = env.step(a)
        new = (fin_r == 0) & (d1 != 0)
        fin_r[new], oc_r[new] = k + 1, o1[new]
        new = (fin_g == 0) & (d2 != 0)
        fin_g[new], oc_g[new] = k + 1, o2[new]
        both = (fin_r == 0) & (fin_g == 0)
        if both.any():
            max_pos = max(max_pos, float(np.abs(env.own_x - ref.own_x)[both].max()),
                          float(np.abs(env.own_y - ref.own_y)[both].max()))
        if (fin_r > 0).all() and (fin_g > 0).all():
            break
    agree = (fin_r == fin_g) & (oc_r == oc_g)
    print("f32 vs f64 episodes N=%d: %d/%d agree, max |dpos| while both running %.3g px" %
          (N, agree.sum(), E, max_pos))
    assert (fin_r > 0).all() and (fin_g > 0).all()
    assert agree.mean() >= 0.98
    assert np.abs(fin_r - fin_g).max() <= 2 or agree.mean() >= 0.98
    assert max_pos < 0.25


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,E,T", ((3, 4096, 60), (8, 2048, 200), (64, 512, 40), (1, 256, 450), (100, 96, 12)))
def test_f64_auto_reset_vs_oracle(g, O, N, E, T, math):
    """VecEnv semantics and the device Philox reset against the oracle, env-for-env: same seed
    => same episodes, bit-exact reset states, terminal obs / returns / lengths, episode counters."""
    ref = O.OracleEnvs(E, N, seed=99, env_offset=1000, auto_reset=True)
    env = GpuEngine(g, E, N, auto_reset=True, seed=99, env_offset=1000, math=math)
    o_ref, o_gpu = ref.reset(), env.reset()
    for name in ("own_x", "own_y", "own_psi", "own_v", "goal_x", "goal_y", "trf_x", "trf_y", "trf_psi", "trf_v"):
        assert np.array_equal(getattr(env, name), getattr(ref, name)), name     # reset: bit-exact
    np.testing.assert_allclose(o_gpu, o_ref, rtol=0, atol=1e-9)
    rng = np.random.default_rng(1)
    dones = 0
    for _ in range(T):
        a = rng.uniform(-1, 1, E)
        o1, r1, d1, oc1, n1 = ref.step(a)
        o2, r2, d2, oc2, n2 = env.step(a)
        assert np.array_equal(d1, d2) and np.array_equal(oc1, oc2)
        np.testing.assert_allclose(o2, o1, rtol=0, atol=1e-9)
        np.testing.assert_allclose(r2, r1, rtol=0, atol=1e-9)
        assert np.array_equal(env.steps, ref.steps) and np.array_equal(env.episode, ref.episode)
        d = d1.astype(bool)
        if d.any():
            dones += int(d.sum())
            np.testing.assert_allclose(env.term_obs[d], ref.term_obs[d], rtol=0, atol=1e-9)
            np.testing.assert_allclose(env.ep_return[d], ref.ep_return[d], rtol=0, atol=1e-8)
            assert np.array_equal(env.ep_steps[d], ref.ep_steps[d])
            assert np.array_equal(env.trf_psi[d], ref.trf_psi[d]) and np.array_equal(env.own_psi[d], ref.own_psi[d])
        np.testing.assert_allclose(env.total_reward, ref.total_reward, rtol=0, atol=1e-8)
    assert dones > 0


def _oracle_config_from(O, cfg):
    """OracleConfig carrying a NON-default product configuration (same field names)."""
    return H.oracle_config(O, cfg)


_ODD_TRAFFIC = H.ODD_TRAFFIC


@pytest.mark.parametrize("N,E,T", _ODD_TRAFFIC)
def test_f64_odd_traffic_counts_and_nondefault_config_vs_oracle(g, O, N, E, T):
    """Generic work shapes (N not a power-of-two multiple of the vector width) and a configuration
    in which every tunable differs from settings.py -- different airspace, frame rate, radii,
    reward constants, an airspeed-factor RANGE (so traffic and player speeds differ and the
    kinematics.py:74 quirk matters everywhere), short episodes (timeouts occur)."""
    _odd_traffic_and_nondefault_config_vs_oracle(g, O, N, E, T, "exact")


@pytest.mark.parametrize("N,E,T", _ODD_TRAFFIC)
def test_f64_fast_odd_traffic_counts_and_nondefault_config_vs_oracle(g, O, N, E, T):
    """test_f64_odd_traffic_counts_and_nondefault_config_vs_oracle in the float64 build's FAST formulation: the same
    work shapes, configuration and criteria."""
    _odd_traffic_and_nondefault_config_vs_oracle(g, O, N, E, T, "fast")


def _odd_traffic_and_nondefault_config_vs_oracle(g, O, N, E, T, math):
    cfg = g.ACAS2DConfig(n_traffic=N, fast_math=(math == "fast"), **H.NONDEFAULT_CONFIGS["wide"])
    ref = O.OracleEnvs(E, N, seed=3, env_offset=17, auto_reset=True, config=_oracle_config_from(O, cfg))
    env = GpuEngine.__new__(GpuEngine)
    env.v = g.ACAS2DVecEnv(E, device="cuda:0", dtype=torch.float64, seed=3, env_offset=17, config=cfg)
    env.E, env.N = E, N
    o1, o2 = ref.reset(), env.reset()
    for name in ("own_psi", "trf_x", "trf_y", "trf_psi", "trf_v", "goal_x", "own_x"):
        assert np.array_equal(getattr(env, name), getattr(ref, name)), name
    assert len(np.unique(ref.trf_v)) > 10                      # speeds really vary
    np.testing.assert_allclose(o2, o1, rtol=0, atol=1e-9)
    rng = np.random.default_rng(9)
    seen = set()
    for _ in range(T):
        a = rng.uniform(-1, 1, E)
        o1, r1, d1, oc1, _ = ref.step(a)
        o2, r2, d2, oc2, _ = env.step(a)
        assert np.array_equal(d1, d2) and np.array_equal(oc1, oc2)
        np.testing.assert_allclose(o2, o1, rtol=0, atol=1e-9)
        np.testing.assert_allclose(r2, r1, rtol=0, atol=1e-9)
        seen |= set(np.unique(oc1))
    assert np.array_equal(env.steps, ref.steps) and np.array_equal(env.episode, ref.episode)
    assert {0, 2} <= seen


def test_f32_statistical_single_step_vs_f64_oracle(g, O):
    """200 000 mid-episode states (oracle rollouts with resets, N = 8), ONE float32 step each from
    the identical float32-representable state, against the float64 oracle: the distribution of the
    observation error, not just a maximum over a few fixtures."""
    E, N = 200_000, 8
    ref = O.OracleEnvs(E, N, seed=1234, auto_reset=True)
    ref.reset()
    rng = np.random.default_rng(4)
    for _ in range(int(rng.integers(20, 40))):
        ref.step(rng.uniform(-1, 1, E))
    f32 = lambda a: a.astype(np.float32).astype(np.float64)  # noqa: E731
    own = f32(np.stack([ref.own_x, ref.own_y, ref.own_psi, ref.own_v], 1))
    trf = f32(np.stack([ref.trf_x, ref.trf_y, ref.trf_psi, ref.trf_v], -1))
    steps = ref.steps.copy()
    act = f32(rng.uniform(-1, 1, E))
    chk = O.OracleEnvs(E, N)
    chk.set_state(own, trf, None, steps)
    o, r, d, oc, _ = chk.step(act)
    env = GpuEngine(g, E, N, dtype=torch.float32)
    env.set_state(own, trf, None, steps)
    obs, rew, done, outcome, _ = env.step(act)
    cfgc = O.default_config()
    ok = ~grazing(o, N, cfgc, 1e-3)
    assert ok.mean() > 0.999
    assert np.array_equal(done[ok], d[ok]) and np.array_equal(outcome[ok], oc[ok])
    rad = np.deg2rad
    v12x = (chk.own_v * np.cos(rad(chk.own_psi)))[:, None] - chk.trf_v * np.cos(rad(chk.trf_psi))
    v12y = (chk.own_v * np.sin(rad(chk.own_psi)))[:, None] - chk.trf_v * np.sin(rad(chk.trf_psi))
    well = (np.abs(v12x) > 0.02) & (np.hypot(v12x, v12y) > 2.0)
    err = np.abs(obs - o)
    err[:, [1, 4]] = np.minimum(err[:, [1, 4]], 1.0 - err[:, [1, 4]])      # headings live on a circle
    col = np.arange(o.shape[1])
    cpa = (col >= 5) & ((col - 5) % 3 == 1)
    vcl = (col >= 5) & ((col - 5) % 3 == 2)
    # closing speed = dot(dv, dp) / |dp| / dt (kinematics.py:77): for aircraft a few pixels apart
    # (random spawns on top of the player) float32 position rounding (1.2e-4 px) is a visible
    # fraction of |dp| -- ill-conditioned in the reference itself; entries with |dp| < 16 px are
    # bounded separately
    near = (o[:, 5::3] * cfgc.d_sep_max) < 16.0
    e_own, e_dist = err[:, :5], err[:, (col >= 5) & ((col - 5) % 3 == 0)]
    e_vc, e_vc_near, e_cpa = err[:, vcl][~near], err[:, vcl][near], err[:, cpa][well]
    print("f32 one-step |obs error| vs f64 oracle over %d states: player entries max %.2e; distance max %.2e; closing "
          "speed max %.2e p99.9 %.2e (|dp| >= 16 px; %d entries closer: max %.2e); d_cpa (well-conditioned, %.2f %%) "
          "max %.2e p99.9 %.2e" % (E, e_own.max(), e_dist.max(), e_vc.max(), np.quantile(e_vc, 0.999), near.sum(),
                                   e_vc_near.max() if near.any() else 0.0, 100 * well.mean(), e_cpa.max(),
                                   np.quantile(e_cpa, 0.999)))
    assert e_own.max() < 1e-5 and e_dist.max() < 1e-5 and e_vc.max() < 1e-5 and e_cpa.max() < 2e-5
    assert near.mean() < 1e-3 and (not near.any() or e_vc_near.max() < 1e-3)
    assert np.quantile(err[:, ~cpa], 0.999) < 2e-6
    # the shaped reward multiplies in (d_cpa / 192)^4 (rewards.py:12-16), i.e. it amplifies the
    # d_cpa entry's error by up to 4 * 1886 / 192 = 39x: 1e-5 holds for 99.99 % of the states,
    # the worst of 200 000 stays below 5e-5
    nt = ok & ~d.astype(bool) & well[:, 0]
    e_rew = np.abs(rew[nt] - r[nt])
    print("f32 one-step |reward error| (non-terminal): max %.2e p99.99 %.2e" % (e_rew.max(), np.quantile(e_rew, 0.9999)))
    assert np.quantile(e_rew, 0.9999) < 1e-5 and e_rew.max() < 5e-5
    assert max(np.abs(env.own_x - chk.own_x).max(), np.abs(env.trf_x - chk.trf_x).max(),
               np.abs(env.trf_y - chk.trf_y).max()) <= 1.3e-4


def test_f64_fast_statistical_single_step_vs_oracle(g, O):
    """The float64 FAST formulation beyond the fixtures: 200 000 mid-episode states (oracle rollouts with resets,
    N = 8), ONE step each from the identical state, against the oracle.  Everything within 1e-9 (the contract asks
    1e-5) except where the reference itself is ill-conditioned: d_cpa divides by |v12| and takes the sign of v12x
    (kinematics.py:40-49), so its error scales with 1 / |v12| and its sign is a coin toss at v12x = +-1e-13."""
    E, N = 200_000, 8
    ref = O.OracleEnvs(E, N, seed=4321, auto_reset=True)
    ref.reset()
    rng = np.random.default_rng(9)
    for _ in range(int(rng.integers(20, 40))):
        ref.step(rng.uniform(-1, 1, E))
    own = np.stack([ref.own_x, ref.own_y, ref.own_psi, ref.own_v], 1)
    trf = np.stack([ref.trf_x, ref.trf_y, ref.trf_psi, ref.trf_v], -1)
    steps, act = ref.steps.copy(), rng.uniform(-1, 1, E)
    chk = O.OracleEnvs(E, N)
    chk.set_state(own, trf, None, steps)
    o, r, d, oc, _ = chk.step(act)
    env = GpuEngine(g, E, N, math="fast")
    env.set_state(own, trf, None, steps)
    obs, rew, done, outcome, _ = env.step(act)
    ok = ~grazing(o, N, O.default_config(), 1e-9)
    assert ok.mean() > 0.99999
    assert np.array_equal(done[ok], d[ok]) and np.array_equal(outcome[ok], oc[ok])
    rad = np.deg2rad
    v12x = (chk.own_v * np.cos(rad(chk.own_psi)))[:, None] - chk.trf_v * np.cos(rad(chk.trf_psi))
    v12y = (chk.own_v * np.sin(rad(chk.own_psi)))[:, None] - chk.trf_v * np.sin(rad(chk.trf_psi))
    well = (np.abs(v12x) > 1e-6) & (np.hypot(v12x, v12y) > 1e-3)
    err = np.abs(obs - o)
    err[:, [1, 4]] = np.minimum(err[:, [1, 4]], 1.0 - err[:, [1, 4]])      # headings live on a circle
    col = np.arange(o.shape[1])
    cpa = (col >= 5) & ((col - 5) % 3 == 1)
    e_cpa = err[:, cpa]
    print("f64 FAST one-step |obs error| vs oracle over %d states: all but d_cpa max %.2e; d_cpa max %.2e (%.4f %% of the "
          "entries ill-conditioned and set aside); reward max %.2e; positions max %.2e"
          % (E, np.nanmax(err[:, ~cpa]), np.nanmax(e_cpa[well]), 100 * (~well).mean(),
             np.nanmax(np.abs(rew - r)[ok & well[:, 0]]), np.abs(env.trf_x - chk.trf_x).max()))
    # measured: 1.1e-15 / 8.4e-13 / 1.1e-13 (reward) / 2.3e-13 (positions)
    assert np.nanmax(err[:, ~cpa]) < 1e-12 and np.nanmax(e_cpa[well]) < 1e-10 and (~well).mean() < 1e-4
    assert np.array_equal(np.isnan(obs), np.isnan(o))
    assert np.nanmax(np.abs(rew - r)[ok & well[:, 0]]) < 1e-11
    for name in ("own_x", "own_y", "own_psi", "trf_x", "trf_y"):
        assert np.nanmax(np.abs(getattr(env, name) - getattr(chk, name))) < 1e-11, name
    assert np.array_equal(env.steps, chk.steps)


def test_f32_reset_names_the_same_episodes(g, O):
    """(seed, global env index, episode counter) names ONE episode per element type, whichever path draws
    it: reset() / reset_masked() (reset_kernel) and the auto-reset inside a step (both of its walks) call
    the same per-entity function.  The float32 build evaluates the draws in float32 (24 random bits):
    equal to the float64 oracle up to float32 rounding of the 1600-px / 360-degree ranges (positions
    2.5e-4, headings 6e-5); the float64 build is bit-equal to the oracle (test_f64_auto_reset_vs_oracle)."""
    E, N = 4096, 8
    ref = O.OracleEnvs(E, N, seed=5, auto_reset=True)

    def close_to_oracle(env, sel):
        assert np.abs(env.trf_x[sel] - ref.trf_x[sel]).max() < 2.5e-4
        assert np.abs(env.trf_y[sel] - ref.trf_y[sel]).max() < 2.5e-4
        for name in ("trf_psi", "own_psi"):
            dpsi = np.abs(getattr(env, name)[sel] - getattr(ref, name)[sel])
            assert np.minimum(dpsi, 360 - dpsi).max() < 6e-5, name
        assert np.array_equal(env.trf_v[sel], ref.trf_v[sel])

    ref.reset()
    env = GpuEngine(g, E, N, dtype=torch.float32, auto_reset=True, seed=5)
    env.reset()
    close_to_oracle(env, np.ones(E, bool))
    # step both with the same actions until plenty of envs have been reset inside the step
    rng = np.random.default_rng(3)
    checked = 0
    twin = g.ACAS2DVecEnv(E, N, device="cuda:0", dtype=torch.float32, auto_reset=True, seed=5)
    for _ in range(40):
        a = rng.uniform(-1, 1, E).astype(np.float32).astype(np.float64)
        _, _, d1, _, _ = ref.step(a)
        _, _, d2, _, _ = env.step(a)
        both = (d1 != 0) & (d2 != 0) & (env.episode == ref.episode)
        if both.any():
            checked += int(both.sum())
            close_to_oracle(env, both)
        fresh = torch.as_tensor(d2 != 0, device="cuda:0")
        if fresh.any():
            # the same episodes drawn by reset_kernel on a twin env: bit for bit what the step produced
            twin.episode.copy_(env.v.episode)
            twin._launch_reset(fresh.to(torch.uint8), do_init=1)
            for name in ("own_x", "own_y", "own_psi", "own_v", "goal_x", "goal_y", "trf_x", "trf_y", "trf_psi", "trf_v"):
                assert torch.equal(getattr(twin, name)[fresh], getattr(env.v, name)[fresh]), name
            assert bits_equal(twin.outputs["obs"][fresh], env.v.outputs["obs"][fresh])
    assert checked > 50


def _dtype_and_config(g, dtype_name, N):
    """"float64fast" = the float64 build's FAST formulation (ACAS2DConfig.fast_math)."""
    fast = dtype_name == "float64fast"
    return getattr(torch, "float64" if fast else dtype_name), g.ACAS2DConfig(n_traffic=N, fast_math=fast)


@pytest.mark.parametrize("dtype_name,N,E,T", (("float32", 8, 4096, 160), ("float64", 8, 1024, 120), ("float32", 64, 512, 40),
                                               ("float32", 3, 2048, 60), ("float32", 1, 640, 450), ("float64", 3, 333, 50),
                                               ("float64fast", 8, 1024, 120), ("float64fast", 3, 333, 50)))
def test_rollout_equals_sequential_steps(g, dtype_name, N, E, T):
    """acas2d_rollout_* (T steps fused in one launch, state in registers) == T x acas2d_step_*,
    bit for bit: observations, rewards, masks, side channels and the final state."""
    dtype, cfg = _dtype_and_config(g, dtype_name, N)
    dev = "cuda:0"
    a = g.ACAS2DVecEnv(E, N, device=dev, dtype=dtype, seed=77, env_offset=5, config=cfg)
    b = g.ACAS2DVecEnv(E, N, device=dev, dtype=dtype, seed=77, env_offset=5, config=cfg)
    a.reset()
    b.reset()
    gen = torch.Generator(device=dev).manual_seed(11)
    actions = torch.rand(T, E, generator=gen, device=dev, dtype=dtype) * 2 - 1
    out = a.rollout(actions, keep_terminal_obs=True)
    torch.cuda.synchronize()
    dones = 0
    for t in range(T):
        obs, rew, done, infos = b.step(actions[t])
        assert bits_equal(out["obs"][t], obs), t
        assert bits_equal(out["reward"][t], rew) and bits_equal(out["done"][t], done)
        assert bits_equal(out["outcome"][t], infos.outcome)
        d = done
        if bool(d.any()):
            dones += int(d.sum())
            assert bits_equal(out["episode_return"][t][d], infos.episode_return[d])
            assert bits_equal(out["episode_steps"][t][d], infos.episode_steps[d])
            assert bits_equal(out["terminal_observation"][t][d], infos.terminal_observation[d])
    assert dones > 0
    for name in ("own_x", "own_y", "own_psi", "own_v", "goal_x", "goal_y", "trf_x", "trf_y", "trf_psi", "trf_v",
                 "steps", "total_reward", "episode"):
        assert bits_equal(getattr(a, name), getattr(b, name)), name
    assert bits_equal(a.outputs["obs"], b.outputs["obs"])          # the latest observation, either way
    # and a second rollout continues from the state the first one left, reusing the buffers
    actions2 = torch.rand(T, E, generator=gen, device=dev, dtype=dtype) * 2 - 1
    out = a.rollout(actions2, out=out)
    for t in range(T):
        obs, rew, done, _ = b.step(actions2[t])
        assert bits_equal(out["obs"][t], obs) and bits_equal(out["done"][t], done)
    with pytest.raises(RuntimeError, match="packed work shape"):
        g.ACAS2DVecEnv(16, 5, device=dev, dtype=dtype).rollout(torch.zeros(2, 16, device=dev, dtype=dtype))


@pytest.mark.parametrize("dtype_name", ("float32", "float64", "float64fast"))
def test_rollout_wraps_and_stores_injected_headings_like_steps(g, dtype_name):
    """aircraft.py:22 wraps a heading (psi % 360) on every step.  Headings injected outside [0, 360)
    are wrapped by the first step and written back; the fused rollout keeps the traffic's sin / cos
    in registers across steps and must still leave the same (wrapped) state behind."""
    E, N, T = 256, 8, 7
    dtype, cfg = _dtype_and_config(g, dtype_name, N)
    own, trf, goal = H.parity_reset_states(cfg, 99, 0, E)
    own[:, 2] += 360.0                       # 357..363 -> 717..723: inside the float32 window (-360, 720)
    own[:, 2] = np.minimum(own[:, 2], 719.0)
    trf[:, :, 2] += 360.0 * (np.arange(N)[None, :] % 2)
    a = g.ACAS2DVecEnv(E, N, device="cuda:0", dtype=dtype, seed=3, config=cfg)
    b = g.ACAS2DVecEnv(E, N, device="cuda:0", dtype=dtype, seed=3, config=cfg)
    for v in (a, b):
        v.set_state(own, trf, goal, np.zeros(E, np.int32), observe=False)
    gen = torch.Generator(device="cuda:0").manual_seed(2)
    actions = torch.rand(T, E, generator=gen, device="cuda:0", dtype=dtype) * 2 - 1
    out = a.rollout(actions)
    for t in range(T):
        obs, rew, done, _ = b.step(actions[t])
        assert bits_equal(out["obs"][t], obs) and bits_equal(out["reward"][t], rew), t
    for name in ("own_psi", "trf_psi", "trf_x", "trf_y", "own_x", "own_y", "steps", "episode"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert float(a.trf_psi.max()) < 360.0 and float(a.own_psi.max()) < 360.0


@pytest.mark.parametrize("dtype_name,N,shapes", (
    ("float32", 8, ("4,2", "8,1", "2,4", "generic,4", "generic,1")),
    ("float32", 64, ("4,16", "8,8", "2,32", "generic,16", "generic,64")),
    ("float64", 8, ("2,4", "4,2", "generic,4")),
    ("float64fast", 8, ("2,4", "4,2", "generic,4"))))
def test_results_do_not_depend_on_the_work_shape(g, dtype_name, N, shapes):
    """How the traffic of an env is spread over lanes (ACAS2D_SHAPE, a tuning knob) must not change a
    single bit: both builds compile with -ffp-contract=off, every variant runs the same IEEE
    operations per aircraft (packed float2 math included), and the reset RNG is keyed per entity."""
    dtype, cfg = _dtype_and_config(g, dtype_name, N)
    E, T = 1536, 120
    gen = torch.Generator(device="cuda:0").manual_seed(4)
    actions = torch.rand(T, E, generator=gen, device="cuda:0", dtype=dtype) * 2 - 1
    ref = None
    try:
        for sh in shapes:
            os.environ["ACAS2D_SHAPE"] = sh
            v = g.ACAS2DVecEnv(E, N, device="cuda:0", dtype=dtype, seed=8, config=cfg)
            assert g.native.launch_geometry(E, N, 4 if dtype == torch.float32 else 8)["lanes_per_env"] == int(sh.split(",")[1])
            got = [v.reset().clone()]
            dones = 0
            for t in range(T):
                obs, rew, done, infos = v.step(actions[t])
                got += [obs.clone(), rew.clone(), done.clone(), infos.outcome.clone()]
                dones += int(done.sum())
            got += [v.trf_x.clone(), v.trf_psi.clone(), v.own_psi.clone(), v.total_reward.clone(), v.episode.clone()]
            assert dones > 0
            if ref is None:
                ref = got
            else:
                for k, (a, b) in enumerate(zip(ref, got)):
                    assert bits_equal(a, b), (sh, k)
    finally:
        os.environ.pop("ACAS2D_SHAPE", None)


@pytest.mark.parametrize("dtype_name,N,E,T", (("float32", 8, 4096 + 17, 200), ("float32", 64, 640, 40), ("float32", 3, 2048, 80),
                                               ("float32", 5, 1000, 80), ("float64", 8, 1024, 120), ("float64fast", 8, 1024, 120),
                                               ("float64", 7, 500, 60)))
def test_double_buffered_step_equals_in_place(g, dtype_name, N, E, T):
    """acas2d_step_* with a state_out (read generation g, write generation 1 - g; the VecEnv default) against the
    same steps in place: every observation, reward, mask, side channel and the final state bit for bit -- packed
    and generic work shapes (N = 5, 7), a last wave with padding lanes, resets in both."""
    dtype, cfg = _dtype_and_config(g, dtype_name, N)
    bits = torch.int32 if dtype == torch.float32 else torch.int64

    def same(x, y):                          # bit for bit: a NaN d_cpa (exact parallel flight) equals itself
        return torch.equal(x.view(bits), y.view(bits)) if x.is_floating_point() else torch.equal(x, y)

    gen = torch.Generator(device="cuda:0").manual_seed(11)
    actions = torch.rand(T, E, generator=gen, device="cuda:0", dtype=dtype) * 2 - 1
    a = g.ACAS2DVecEnv(E, N, device="cuda:0", dtype=dtype, seed=21, env_offset=3, config=cfg, double_buffer=True)
    b = g.ACAS2DVecEnv(E, N, device="cuda:0", dtype=dtype, seed=21, env_offset=3, config=cfg, double_buffer=False)
    assert a.double_buffer and not b.double_buffer and a._gen["own_x"].shape[0] == 2 and b._gen["own_x"].shape[0] == 1
    assert same(a.reset(), b.reset())
    dones = 0
    for t in range(T):
        oa, ra, da, ia = a.step(actions[t])
        ob, rb, db, ib = b.step(actions[t])
        assert a.generation == (t + 1) % 2 and b.generation == 0
        assert same(oa, ob) and same(ra, rb) and torch.equal(da, db), t
        for k in ("outcome", "terminal_observation", "episode_return", "episode_steps"):
            assert same(a.outputs[k], b.outputs[k]), (t, k)
        dones += int(da.sum())
        if t in (0, 1, T // 2, T - 1):
            for name in ("own_x", "own_y", "own_psi", "own_v", "goal_x", "goal_y", "trf_x", "trf_y", "trf_psi", "trf_v", "steps",
                         "total_reward", "episode"):
                assert same(getattr(a, name), getattr(b, name)), (t, name)
    assert dones > 20
    # a fused rollout and a masked reset act on the LIVE generation, whichever it is
    a.step(actions[0]); b.step(actions[0])
    assert a.generation == (T + 1) % 2
    if N not in (5, 7):                      # (the fused rollout needs a packed work shape)
        ra, rb = a.rollout(actions[:8]), b.rollout(actions[:8])
        assert same(ra["obs"], rb["obs"]) and same(ra["reward"], rb["reward"]) and same(a.trf_x, b.trf_x)
    mask = (torch.arange(E, device="cuda:0") % 3 == 0)
    assert same(a.reset_masked(mask), b.reset_masked(mask)) and same(a.own_psi, b.own_psi)
    oa, _, _, _ = a.step(actions[1]); ob, _, _, _ = b.step(actions[1])
    assert same(oa, ob) and torch.equal(a.steps, b.steps)


@pytest.mark.parametrize("N,E,T,db", ((8, 4096, 150, True), (8, 5120, 150, False), (64, 640, 40, False),
                                      (3, 4096, 80, True), (1, 2048, 560, True)))
def test_consecutive_layout_kernel_equals_the_general_kernel(g, monkeypatch, N, E, T, db):
    """float32 state as ACAS2DVecEnv allocates it (consecutive rows: include/acas2d.h) takes the step kernel whose
    loads all go through preloaded base pointers; ACAS2D_NO_ARENA (read per launch) sends the same state through the
    general kernel.  Every observation, reward, mask, side channel and the final state bit for bit, resets, both
    store policies.  (The kernel assumes whole multiples of eight workgroups; other sizes take the general kernel.)"""
    dtype, cfg = _dtype_and_config(g, "float32", N)
    same = lambda x, y: torch.equal(x.view(torch.int32), y.view(torch.int32)) if x.is_floating_point() else torch.equal(x, y)  # noqa: E731
    gen = torch.Generator(device="cuda:0").manual_seed(12)
    actions = torch.rand(T, E, generator=gen, device="cuda:0") * 2 - 1
    a = g.ACAS2DVecEnv(E, N, device="cuda:0", seed=5, env_offset=9, config=cfg, double_buffer=db)
    b = g.ACAS2DVecEnv(E, N, device="cuda:0", seed=5, env_offset=9, config=cfg, double_buffer=db)
    assert a.consecutive_layout and a.own_y.data_ptr() == a.own_x.data_ptr() + 4 * E
    assert not g.ACAS2DVecEnv(E + 17, N, device="cuda:0").consecutive_layout          # not whole workgroups
    assert not g.ACAS2DVecEnv(64, N, device="cuda:0", dtype=torch.float64).consecutive_layout
    assert not g.ACAS2DVecEnv(64, N, device="cuda:0", auto_reset=False).consecutive_layout
    assert same(a.reset(), b.reset())
    dones = 0
    for t in range(T):
        oa, ra, da, _ = a.step(actions[t])
        monkeypatch.setenv("ACAS2D_NO_ARENA", "1")
        assert not b.consecutive_layout
        ob, rb, db_, _ = b.step(actions[t])
        monkeypatch.delenv("ACAS2D_NO_ARENA")
        assert same(oa, ob) and same(ra, rb) and torch.equal(da, db_), t
        for k in ("outcome", "terminal_observation", "episode_return", "episode_steps"):
            assert same(a.outputs[k], b.outputs[k]), (t, k)
        dones += int(da.sum())
    for name in ("own_x", "own_y", "own_psi", "own_v", "goal_x", "goal_y", "trf_x", "trf_y", "trf_psi", "trf_v", "steps",
                 "total_reward", "episode"):
        assert same(getattr(a, name), getattr(b, name)), name
    assert dones > (20 if N > 1 else 0)          # (one traffic aircraft: head-on, the first collisions near step 500)


def test_double_buffered_steps_in_a_replayed_graph(g):
    """A hipGraph holds the state generation it was captured at: an EVEN number of captured steps leaves the live
    generation where the capture found it, and align_generation() puts it back there after an odd number of
    other steps -- the replayed run equals the same steps launched one by one."""
    E, N, CH = 2048, 8, 6
    gen = torch.Generator(device="cuda:0").manual_seed(2)
    actions = torch.rand(CH, E, generator=gen, device="cuda:0") * 2 - 1
    a = g.ACAS2DVecEnv(E, N, device="cuda:0", seed=4, double_buffer=True)
    b = g.ACAS2DVecEnv(E, N, device="cuda:0", seed=4, double_buffer=True)
    a.reset(); b.reset()
    for t in range(3):                      # warm-up before the capture (an odd number: generation 1 is live)
        a.step_from(actions[t]); b.step_from(actions[t])
    torch.cuda.synchronize()
    g0 = a.generation
    assert g0 == 1
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for t in range(CH):
            a.step_from(actions[t])
    assert a.generation == g0               # an even number of steps was captured; nothing ran
    for rep in range(5):
        if rep == 2:                        # an odd number of plain steps in between: the live generation moves on
            a.step_from(actions[0]); b.step_from(actions[0])
            assert a.generation != g0
        a.align_generation(g0)
        assert a.generation == g0
        graph.replay()
        for t in range(CH):
            b.step_from(actions[t])
        torch.cuda.synchronize()
        assert bits_equal(a.outputs["obs"], b.outputs["obs"]) and bits_equal(a.outputs["reward"], b.outputs["reward"])
        for name in ("own_x", "own_psi", "trf_y", "steps", "total_reward", "episode"):
            assert torch.equal(getattr(a, name), getattr(b, name)), (rep, name)
    with pytest.raises(RuntimeError):
        g.ACAS2DVecEnv(64, 1, device="cuda:0", double_buffer=False).align_generation(1)
    # the default is the measured policy: on for launches of one generation of wavefronts (the headline size), off beyond
    assert g.ACAS2DVecEnv(65536, 8, device="cuda:0").double_buffer and g.ACAS2DVecEnv(65536, 8, device="cuda:0", dtype=torch.float64).double_buffer
    assert not g.ACAS2DVecEnv(131072, 8, device="cuda:0").double_buffer and not g.ACAS2DVecEnv(16384, 64, device="cuda:0").double_buffer
    assert not g.ACAS2DVecEnv(64, 1, device="cuda:0", auto_reset=False).double_buffer
    with pytest.raises(ValueError):
        g.ACAS2DVecEnv(64, 1, device="cuda:0", auto_reset=False, double_buffer=True)


def _first_episode(out, E):
    """outcome / game.steps / return of each env's FIRST finished episode in a rollout dict."""
    done = out["done"].cpu().numpy()
    assert done.any(0).all(), "every env must finish at least once"
    t0 = done.argmax(0)
    e = np.arange(E)
    return (out["outcome"].cpu().numpy()[t0, e], out["episode_steps"].cpu().numpy()[t0, e],
            out["episode_return"].cpu().numpy()[t0, e].astype(np.float64))


def test_fused_policy_rollout_reproduces_the_reference_policy_evaluation(g):
    """acas2d_rollout_policy_f64: testing_main.py's whole loop (policy.predict + env.step, 1001 steps,
    100 episodes) in ONE launch with the reference's trained SB3 actor evaluated inside the kernel.
    It must score what the reference recorded for that policy (mean return 1210.069219, mean length
    704.35, 100/100 goals) -- the in-kernel float32 MLP differs from torch's by summation order
    only (~1e-7 per action), so the table is held to 1e-4 relative instead of every digit."""
    pol = g.load_sb3_policy(os.path.join(H.GOLDEN, "ref_policy_best_model.npz"), device="cuda:0")
    own, trf, goal = H.parity_reset_states(g.ACAS2DConfig(), 13, 0, 100)
    v = g.ACAS2DVecEnv(100, 1, device="cuda:0", dtype=torch.float64, auto_reset=True)
    obs0 = v.set_state(own, trf, goal, np.zeros(100, np.int32), observe=True).clone()
    out = v.rollout_policy(pol, 1001)
    a0 = pol.predict(obs0).reshape(-1).to(torch.float64)
    assert float((out["actions"][0] - a0).abs().max()) < 2e-6
    oc, steps, ret = _first_episode(out, 100)
    assert (oc == 1).all()
    H.assert_matches_reference_policy_eval(ret, steps, 2.0 * (steps - 1), tol=1e-4)
    # a loose speed floor: the in-kernel MLP once regressed 7x (its weight loads were hoisted out of the
    # step loop and spilled) without a single wrong bit; 65 536 envs x 100 steps take ~1.5 ms
    big = g.ACAS2DVecEnv(65536, 1, device="cuda:0", dtype=torch.float32, seed=1)
    big.reset()
    o = big.rollout_policy(pol, 100)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    big.rollout_policy(pol, 100, out=o)
    t1.record()
    torch.cuda.synchronize()
    assert t0.elapsed_time(t1) < 6.0, t0.elapsed_time(t1)
    # the convenience wrapper, and the step-by-step evaluation it replaces
    fused = g.evaluate_policy_fused(pol, own, trf, goal)
    assert fused["unfinished"] == 0 and np.array_equal(fused["outcome"], oc) and np.array_equal(fused["steps"], steps)
    ev = g.ACAS2DVecEnv(100, 1, device="cuda:0", dtype=torch.float64, auto_reset=False)
    ev.set_state(own, trf, goal, np.zeros(100, np.int32))
    slow = g.evaluate_policy(ev, pol)
    assert np.array_equal(slow["outcome"], fused["outcome"]) and np.array_equal(slow["steps"], fused["steps"])
    assert np.abs(slow["total_reward"] - fused["total_reward"]).max() < 1e-3
    np.testing.assert_allclose(slow["path_length"], fused["path_length"])


_POLICY_CASES = (("float32", 1, 4096, 800), ("float32", 2, 2048, 120), ("float32", 3, 2048, 120), ("float32", 4, 2048, 100),
                 ("float32", 8, 2048, 60), ("float64", 1, 1024, 800), ("float64", 2, 2048, 120), ("float64", 3, 2048, 120),
                 ("float64", 4, 2048, 100))


@pytest.mark.parametrize("dtype_name,N,E,T", _POLICY_CASES,
                         ids=["%s%d-%d-%d" % ("" if d == "float32" else "f64-", n, e, t) for d, n, e, t in _POLICY_CASES])
def test_fused_policy_rollout_equals_policy_then_step(g, dtype_name, N, E, T):
    """The fused launch against torch's policy.predict() + step() per step on a twin env, for every thread-per-env
    instantiation of the policy kernel (C = N, G = 1: N in {1, 2, 3, 4, 8} for float32, {1, 2, 3, 4} for float64).
    Same env arithmetic (bit-identical given the same actions); the two MLP evaluations (float32 in both builds)
    differ by rounding, so actions are compared to 1e-5 (NaN actions at the same places) -- and the env outputs and
    state bit for bit, the twin being fed the fused run's own actions."""
    dev = "cuda:0"
    dtype = getattr(torch, dtype_name)
    torch.manual_seed(5)
    if N == 1:                                          # the reference's trained policy: reaches the goal
        pol = g.load_sb3_policy(os.path.join(H.GOLDEN, "ref_policy_best_model.npz"), device=dev)
    else:
        pol = g.ActorCritic(5 + 3 * N).to(dev)
        with torch.no_grad():                           # a policy that actually steers (the SB3 init is ~0)
            pol.action_net.weight.mul_(60.0)
    a = g.ACAS2DVecEnv(E, N, device=dev, dtype=dtype, seed=21)
    b = g.ACAS2DVecEnv(E, N, device=dev, dtype=dtype, seed=21)
    a.reset()
    obs = b.reset().clone()
    out = a.rollout_policy(pol, T)
    same = torch.ones(E, dtype=torch.bool, device=dev)
    worst_a = 0.0
    for t in range(T):
        act = pol.predict(obs.float()).reshape(-1).to(dtype)
        # a NaN observation (exact parallel flight) gives a NaN action in both; Python's max() would drop a NaN difference
        nan = torch.isnan(act)
        assert torch.equal(torch.isnan(out["actions"][t]), nan), t
        if not bool(nan.all()):
            worst_a = max(worst_a, float((out["actions"][t] - act)[~nan].abs().max()))
        same &= out["actions"][t] == act
        obs, rew, done, infos = b.step(out["actions"][t])          # feed the fused run's own actions
        assert bits_equal(out["obs"][t], obs) and bits_equal(out["reward"][t], rew), t
        assert torch.equal(out["done"][t], done) and torch.equal(out["outcome"][t], infos.outcome), t
        obs = obs.clone()
    assert worst_a < 1e-5, worst_a
    assert float(out["actions"].abs().max()) > 0.2 and int(out["done"].sum()) > 0
    for name in ("own_x", "own_y", "own_psi", "trf_x", "trf_y", "steps", "total_reward", "episode"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert bits_equal(a.outputs["obs"], b.outputs["obs"])
    with pytest.raises(RuntimeError, match="thread-per-env"):
        g.ACAS2DVecEnv(64, 16, device=dev, dtype=dtype).rollout_policy(g.ActorCritic(53).to(dev), 2)


def test_lazy_infos_and_vecenv_surface(g):
    E, N = 256, 64                          # N = 64: episodes last ~8 steps -> many dones
    env = g.ACAS2DVecEnv(E, N, device="cuda:0", dtype=torch.float32, seed=3)
    obs = env.reset()
    assert obs.shape == (E, 5 + 3 * N) and env.observation_space.shape == (5 + 3 * N,)
    assert env.num_envs == E and env.env_is_wrapped(None) == [False] * E
    seen = 0
    for _ in range(10):
        obs, rew, done, infos = env.step(torch.zeros(E, 1, device="cuda:0"))
        assert obs.shape == (E, 5 + 3 * N) and rew.shape == (E,) and done.dtype == torch.bool
        assert len(infos) == E
        dn = done.cpu().numpy()
        for i in np.nonzero(dn)[0][:5]:
            info = infos[int(i)]
            assert set(info) == {"outcome", "episode", "terminal_observation"}
            assert info["episode"]["l"] == info["episode"]["steps"] - 1 >= 1
            assert info["terminal_observation"].shape == (5 + 3 * N,)
            assert info["outcome"] in (1, 2, 3)
            seen += 1
        for i in np.nonzero(~dn)[0][:3]:
            assert infos[int(i)] == {}
    assert seen > 0
    sd = env.state_dict()
    env.step(torch.zeros(E, device="cuda:0"))
    env.load_state_dict(sd)
    assert torch.equal(env.own_x, sd["own_x"])
    with pytest.raises(ValueError):
        env.step(torch.zeros(E + 1, device="cuda:0"))


# ---- BASELINE.json full sizes: oracle spot check + size-independent properties -------------------
@pytest.mark.parametrize("E,N,T", ((65536, 8, 12), (131072, 8, 6), (65536, 64, 6), (4096, 3, 40)))
def test_full_size_f64_vs_oracle(g, O, E, N, T):
    ref = O.OracleEnvs(E, N, seed=13, auto_reset=True)
    env = GpuEngine(g, E, N, auto_reset=True, seed=13)
    ref.reset()
    env.reset()
    rng = np.random.default_rng(2)
    for _ in range(T):
        a = rng.uniform(-1, 1, E)
        o1, r1, d1, oc1, _ = ref.step(a)
        o2, r2, d2, oc2, _ = env.step(a)
        assert np.array_equal(d1, d2) and np.array_equal(oc1, oc2)
        assert np.abs(o2 - o1).max() < 1e-9 and np.abs(r2 - r1).max() < 1e-9
    assert np.array_equal(env.steps, ref.steps) and np.array_equal(env.episode, ref.episode)


def _default_oracle_config():
    from oracle import oracle
    return oracle.default_config()


def _new_f32_totals():
    return dict(steps=0, mask_mismatch=0, in_band=0, finished=0, e_obs=0.0, e_cpa=0.0, e_rew=0.0, e_term=0.0, e_fresh_obs=0.0,
                outcomes=set(), cpa_ratio=0.0, e_pos=0.0, pos_bound=0.0, e_ret=0.0, e_reset_pos=0.0, e_reset_psi=0.0, e_speed=0.0,
                bounds=None)


def _check_f32_step_vs_oracle(env, chk, stepped, got, N, tot, t=0, in_band=None):
    """One float32 step against the float64 oracle `chk` stepped from the identical (float32-representable) state:
    stepped = chk.step()'s (o, r, d, oc), got = the engine's (obs, rew, done, outcome).  done / outcome masks equal
    outside a 1e-3 px band around the thresholds; observations, rewards and positions of the envs that go on within the
    tolerances of test_f32_statistical_single_step_vs_f64_oracle; for the envs that finish: the terminal observation,
    the episode return and length, and the freshly drawn episode with its first observation.  Accumulates the counts,
    the worst errors and the outcomes compared in `tot`; returns the envs that went on and those that finished, both
    outside the band.

    The bounds that depend on the configuration are derived from chk.cfg (the oracle's copy of it) by helpers.f32_bounds
    and f32_pos_bound; for the default configuration they are the fixed numbers below in brackets.  Positions: 1 float32
    ulp of the largest |coordinate| M of the compared envs, at least 1.3e-4 (M < 2048 px; [1.3e-4]).  Episode return:
    1 ulp of the larger terminal bonus, at least 1.3e-4, + 1e-5 [1.4e-4].  Non-terminal reward: 5e-5 times the d_cpa
    amplification 4 d_cpa_max / safe_distance over the default's, at least 1 [5e-5].  The fresh episode (the float32
    build draws in float32 from 24 random bits): positions 2 ulp of the largest drawn coordinate, at least 2.5e-4
    [2.5e-4], headings 6e-5 (2 ulp of 360); speeds bit-equal when the speed factor is a single value [always], else
    within (max - min) airspeed 2^-24 + 2 ulp of max airspeed.  The d_cpa entry: 2e-5 [2e-5], plus under a speed range
    d (max airspeed 2^-20) / (|v12| d_cpa_max) per entry (see below).  At most a fraction 1e-3 [1e-3] of the envs in the
    band, times the collision distance over the traffic's draw area relative to the default's -- or, with `in_band` (bool [E]),
    exactly the envs it names (hand-placed states, tests/edge_states.py).  With a latching `chk` (auto_reset off) the
    finished envs are checked like the others: their state latches, nothing is reset; the terminal reward to the return's
    bound."""
    o, r, d, oc = stepped
    obs, rew, done, outcome = got
    E = len(d)
    cfgc = chk.cfg
    bnd = H.f32_bounds(cfgc, _default_oracle_config())
    tot["bounds"] = bnd
    col = np.arange(5 + 3 * N)
    cpa, vcl = (col >= 5) & ((col - 5) % 3 == 1), (col >= 5) & ((col - 5) % 3 == 2)
    d = d.astype(bool)
    # ---- masks: bit-exact outside the band
    ok = ~grazing(np.where(d[:, None] & chk.auto_reset, chk.term_obs, o), N, cfgc, 1e-3)
    mism = (done.astype(bool) != d) | (outcome != oc)
    tot["mask_mismatch"] += int((mism & ok).sum()); tot["in_band"] += int((~ok).sum()); tot["steps"] += E
    assert not (mism & ok).any(), (t, int((mism & ok).sum()))
    if in_band is None:
        assert ok.mean() > 1 - bnd["band"], (t, ok.mean(), bnd["band"])
    else:
        assert np.array_equal(~ok, in_band), (t, int((~ok).sum()), int(in_band.sum()))
    same = ok & ~mism
    go, fin = same & ~d, same & d
    latch = same & d if not chk.auto_reset else np.zeros_like(d)
    if latch.any():
        assert np.array_equal(env.status[same], chk.status[same])
        go, fin = same, np.zeros_like(d)
    tot["finished"] += int(fin.sum())
    tot["outcomes"] |= set(int(k) for k in np.unique(oc[fin]))
    # ---- envs that go on: the step itself
    v12x = (chk.own_v * np.cos(np.deg2rad(chk.own_psi)))[:, None] - chk.trf_v * np.cos(np.deg2rad(chk.trf_psi))
    v12y = (chk.own_v * np.sin(np.deg2rad(chk.own_psi)))[:, None] - chk.trf_v * np.sin(np.deg2rad(chk.trf_psi))
    well = (np.abs(v12x) > 0.02) & (np.hypot(v12x, v12y) > 2.0)
    near = (o[:, 5::3] * cfgc.d_sep_max) < 16.0
    err = np.abs(obs - o)
    err[:, [1, 4]] = np.minimum(err[:, [1, 4]], 1.0 - err[:, [1, 4]])
    # d_cpa: 2e-5, plus -- when speeds differ -- the reference's own conditioning d |dv12| / |v12| (kinematics.py:40-49):
    # the float32 velocity components carry a relative error of order 2^-21 (a heading rounded to float32 near 360
    # degrees, the hardware sin / cos) that equal speeds cancel in v12 and unequal ones do not (measured: 5.5e-7 v)
    cpa_tol = 2e-5
    if bnd["speed"] is not None:
        dv12 = cfgc.speed_factor_max * cfgc.airspeed * 2.0 ** -20
        cpa_tol = 2e-5 + (o[:, 5::3] * cfgc.d_sep_max) * dv12 / (np.hypot(v12x, v12y) * cfgc.d_cpa_max)
    if go.any():
        e_plain = err[:, ~(cpa | vcl)][go]
        e_vc, e_cpa = err[:, vcl][go][~near[go]], err[:, cpa][go][well[go]]
        cpa_excess = (err[:, cpa] - cpa_tol)[go][well[go]]
        tot["e_obs"] = max(tot["e_obs"], float(e_plain.max()), float(e_vc.max(initial=0.0)))
        tot["e_cpa"] = max(tot["e_cpa"], float(e_cpa.max(initial=0.0)))
        tot["cpa_ratio"] = max(tot["cpa_ratio"], float((err[:, cpa] / cpa_tol)[go][well[go]].max(initial=0.0)))
        assert e_plain.max() < 1e-5 and e_vc.max(initial=0.0) < 1e-5 and cpa_excess.max(initial=-1.0) < 0, \
            (t, e_plain.max(), e_vc.max(initial=0.0), e_cpa.max(initial=0.0))
        nt = go & ~latch & well[:, 0] & ~near[:, 0]
        e_rew = np.abs(rew[nt] - r[nt])
        lt = latch & well[:, 0] & ~near[:, 0]
        e_lret = np.abs(rew[lt] - r[lt])
        tot["e_ret"] = max(tot["e_ret"], float(e_lret.max(initial=0.0)))
        assert e_lret.max(initial=0.0) <= bnd["ret"], (t, e_lret.max(), bnd["ret"])
        tot["e_rew"] = max(tot["e_rew"], float(e_rew.max(initial=0.0)))
        # (1e-5 for 99.99 % of the env-steps, the worst below 5e-5: the reward amplifies the d_cpa error up to 39 x --
        #  see test_f32_statistical_single_step_vs_f64_oracle; a percentile needs the samples to carry it)
        assert e_rew.max(initial=0.0) < bnd["rew"] and (e_rew.size < 50000 or np.quantile(e_rew, 0.9999) < 1e-5), \
            (t, e_rew.max(), bnd["rew"])
        m = max(np.abs(chk.own_x)[go].max(), np.abs(chk.own_y)[go].max(), np.abs(chk.trf_x)[go].max(),
                np.abs(chk.trf_y)[go].max())
        pos_bound = H.f32_pos_bound(m)
        e_pos = max(np.abs(env.own_x - chk.own_x)[go].max(), np.abs(env.trf_x - chk.trf_x)[go].max(),
                    np.abs(env.trf_y - chk.trf_y)[go].max())
        tot["e_pos"], tot["pos_bound"] = max(tot["e_pos"], float(e_pos)), max(tot["pos_bound"], pos_bound)
        assert e_pos <= pos_bound, (t, e_pos, pos_bound)
        assert np.array_equal(env.steps[go], chk.steps[go])
    # ---- envs that finish: side channels of the finished episode, then the fresh one
    if fin.any():
        te = np.abs(env.term_obs - chk.term_obs)
        te[:, [1, 4]] = np.minimum(te[:, [1, 4]], 1.0 - te[:, [1, 4]])
        tw = te[:, ~(cpa | vcl)][fin]
        tot["e_term"] = max(tot["e_term"], float(tw.max()))
        assert tw.max() < 1e-5
        assert np.array_equal(env.ep_steps[fin], chk.ep_steps[fin]) and np.array_equal(env.episode[fin], chk.episode[fin])
        e_ret = np.abs(env.ep_return - chk.ep_return)[fin].max()
        tot["e_ret"] = max(tot["e_ret"], float(e_ret))
        assert e_ret <= bnd["ret"], (t, e_ret, bnd["ret"])             # one float32 ulp of the terminal bonus
        e_rp = max(np.abs(env.trf_x - chk.trf_x)[fin].max(), np.abs(env.trf_y - chk.trf_y)[fin].max())
        tot["e_reset_pos"] = max(tot["e_reset_pos"], float(e_rp))
        assert e_rp < bnd["reset_pos"], (t, e_rp, bnd["reset_pos"])
        for name in ("trf_psi", "own_psi"):
            dpsi = np.abs(getattr(env, name) - getattr(chk, name))[fin]
            tot["e_reset_psi"] = max(tot["e_reset_psi"], float(np.minimum(dpsi, 360 - dpsi).max()))
            assert np.minimum(dpsi, 360 - dpsi).max() < bnd["reset_psi"], name
        if bnd["speed"] is None:
            assert np.array_equal(env.trf_v[fin], chk.trf_v[fin])
        else:
            e_v = np.abs(env.trf_v - chk.trf_v)[fin].max()
            tot["e_speed"] = max(tot["e_speed"], float(e_v))
            assert e_v <= bnd["speed"], (t, e_v, bnd["speed"])
        assert np.array_equal(env.steps[fin], chk.steps[fin]) and (env.steps[fin] == 1).all()
        fe = np.abs(obs - o)
        fe[:, [1, 4]] = np.minimum(fe[:, [1, 4]], 1.0 - fe[:, [1, 4]])
        ff = fe[:, ~(cpa | vcl)][fin]                        # (a fresh episode's d_cpa / closing speed: from states 2.5e-4 px apart)
        tot["e_fresh_obs"] = max(tot["e_fresh_obs"], float(ff.max()))
        assert ff.max() < 1e-5
    return go, fin


def _print_f32_totals(what, tot):
    b = tot["bounds"]
    print("f32 vs f64 oracle %s: %d env-steps, %d finished (outcomes compared %s); mask mismatches outside the 1e-3 band %d "
          "(%d env-steps inside it); max |obs| %.2e, d_cpa %.2e (%.2f of its bound), reward %.2e (bound %.2e), terminal obs %.2e, first obs of "
          "a fresh episode %.2e; positions %.2e (bound %.2e), return %.2e (bound %.2e), fresh positions %.2e (bound %.2e), "
          "fresh headings %.2e (bound %.0e), fresh speeds %s"
          % (what, tot["steps"], tot["finished"], sorted(tot["outcomes"]), tot["mask_mismatch"], tot["in_band"], tot["e_obs"],
             tot["e_cpa"], tot["cpa_ratio"], tot["e_rew"], b["rew"], tot["e_term"], tot["e_fresh_obs"], tot["e_pos"], tot["pos_bound"],
             tot["e_ret"], b["ret"], tot["e_reset_pos"], b["reset_pos"], tot["e_reset_psi"], b["reset_psi"],
             "bit-equal" if b["speed"] is None else "%.2e (bound %.2e)" % (tot["e_speed"], b["speed"])))


def _f32_steps_vs_oracle(g, O, E, N, T, seed=13, env_offset=0, config=None, warmup=None, episode0=None):
    """T float32 steps WITH auto-reset, each from the oracle trajectory's state rounded to float32 (so that both sides
    start every step from the identical state and the comparison is the step's, not the accumulated drift's), checked
    by _check_f32_step_vs_oracle.  config: ACAS2DConfig keywords other than n_traffic (None: the default configuration);
    warmup: oracle steps before the first checked one (helpers.f32_oracle_steps); episode0: the episode counters after
    reset() (None: 0).  Returns the totals; "wrapped" counts the envs whose reset in a checked step wrapped the counter
    to 0."""
    cfg = g.ACAS2DConfig(n_traffic=N, **(config or {}))
    ocfg = None if config is None else _oracle_config_from(O, cfg)
    env = _engine(g.ACAS2DVecEnv(E, device="cuda:0", dtype=torch.float32, auto_reset=True, seed=seed,
                                 env_offset=env_offset, config=cfg))
    tot = _new_f32_totals()
    tot["wrapped"] = 0
    for t, own, trf, steps, episode, act, chk, stepped in H.f32_oracle_steps(O, E, N, T, seed, env_offset, warmup, ocfg,
                                                                             episode0):
        env.set_state(own, trf, None, steps)
        env.v.episode.copy_(torch.as_tensor(episode.view(np.int32), device="cuda:0"))
        obs, rew, done, outcome, _ = env.step(act)
        _check_f32_step_vs_oracle(env, chk, stepped, (obs, rew, done, outcome), N, tot, t)
        tot["wrapped"] += int(((done != 0) & (env.episode == 0)).sum())
    tot["speeds"] = len(np.unique(env.trf_v))
    if config is None:       # the default configuration's windows stay below 2048 px: the fixed 1.3e-4
        assert tot["pos_bound"] == 1.3e-4, tot["pos_bound"]
    return tot


@pytest.mark.parametrize("E,N,T", ((4096, 3, 24), (65536, 8, 5), (65536, 64, 3), (131072, 8, 4)))
def test_full_size_f32_vs_f64_oracle(g, O, E, N, T):
    """The headline dtype at the single-GPU BASELINE sizes and the per-rank shard of the 8-GPU one against the float64
    oracle: _f32_steps_vs_oracle.  Mismatches are counted and printed."""
    tot = _f32_steps_vs_oracle(g, O, E, N, T)
    _print_f32_totals("at %d x %d over %d steps" % (E, N, T), tot)
    assert tot["finished"] > (40 if N == 3 else 300)


@pytest.mark.parametrize("dtype_name", ("float32", "float64"))
def test_full_size_properties(g, dtype_name):
    """65 536 envs x 8 traffic (headline config): invariants every step, bitwise determinism,
    and invariance to sharding (2 shards with env_offset == 1 shard)."""
    dtype = getattr(torch, dtype_name)
    E, N, T = 65536, 8, 40
    dev = "cuda:0"
    full = g.ACAS2DVecEnv(E, N, device=dev, dtype=dtype, seed=13)
    again = g.ACAS2DVecEnv(E, N, device=dev, dtype=dtype, seed=13)
    a_sh = g.ACAS2DVecEnv(40000, N, device=dev, dtype=dtype, seed=13, env_offset=0)
    b_sh = g.ACAS2DVecEnv(E - 40000, N, device=dev, dtype=dtype, seed=13, env_offset=40000)
    for e in (full, again, a_sh, b_sh):
        e.reset()
    gen = torch.Generator(device=dev).manual_seed(0)
    prev_steps = full.steps.clone()
    total_done = 0
    for _ in range(T):
        a = torch.rand(E, generator=gen, device=dev, dtype=dtype) * 2 - 1
        obs, rew, done, infos = full.step(a)
        o2, r2, d2, _ = again.step(a)
        oa, ra, da, _ = a_sh.step(a[:40000].contiguous())
        ob, rb, db, _ = b_sh.step(a[40000:].contiguous())
        assert bits_equal(obs, o2) and bits_equal(rew, r2) and torch.equal(done, d2)
        assert bits_equal(obs, torch.cat([oa, ob])) and bits_equal(rew, torch.cat([ra, rb]))
        assert torch.equal(done, torch.cat([da, db]))
        steps = full.steps
        # steps advance by one, or restart at 1 exactly where done
        assert torch.equal(torch.where(done, torch.ones_like(steps), prev_steps + 1), steps)
        assert torch.equal(done, infos.outcome > 0)
        want = steps.to(dtype) / torch.full_like(obs[:, 0], 1000)                    # true division
        assert torch.equal(obs[:, 0], want) if dtype == torch.float64 else bool(((obs[:, 0] - want).abs() <= 1.2e-7 * want).all())
        psi = full.own_psi
        assert bool(((psi >= 0) & (psi <= 360)).all())
        assert bool(torch.isfinite(obs[:, [0, 1, 2, 3, 4]]).all()) and bool(torch.isfinite(rew).all())
        assert bool((obs[:, 5::3] >= 0).all())                                  # distances
        # a finished env collected the terminal bonus that its outcome implies
        oc = infos.outcome
        assert bool((rew[oc == 2] < -900).all()) and bool((rew[oc == 1] > 900).all())
        assert bool((rew[~done].abs() <= 1.0 + 1e-6).all())
        total_done += int(done.sum())
        prev_steps = steps.clone()
    assert total_done > 0


def test_linearity_of_motion_at_one_million_envs(g):
    """Size-independent physics properties at 1 M envs: with action 0 every aircraft moves
    exactly v*dt = 2 px per step along its heading and headings are unchanged."""
    E, N = 1 << 20, 8
    env = g.ACAS2DVecEnv(E, N, device="cuda:0", dtype=torch.float64, seed=21, auto_reset=False)
    env.reset()
    x0, y0, psi0 = env.own_x.clone(), env.own_y.clone(), env.own_psi.clone()
    tx0, ty0, tpsi0 = env.trf_x.clone(), env.trf_y.clone(), env.trf_psi.clone()
    env.step(torch.zeros(E, dtype=torch.float64, device="cuda:0"))
    live = env.status == 0
    d_own = torch.hypot(env.own_x - x0, env.own_y - y0)
    d_trf = torch.hypot(env.trf_x - tx0, env.trf_y - ty0)
    assert float((d_own - 2.0).abs().max()) < 1e-9 and float((d_trf - 2.0).abs().max()) < 1e-9
    assert torch.equal(env.own_psi, psi0) and torch.equal(env.trf_psi, tpsi0)
    rad = torch.deg2rad(psi0)
    assert float((env.own_x - x0 - 2 * torch.cos(rad)).abs().max()) < 1e-9
    assert int(live.sum()) > 0


def test_plain_cpp_host_program_on_the_c_abi_matches_the_python_host(g):
    """examples/c_abi_example.cpp: hipMalloc + acas2d_reset_f32 + acas2d_step_f32 from C++, no Python
    and no torch in the process.  Same seed, same constant action 0, auto-reset: it must count the same
    finished episodes and end on the same observations as ACAS2DVecEnv."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "c_abi_example")
    subprocess.run(["make", "-C", os.path.join(root, "gym-acas2d_amd", "csrc"), "example"], check=True,
                   capture_output=True)
    E, N, T = 3000, 3, 450
    out = subprocess.run([exe, str(E), str(N), str(T)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(out[0]), int(out[1]), int(out[2])] == [E, N, T]
    v = g.ACAS2DVecEnv(E, N, device="cuda:0", dtype=torch.float32, seed=13)
    v.reset()
    zero = torch.zeros(E, device="cuda:0")
    finished, reward_sum = 0, 0.0
    for _ in range(T):
        obs, rew, done, _ = v.step(zero)
        finished += int(done.sum())
        reward_sum += float(rew.double().sum())
    w = (1 + torch.arange(obs.numel(), device="cuda:0") % 7).double()
    checksum = float((obs.reshape(-1).double() * w).sum())
    assert finished > 0 and int(out[3]) == finished
    assert abs(float(out[4]) - reward_sum) <= 1e-9 * abs(reward_sum)
    assert abs(float(out[5]) - checksum) <= 1e-9 * abs(checksum)


def test_c_abi_rejects_bad_arguments_on_gpu_box(g):
    import ctypes as C
    L = g.native.lib()
    assert L.acas2d_step_f32(None, None, None, None, 0, 0, 0, 16, 1, None) == -22
    assert b"NULL" in L.acas2d_last_error()


# ---- every compiled work shape (helpers.SHAPES; tests/test_host.py holds the table to the .hip lists) ---------------
_STATE = ("own_x", "own_y", "own_psi", "own_v", "goal_x", "goal_y", "trf_x", "trf_y", "trf_psi", "trf_v")
_PACKED = [s for s in H.SHAPES if s.packed]


def _ids(rows):
    return [s.id for s in rows]


def _use_shape(g, monkeypatch, shape, E=1000):
    """Route every launch of this test to `shape` (ACAS2D_SHAPE is read per launch) and check that it does."""
    if shape.override is None:
        monkeypatch.delenv("ACAS2D_SHAPE", raising=False)
    else:
        monkeypatch.setenv("ACAS2D_SHAPE", shape.override)
    monkeypatch.delenv("ACAS2D_NO_ARENA", raising=False)
    geo = g.native.launch_geometry(E, shape.n_traffic, shape.elem)
    assert (geo["lanes_per_env"], geo["traffic_per_lane"]) == (shape.G, shape.C if shape.packed else -1), shape.id


def _shape_env(g, shape, E, seed=21, env_offset=37, **kw):
    cfg_kw = kw.pop("config", {})
    cfg = g.ACAS2DConfig(n_traffic=shape.n_traffic, fast_math=(shape.math == "fast"), **cfg_kw)
    return g.ACAS2DVecEnv(E, device="cuda:0", dtype=getattr(torch, shape.dtype), seed=seed, env_offset=env_offset,
                          config=cfg, **kw)


def _engine(v):
    e = GpuEngine.__new__(GpuEngine)
    e.v, e.E, e.N = v, v.num_envs, v.n_traffic
    return e


def _same_state(a, b, names=_STATE + ("steps", "total_reward", "episode")):
    for name in names:
        assert bits_equal(getattr(a, name), getattr(b, name)), name


# short episodes (timeouts at step 40 / 80) so that whole episodes, resets and re-resets fit in a few dozen steps
_SHORT = dict(max_steps=40)


@pytest.mark.parametrize("auto_reset", (True, False), ids=("auto_reset", "latching"))
@pytest.mark.parametrize("shape", [s for s in H.SHAPES if s.dtype == "float64"],
                         ids=_ids([s for s in H.SHAPES if s.dtype == "float64"]))
def test_every_f64_shape_vs_oracle(g, O, monkeypatch, shape, auto_reset):
    """Whole episodes on every float64 work shape and formulation against the oracle, env for env: E = 1001 (a partial
    last wave and workgroup), env_offset 37, max_steps 80 so that every env finishes (and is reset) at least twice.
    Observations, rewards, returns to 1e-9; masks, steps, episode counters and the reset states bit for bit.  With
    auto_reset=False: the latching step -- status latches the outcome, the player moves on, the traffic is frozen."""
    _use_shape(g, monkeypatch, shape)
    E, N, T = 1001, shape.n_traffic, 170
    v = _shape_env(g, shape, E, seed=99, auto_reset=auto_reset, config=dict(max_steps=80))
    ref = O.OracleEnvs(E, N, seed=99, env_offset=37, auto_reset=auto_reset, config=_oracle_config_from(O, v.config))
    env = _engine(v)
    o_ref, o_gpu = ref.reset(), env.reset()
    for name in _STATE:
        assert np.array_equal(getattr(env, name), getattr(ref, name)), name
    np.testing.assert_allclose(o_gpu, o_ref, rtol=0, atol=1e-9)
    rng = np.random.default_rng(1)
    dones = 0
    for t in range(T):
        a = rng.uniform(-1, 1, E)
        o1, r1, d1, oc1, _ = ref.step(a)
        o2, r2, d2, oc2, _ = env.step(a)
        assert np.array_equal(d1, d2) and np.array_equal(oc1, oc2), t
        np.testing.assert_allclose(o2, o1, rtol=0, atol=1e-9, equal_nan=True)
        np.testing.assert_allclose(r2, r1, rtol=0, atol=1e-9, equal_nan=True)
        assert np.array_equal(env.steps, ref.steps) and np.array_equal(env.episode, ref.episode)
        np.testing.assert_allclose(env.total_reward, ref.total_reward, rtol=0, atol=1e-9, equal_nan=True)
        d = d1.astype(bool)
        if auto_reset and d.any():
            dones += int(d.sum())
            np.testing.assert_allclose(env.term_obs[d], ref.term_obs[d], rtol=0, atol=1e-9, equal_nan=True)
            np.testing.assert_allclose(env.ep_return[d], ref.ep_return[d], rtol=0, atol=1e-9, equal_nan=True)
            assert np.array_equal(env.ep_steps[d], ref.ep_steps[d])
            for name in _STATE:                                   # the fresh episode: bit for bit
                assert np.array_equal(getattr(env, name)[d], getattr(ref, name)[d]), (t, name)
        if not auto_reset:
            assert np.array_equal(env.status, ref.status), t
            for name in ("own_x", "own_y", "own_psi", "trf_x", "trf_y"):
                np.testing.assert_allclose(getattr(env, name), getattr(ref, name), rtol=0, atol=1e-9)
    if auto_reset:
        assert dones > E and (ref.episode >= 2).all()
    else:
        assert (ref.status != 0).all() and (ref.status == 3).any()        # every env latched; frozen traffic compared above


@pytest.mark.parametrize("shape", [s for s in H.SHAPES if s.dtype == "float32"],
                         ids=_ids([s for s in H.SHAPES if s.dtype == "float32"]))
def test_every_f32_shape_vs_f64_oracle(g, O, monkeypatch, shape):
    """Every float32 work shape against the float64 oracle, step by step from the oracle's state rounded to float32,
    with the criteria and tolerances of test_full_size_f32_vs_f64_oracle (_check_f32_step_vs_oracle); E = 1001."""
    _use_shape(g, monkeypatch, shape)
    tot = _f32_steps_vs_oracle(g, O, 1001, shape.n_traffic, 12, env_offset=37)
    _print_f32_totals("on %s, 1001 envs x 12 steps" % shape.id, tot)


@pytest.mark.parametrize("shape", _PACKED, ids=_ids(_PACKED))
def test_every_packed_shape_rollout_equals_steps(g, monkeypatch, shape):
    """acas2d_rollout_* == the same number of acas2d_step_* calls, bit for bit, on every packed work shape (the fused
    rollout has no generic walk): outputs, side channels where done, the final state."""
    _rollout_equals_steps(g, monkeypatch, shape, _SHORT)


def _rollout_equals_steps(g, monkeypatch, shape, config, **keys):
    """keys: seed / env_offset of both envs (_shape_env's by default) and `episode0`, the episode counters after reset()."""
    _use_shape(g, monkeypatch, shape)
    E, T = 1001, 90
    episode0 = keys.pop("episode0", None)
    a = _shape_env(g, shape, E, config=config, **keys)
    b = _shape_env(g, shape, E, config=config, double_buffer=False, **keys)
    assert bits_equal(a.reset(), b.reset())
    if episode0 is not None:
        for v in (a, b):
            v.episode.copy_(torch.as_tensor(episode0.view(np.int32), device="cuda:0"))
    gen = torch.Generator(device="cuda:0").manual_seed(3)
    actions = torch.rand(T, E, generator=gen, device="cuda:0", dtype=a.dtype) * 2 - 1
    out = a.rollout(actions, keep_terminal_obs=True)
    dones = 0
    for t in range(T):
        obs, rew, done, infos = b.step(actions[t])
        assert bits_equal(out["obs"][t], obs) and bits_equal(out["reward"][t], rew), t
        assert torch.equal(out["done"][t], done) and torch.equal(out["outcome"][t], infos.outcome), t
        if bool(done.any()):
            dones += int(done.sum())
            for k, want in (("episode_return", infos.episode_return), ("episode_steps", infos.episode_steps),
                            ("terminal_observation", infos.terminal_observation)):
                assert bits_equal(out[k][t][done], want[done]), (t, k)
    assert dones >= E
    _same_state(a, b)
    if episode0 is not None:                               # preset counters wrapped inside the window
        assert int((a.episode[torch.as_tensor(episode0 != 0, device="cuda:0")] >= 0).sum()) >= 50


@pytest.mark.parametrize("shape", H.SHAPES, ids=_ids(H.SHAPES))
def test_every_shape_double_buffered_equals_in_place(g, monkeypatch, shape):
    """A separate state_out (two generations) == stepping in place, bit for bit, on every work shape."""
    _use_shape(g, monkeypatch, shape)
    E, T = 1001, 90
    a = _shape_env(g, shape, E, config=_SHORT, double_buffer=True)
    b = _shape_env(g, shape, E, config=_SHORT, double_buffer=False)
    assert bits_equal(a.reset(), b.reset())
    gen = torch.Generator(device="cuda:0").manual_seed(4)
    actions = torch.rand(T, E, generator=gen, device="cuda:0", dtype=a.dtype) * 2 - 1
    dones = 0
    for t in range(T):
        oa, ra, da, _ = a.step(actions[t])
        ob, rb, db, _ = b.step(actions[t])
        assert a.generation == (t + 1) % 2
        assert bits_equal(oa, ob) and bits_equal(ra, rb) and torch.equal(da, db), t
        for k in ("outcome", "terminal_observation", "episode_return", "episode_steps"):
            assert bits_equal(a.outputs[k], b.outputs[k]), (t, k)
        dones += int(da.sum())
    assert dones >= E
    _same_state(a, b)


_F32_PACKED = [s for s in _PACKED if s.dtype == "float32"]


@pytest.mark.parametrize("shape", _F32_PACKED, ids=_ids(_F32_PACKED))
def test_every_f32_packed_shape_arena_equals_general(g, monkeypatch, shape):
    """The consecutive-layout ("arena") step kernel == the general kernel (ACAS2D_NO_ARENA, read per launch), bit for
    bit, on every float32 packed shape; E = 32 waves, a whole multiple of eight workgroups (the arena kernel's size)."""
    _arena_equals_general(g, monkeypatch, shape, _SHORT)


def _arena_equals_general(g, monkeypatch, shape, config):
    E, T = 32 * shape.envs_per_wave, 90
    _use_shape(g, monkeypatch, shape, E)
    a = _shape_env(g, shape, E, config=config)
    b = _shape_env(g, shape, E, config=config)
    assert a.consecutive_layout
    assert bits_equal(a.reset(), b.reset())
    gen = torch.Generator(device="cuda:0").manual_seed(5)
    actions = torch.rand(T, E, generator=gen, device="cuda:0") * 2 - 1
    dones = 0
    for t in range(T):
        oa, ra, da, _ = a.step(actions[t])
        monkeypatch.setenv("ACAS2D_NO_ARENA", "1")
        assert not b.consecutive_layout
        ob, rb, db, _ = b.step(actions[t])
        monkeypatch.delenv("ACAS2D_NO_ARENA")
        assert bits_equal(oa, ob) and bits_equal(ra, rb) and torch.equal(da, db), t
        for k in ("outcome", "terminal_observation", "episode_return", "episode_steps"):
            assert bits_equal(a.outputs[k], b.outputs[k]), (t, k)
        dones += int(da.sum())
    assert dones >= E
    _same_state(a, b)


_F64 = [s for s in H.SHAPES if s.dtype == "float64"]


@pytest.mark.parametrize("shape", _F64, ids=_ids(_F64))
def test_every_f64_shape_reset_masked_vs_oracle(g, O, monkeypatch, shape):
    """reset_masked() (reset_kernel on a mask) against the oracle's Philox reset of the same envs: the re-drawn envs bit
    for bit, their first observation to 1e-9, every other env untouched."""
    _use_shape(g, monkeypatch, shape)
    E, N = 1001, shape.n_traffic
    v = _shape_env(g, shape, E, seed=7)
    ref = O.OracleEnvs(E, N, seed=7, env_offset=37, auto_reset=True)
    env = _engine(v)
    ref.reset()
    env.reset()
    rng = np.random.default_rng(6)
    for frac in (0.5, 0.2, 0.9):
        mask = rng.random(E) < frac
        before = {name: getattr(env, name).copy() for name in _STATE + ("steps", "episode")}
        obs = env._np(v.reset_masked(torch.as_tensor(mask, device="cuda:0")))
        ref.episode[mask] += 1
        ref.reset_philox(mask.astype(np.uint8))
        for name in _STATE:
            got = getattr(env, name)
            assert np.array_equal(got[mask], getattr(ref, name)[mask]), name
            assert np.array_equal(got[~mask], before[name][~mask]), name
        assert np.array_equal(env.episode, ref.episode) and np.array_equal(env.steps[~mask], before["steps"][~mask])
        o_ref = ref.observe()                               # (observes every env: steps compared on the mask only)
        np.testing.assert_allclose(obs[mask], o_ref[mask], rtol=0, atol=1e-9)
        assert np.array_equal(env.steps[mask], ref.steps[mask])
        ref.steps[~mask] = before["steps"][~mask]


# ---- the float32 build under non-default configurations (helpers.NONDEFAULT_CONFIGS) ---------------------------------
# Under the default configuration every aircraft flies at exactly `airspeed`: the float32 speed draw, the kinematics.py:74
# quirk of the paired float2 path (v2y from the PLAYER's speed), the float32 rounding of the configuration and its
# reciprocals, and timeouts / the step-reward decay at another max_steps are seen by the tests above only at their
# default values.
_F32_SHAPES = [s for s in H.SHAPES if s.dtype == "float32"]


@pytest.mark.parametrize("name", tuple(H.NONDEFAULT_CONFIGS))
@pytest.mark.parametrize("shape", _F32_SHAPES, ids=_ids(_F32_SHAPES))
def test_every_f32_shape_nondefault_config_vs_f64_oracle(g, O, monkeypatch, shape, name):
    """Every float32 work shape under each non-default configuration against the float64 oracle, step by step from the
    oracle's state rounded to float32 (_f32_steps_vs_oracle; bounds derived from the configuration); E = 1001, env_offset
    37, the window of helpers.NONDEFAULT_SHAPE_WINDOW: it covers timeouts, and under "small" goals -- every outcome the
    oracle produces there (helpers.nondefault_outcomes) must have been compared."""
    _use_shape(g, monkeypatch, shape)
    w = H.NONDEFAULT_SHAPE_WINDOW[name]
    tot = _f32_steps_vs_oracle(g, O, 1001, shape.n_traffic, w["T"], seed=w["seed"], env_offset=w["env_offset"],
                               config=H.NONDEFAULT_CONFIGS[name], warmup=w["warmup"])
    _print_f32_totals('"%s" on %s, 1001 envs x %d steps after %d' % (name, shape.id, w["T"], w["warmup"]), tot)
    assert tot["speeds"] > 10                                          # speeds really vary
    assert tot["outcomes"] >= H.nondefault_outcomes(name, shape.n_traffic), tot["outcomes"]


@pytest.mark.parametrize("N,E,T", _ODD_TRAFFIC)
def test_f32_odd_traffic_counts_and_nondefault_config_vs_f64_oracle(g, O, N, E, T):
    """The float32 twin of test_f64_odd_traffic_counts_and_nondefault_config_vs_oracle: the same traffic counts, env
    counts and "wide" configuration, stepped from the oracle's state rounded to float32 (_f32_steps_vs_oracle) in a window
    that starts at step 100, so that both collisions and timeouts are compared."""
    tot = _f32_steps_vs_oracle(g, O, E, N, T, config=H.NONDEFAULT_CONFIGS["wide"], **H.NONDEFAULT_ODD_WINDOW)
    _print_f32_totals('"wide" at %d x %d over %d steps' % (E, N, T), tot)
    assert tot["speeds"] > 10
    assert tot["outcomes"] >= {H.COLLISION, H.TIMEOUT}, tot["outcomes"]


@pytest.mark.parametrize("name", tuple(H.NONDEFAULT_CONFIGS))
def test_f32_reset_names_the_same_episodes_nondefault(g, O, name):
    """test_f32_reset_names_the_same_episodes under a non-default configuration with an airspeed-factor range: the draws
    of reset() and of the in-step reset within the bounds of helpers.f32_bounds (speeds included), and reset_kernel on a
    twin env bit for bit what the step drew."""
    E, N = 4096, 8
    cfg = g.ACAS2DConfig(n_traffic=N, **H.NONDEFAULT_CONFIGS[name])
    ref = O.OracleEnvs(E, N, seed=5, auto_reset=True, config=_oracle_config_from(O, cfg))
    bnd = H.f32_bounds(ref.cfg, _default_oracle_config())
    assert bnd["speed"] is not None
    worst = dict(pos=0.0, psi=0.0, speed=0.0)

    def close_to_oracle(env, sel):
        e = max(np.abs(env.trf_x[sel] - ref.trf_x[sel]).max(), np.abs(env.trf_y[sel] - ref.trf_y[sel]).max())
        worst["pos"] = max(worst["pos"], float(e))
        assert e < bnd["reset_pos"], e
        for k in ("trf_psi", "own_psi"):
            dpsi = np.abs(getattr(env, k)[sel] - getattr(ref, k)[sel])
            worst["psi"] = max(worst["psi"], float(np.minimum(dpsi, 360 - dpsi).max()))
            assert np.minimum(dpsi, 360 - dpsi).max() < bnd["reset_psi"], k
        e = np.abs(env.trf_v[sel] - ref.trf_v[sel]).max()
        worst["speed"] = max(worst["speed"], float(e))
        assert e <= bnd["speed"], e

    ref.reset()
    env = _engine(g.ACAS2DVecEnv(E, device="cuda:0", dtype=torch.float32, auto_reset=True, seed=5, config=cfg))
    env.reset()
    close_to_oracle(env, np.ones(E, bool))
    assert len(np.unique(env.trf_v)) > 10                       # speeds really vary
    rng = np.random.default_rng(3)
    checked = 0
    twin = g.ACAS2DVecEnv(E, device="cuda:0", dtype=torch.float32, auto_reset=True, seed=5, config=cfg)
    for _ in range(40):
        a = rng.uniform(-1, 1, E).astype(np.float32).astype(np.float64)
        _, _, d1, _, _ = ref.step(a)
        _, _, d2, _, _ = env.step(a)
        both = (d1 != 0) & (d2 != 0) & (env.episode == ref.episode)
        if both.any():
            checked += int(both.sum())
            close_to_oracle(env, both)
        fresh = torch.as_tensor(d2 != 0, device="cuda:0")
        if fresh.any():
            twin.episode.copy_(env.v.episode)
            twin._launch_reset(fresh.to(torch.uint8), do_init=1)
            for k in _STATE:
                assert torch.equal(getattr(twin, k)[fresh], getattr(env.v, k)[fresh]), k
            assert bits_equal(twin.outputs["obs"][fresh], env.v.outputs["obs"][fresh])
    print('f32 reset draws under "%s": %d in-step resets checked; worst positions %.2e (bound %.2e), headings %.2e (bound '
          '%.0e), speeds %.2e (bound %.2e)' % (name, checked, worst["pos"], bnd["reset_pos"], worst["psi"], bnd["reset_psi"],
                                             worst["speed"], bnd["speed"]))
    assert checked > 50


@pytest.mark.parametrize("shape", _F32_PACKED, ids=_ids(_F32_PACKED))
def test_every_f32_packed_shape_rollout_equals_steps_nondefault(g, monkeypatch, shape):
    """test_every_packed_shape_rollout_equals_steps on the float32 packed shapes under the "small" configuration."""
    _rollout_equals_steps(g, monkeypatch, shape, H.NONDEFAULT_CONFIGS["small"])


@pytest.mark.parametrize("shape", _F32_PACKED, ids=_ids(_F32_PACKED))
def test_every_f32_packed_shape_arena_equals_general_nondefault(g, monkeypatch, shape):
    """test_every_f32_packed_shape_arena_equals_general under the "small" configuration."""
    _arena_equals_general(g, monkeypatch, shape, H.NONDEFAULT_CONFIGS["small"])


# ---- waves whose envs finish together -----------------------------------------------------------------------------
def _wave_variants(shape):
    if shape.dtype == "float32" and shape.packed:
        vs = ("inplace-arena", "inplace-general", "double-arena", "double-general", "rollout")
    else:
        vs = ("inplace", "double") + (("rollout",) if shape.packed else ())
    return [(shape, v) for v in vs]


_WAVE_CASES = [c for s in H.SHAPES for c in _wave_variants(s)]
# injected own_v / goal other than the configuration's: the reset must write the configuration's back
_CONSTS_CASES = [(s, "consts") for s in H.SHAPES if s.override is None and s.n_traffic in (5, 8, 64)]
# at the wide reset keys (helpers.WIDE_SEED, the 2^32 crossing of the global env index inside the middle wave, which
# finishes whole; episode counters at 2^32 - 2 .. 2): the in-place step (float32: both kernels) and the rollout
_WIDE_WAVE_CASES = [(s, "wide-" + v) for s, v in _WAVE_CASES if not v.startswith("double")]


@pytest.mark.parametrize("shape,variant", _WAVE_CASES + _CONSTS_CASES + _WIDE_WAVE_CASES,
                         ids=["%s-%s" % (s.id, v) for s, v in _WAVE_CASES + _CONSTS_CASES + _WIDE_WAVE_CASES])
def test_waves_finishing_together_vs_oracle(g, O, monkeypatch, shape, variant):
    """The in-step reset takes a wave's finished envs SLOTS at a time (a packed shape with N + 1 <= 32: SLOTS = 64 /
    the power of two >= max(2, N + 1), geometry_for() / ResetSlots; otherwise one per pass).  A step where a chosen
    number of envs of each wave finish -- 0, 1, SLOTS, SLOTS + 1, wave - 1 and the whole wave, varied across the 32
    waves of one launch -- forced by injecting steps = max_steps (observe() counts it past max_steps and the timeout
    outranks collision and goal, oracle/acas2d_oracle.c is_done).  Against the oracle with the float64 criteria
    (1e-9, masks and reset states bit for bit) or the float32 ones (_check_f32_step_vs_oracle): the terminal
    observation, return and length, the fresh episode and its first observation, and the untouched envs -- for the
    step kernel in place and double-buffered (float32: the arena kernel and the general one) and for rollout().
    "consts": the injected states fly at own_v = 190 towards goal (1400, 520); the reset restores 200 / (1456, 500).
    "wide-*": at helpers.WIDE_SEED, the global env index crossing 2^32 inside the middle wave, whose envs all finish,
    and episode counters 2^32 - 2 .. 2 (the resets from 2^32 - 1 wrap to 0)."""
    wide = variant.startswith("wide-")
    variant = variant[5:] if wide else variant
    f32 = shape.dtype == "float32"
    wave = shape.envs_per_wave
    E, N = 32 * wave, shape.n_traffic                          # a whole multiple of eight workgroups (the arena kernel)
    _use_shape(g, monkeypatch, shape, E)
    cfg = g.ACAS2DConfig(n_traffic=N, fast_math=(shape.math == "fast"))
    cfgc = _oracle_config_from(O, cfg)
    rnd = (lambda a: a.astype(np.float32).astype(np.float64)) if f32 else (lambda a: a)
    band = 1e-3 if f32 else 1e-9
    # ---- candidate mid-episode states (oracle), keep those that neither finish nor graze a threshold on this step
    P = 4 * E
    pool = O.OracleEnvs(P, N, seed=31, auto_reset=True, config=cfgc)
    pool.reset()
    rng = np.random.default_rng(8)
    for _ in range(12):
        pool.step(rng.uniform(-1, 1, P))
    own = rnd(np.stack([pool.own_x, pool.own_y, pool.own_psi, pool.own_v], 1))
    trf = rnd(np.stack([pool.trf_x, pool.trf_y, pool.trf_psi, pool.trf_v], -1))
    goal = np.broadcast_to(np.array([cfgc.goal_x, cfgc.goal_y]), (P, 2)).copy()
    if variant == "consts":
        own[:, 3], goal[:] = 190.0, (1400.0, 520.0)
    steps0, act = pool.steps.copy(), rnd(rng.uniform(-1, 1, P))
    trial = O.OracleEnvs(P, N, config=cfgc)
    trial.set_state(own, trf, goal, steps0)
    o, _, d, _, _ = trial.step(act)
    keep = np.nonzero((d == 0) & ~grazing(o, N, cfgc, band) & (steps0 < cfgc.max_steps - 1))[0]
    assert len(keep) >= E, len(keep)
    keep = keep[:E]
    own, trf, goal, steps, act = own[keep], trf[keep], goal[keep], steps0[keep].copy(), act[keep]
    # ---- the envs that finish: a chosen number per wave
    counts = sorted({c for c in (0, 1, shape.reset_slots, shape.reset_slots + 1, wave - 1, wave) if 0 <= c <= wave})
    chosen = np.zeros(E, bool)
    for w in range(E // wave):
        k = counts[(w + len(counts) // 2) % len(counts)]          # every count, at different waves
        chosen[w * wave + rng.choice(wave, k, replace=False)] = True
    seed, off = 21, 37
    if wide:
        seed, off = H.WIDE_SEED, H.wide_crossing_offset(E, wave)
        w = (2 ** 32 - off) // wave
        chosen[w * wave:(w + 1) * wave] = True
    steps[chosen] = cfgc.max_steps
    episode = rng.integers(0, 5, E).astype(np.uint32)
    if wide:
        episode = ((episode.astype(np.int64) + H.WIDE_EPISODE) % 2 ** 32).astype(np.uint32)
    chk = O.OracleEnvs(E, N, seed=seed, env_offset=off, auto_reset=True, config=cfgc)
    chk.set_state(own, trf, goal, steps)
    chk.episode[:] = episode
    o, r, d, oc, _ = chk.step(act)
    assert np.array_equal(oc == 3, chosen) and np.array_equal(d != 0, chosen)      # the setup: exactly the chosen envs
    # ---- the engine
    kind = variant.split("-")[0]
    v = g.ACAS2DVecEnv(E, device="cuda:0", dtype=getattr(torch, shape.dtype), seed=seed, env_offset=off, config=cfg,
                       double_buffer=(kind == "double"))
    if variant.endswith("general"):
        monkeypatch.setenv("ACAS2D_NO_ARENA", "1")
    if variant.endswith(("arena", "general")):
        assert v.consecutive_layout == variant.endswith("arena")
    v.set_state(own, trf, goal, steps, observe=False)
    v.episode.copy_(torch.as_tensor(episode.view(np.int32), device="cuda:0"))
    env = _engine(v)
    a = torch.as_tensor(act, dtype=v.dtype, device="cuda:0")
    if kind == "rollout":
        out = v.rollout(a.reshape(1, E), keep_terminal_obs=True)
        got = {k: env._np(out[k][0]) for k in ("obs", "reward", "done", "outcome", "terminal_observation",
                                               "episode_return", "episode_steps")}
    else:
        v.step(a)
        got = {k: env._np(t) for k, t in v.outputs.items()}
    monkeypatch.delenv("ACAS2D_NO_ARENA", raising=False)
    if wide and variant == "inplace-arena":                 # the arena kernel == the general one, bit for bit
        twin = g.ACAS2DVecEnv(E, device="cuda:0", dtype=v.dtype, seed=seed, env_offset=off, config=cfg, double_buffer=False)
        twin.set_state(own, trf, goal, steps, observe=False)
        twin.episode.copy_(torch.as_tensor(episode.view(np.int32), device="cuda:0"))
        monkeypatch.setenv("ACAS2D_NO_ARENA", "1")
        assert not twin.consecutive_layout
        twin.step(a)
        monkeypatch.delenv("ACAS2D_NO_ARENA")
        for k in v.outputs:
            assert bits_equal(v.outputs[k], twin.outputs[k]), k
        _same_state(v, twin, _STATE + ("steps", "total_reward", "episode", "status"))
    snap =types.SimpleNamespace(**{n: getattr(env, n) for n in _STATE + ("steps", "total_reward", "episode")})
    snap.term_obs, snap.ep_return, snap.ep_steps = got["terminal_observation"], got["episode_return"], got["episode_steps"]
    obs, rew, done, outcome = got["obs"], got["reward"], got["done"].astype(np.uint8), got["outcome"]
    print("%s %s: %d envs, %d finish (per wave: %s; SLOTS %d)" % (shape.id, variant, E, chosen.sum(), counts,
                                                                 shape.reset_slots))
    if f32:
        tot = _new_f32_totals()
        go, fin = _check_f32_step_vs_oracle(snap, chk, (o, r, d, oc), (obs, rew, done, outcome), N, tot)
        _print_f32_totals("%s %s" % (shape.id, variant), tot)
        assert np.array_equal(fin, chosen) and np.array_equal(go, ~chosen)           # nothing set aside in the band
        assert np.array_equal(snap.episode, chk.episode)
        assert np.array_equal(snap.trf_v, chk.trf_v)
        assert np.array_equal(snap.trf_psi[~chosen], trf[~chosen, :, 2])        # untouched envs: the injected headings
    else:
        assert np.array_equal(done, d) and np.array_equal(outcome, oc)
        np.testing.assert_allclose(obs, o, rtol=0, atol=1e-9, equal_nan=True)
        np.testing.assert_allclose(rew, r, rtol=0, atol=1e-9, equal_nan=True)
        np.testing.assert_allclose(snap.term_obs[chosen], chk.term_obs[chosen], rtol=0, atol=1e-9, equal_nan=True)
        np.testing.assert_allclose(snap.ep_return[chosen], chk.ep_return[chosen], rtol=0, atol=1e-9)
        assert np.array_equal(snap.ep_steps[chosen], chk.ep_steps[chosen])
        for name in _STATE:
            want = getattr(chk, name)
            if name in ("own_x", "own_y", "own_psi", "trf_x", "trf_y"):
                assert np.array_equal(getattr(snap, name)[chosen], want[chosen]), name      # the fresh episode
                np.testing.assert_allclose(getattr(snap, name), want, rtol=0, atol=1e-9, err_msg=name)
            else:
                assert np.array_equal(getattr(snap, name), want), name
        assert np.array_equal(snap.steps, chk.steps) and np.array_equal(snap.episode, chk.episode)
        np.testing.assert_allclose(snap.total_reward, chk.total_reward, rtol=0, atol=1e-9)
    # both: the finished envs restart at the configuration's own_v / goal, the others keep what was injected
    assert (snap.steps[chosen] == 1).all() and (snap.ep_steps[chosen] == cfgc.max_steps + 1).all()
    assert (snap.own_v[chosen] == cfgc.own_v).all() and (snap.goal_x[chosen] == cfgc.goal_x).all()
    assert (snap.goal_y[chosen] == cfgc.goal_y).all()
    assert np.array_equal(snap.own_v[~chosen], own[~chosen, 3]) and np.array_equal(snap.goal_x[~chosen], goal[~chosen, 0])
    assert np.array_equal(snap.goal_y[~chosen], goal[~chosen, 1])
    assert np.array_equal(snap.episode, (episode + chosen).astype(np.uint32))
    if wide:
        assert ((snap.episode == 0) & chosen).sum() >= (2 if wave >= 4 else 0) and (off + E) >> 32 == 1


# ---- the headline configuration as bench.py measures it ------------------------------------------------------------
def test_benched_step_runner_equals_the_general_kernel_in_place(g, monkeypatch):
    """65 536 envs x 8 float32 as bench.py runs them: the default ACAS2DVecEnv (consecutive "arena" layout, double-
    buffered), bench.StepRunner's captured graph of 10 steps over a ring of 4 action rows, replayed several times with
    an odd number of eager steps in between (the runner re-aligns the state generation).  A twin env stepped eagerly
    through the general kernel in place (ACAS2D_NO_ARENA, double_buffer=False) must agree bit for bit after every
    replay: outputs, side channels and the full state.  The kernel is chosen when the graph is CAPTURED, so
    ACAS2D_NO_ARENA is set around the twin's launches only."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    E, N, ROWS, GRAPH = 65536, 8, 4, 12
    monkeypatch.delenv("ACAS2D_NO_ARENA", raising=False)
    monkeypatch.delenv("ACAS2D_SHAPE", raising=False)
    a = g.ACAS2DVecEnv(E, N, device="cuda:0", seed=13)
    b = g.ACAS2DVecEnv(E, N, device="cuda:0", seed=13, double_buffer=False)
    assert a.double_buffer and a.consecutive_layout and not b.double_buffer
    assert bits_equal(a.reset(), b.reset())
    gen = torch.Generator(device="cuda:0").manual_seed(1000)
    actions = torch.rand(ROWS, E, generator=gen, device="cuda:0") * 2 - 1

    def twin(n):                                   # what StepRunner.eager(n) / one replay steps: rows t % ROWS
        monkeypatch.setenv("ACAS2D_NO_ARENA", "1")
        for t in range(n):
            b.step_from(actions[t % ROWS])
        monkeypatch.delenv("ACAS2D_NO_ARENA")

    runner = bench.StepRunner(a, actions, True, GRAPH)          # 3 eager steps, then the capture (nothing runs)
    assert runner.graph is not None and a.double_buffer and a.generation == runner.gen0 == 1
    twin(3)
    dones = 0
    for rep, eager in enumerate((0, 3, 0, 5, 1)):
        if eager:
            runner.eager(eager)
            twin(eager)
        runner.run(GRAPH)
        twin(GRAPH)
        torch.cuda.synchronize()
        for k in ("obs", "reward", "done", "outcome", "terminal_observation", "episode_return", "episode_steps"):
            assert bits_equal(a.outputs[k], b.outputs[k]), (rep, k)
        _same_state(a, b, _STATE + ("steps", "total_reward", "episode", "status"))
        dones += int(a.outputs["done"].sum())
    assert dones > 0 and int(a.episode.sum()) > 1000          # resets in the replayed steps


def test_arena_kernel_in_place_at_the_per_rank_shard_size(g, monkeypatch):
    """131 072 envs x 8 float32 (the per-rank shard of the 8-GPU BASELINE configuration): the default env there steps
    in place through the arena kernel; against the general kernel (ACAS2D_NO_ARENA), bit for bit, over 60 steps with
    resets in every one."""
    E, N, T = 131072, 8, 60
    monkeypatch.delenv("ACAS2D_SHAPE", raising=False)
    monkeypatch.delenv("ACAS2D_NO_ARENA", raising=False)
    a = g.ACAS2DVecEnv(E, N, device="cuda:0", seed=13)
    b = g.ACAS2DVecEnv(E, N, device="cuda:0", seed=13)
    assert not a.double_buffer and a.consecutive_layout
    assert bits_equal(a.reset(), b.reset())
    gen = torch.Generator(device="cuda:0").manual_seed(9)
    actions = torch.rand(T, E, generator=gen, device="cuda:0") * 2 - 1
    dones = 0
    for t in range(T):
        oa, ra, da, _ = a.step(actions[t])
        monkeypatch.setenv("ACAS2D_NO_ARENA", "1")
        ob, rb, db, _ = b.step(actions[t])
        monkeypatch.delenv("ACAS2D_NO_ARENA")
        assert bits_equal(oa, ob) and bits_equal(ra, rb) and torch.equal(da, db), t
        for k in ("outcome", "terminal_observation", "episode_return", "episode_steps"):
            assert bits_equal(a.outputs[k], b.outputs[k]), (t, k)
        dones += int(da.sum())
    _same_state(a, b, _STATE + ("steps", "total_reward", "episode", "status"))
    assert dones > 1000


# ---- wide reset keys (helpers.WIDE_*) ---------------------------------------------------------------------------------
# Every episode is the Philox block of counter (global env index lo, hi, episode, entity) under key (seed lo, hi).  With
# small seeds, offsets and counters the high words are all 0, and a kernel that dropped one -- or added a lane's env to
# its wave's first global index in 32 bits -- would pass every test above.  These run at a seed whose halves differ, the
# 2^32 crossing of the global index inside a wave, and counters that wrap through 2^32 - 1 to 0.
# Both formulations share the reset code and the launchers: every row auto-resets at the "mid" keys; the "tail" keys and
# the latching step (whose draws are reset()'s) run in the reference formulation's rows.
_F64_EXACT = [s for s in _F64 if s.math == "exact"]
_WIDE_F64_CASES = [(s, True, "mid") for s in _F64] + [(s, True, "tail") for s in _F64_EXACT] + \
                  [(s, False, "mid") for s in _F64_EXACT]
_WIDE_MASKED_CASES = [(s, "mid") for s in _F64] + [(s, "tail") for s in _F64_EXACT]


def _wide_episode0(E):
    return np.where(H.wide_preset(E), H.WIDE_EPISODE, 0).astype(np.uint32)


@pytest.mark.parametrize("shape,auto_reset,key", _WIDE_F64_CASES,
                         ids=["%s-%s-%s" % (s.id, "auto_reset" if ar else "latching", k) for s, ar, k in _WIDE_F64_CASES])
def test_every_f64_shape_at_wide_keys_vs_oracle(g, O, monkeypatch, shape, auto_reset, key):
    """test_every_f64_shape_vs_oracle at the wide keys: reset() bit for bit, then the even envs' counters set to
    2^32 - 2 and 90 steps of max_steps 40, so that their second reset wraps the counter to 0 (auto-reset; latching: the
    reset() draws, then the latching step).  Fresh episodes bit for bit, observations 1e-9, episode counters equal."""
    _use_shape(g, monkeypatch, shape)
    E, N, T, off = H.WIDE_E, shape.n_traffic, 90, H.WIDE_OFFSET[key]
    v = _shape_env(g, shape, E, seed=H.WIDE_SEED, env_offset=off, auto_reset=auto_reset, config=_SHORT)
    ref = O.OracleEnvs(E, N, seed=H.WIDE_SEED, env_offset=off, auto_reset=auto_reset, config=_oracle_config_from(O, v.config))
    env = _engine(v)
    o_ref, o_gpu = ref.reset(), env.reset()
    for name in _STATE:
        assert np.array_equal(getattr(env, name), getattr(ref, name)), name
    np.testing.assert_allclose(o_gpu, o_ref, rtol=0, atol=1e-9)
    ref.episode[:] = _wide_episode0(E)
    v.episode.copy_(torch.as_tensor(ref.episode.view(np.int32), device="cuda:0"))
    rng = np.random.default_rng(1)
    wrapped = 0
    for t in range(T):
        a = rng.uniform(-1, 1, E)
        o1, r1, d1, oc1, _ = ref.step(a)
        o2, r2, d2, oc2, _ = env.step(a)
        assert np.array_equal(d1, d2) and np.array_equal(oc1, oc2), t
        np.testing.assert_allclose(o2, o1, rtol=0, atol=1e-9, equal_nan=True)
        np.testing.assert_allclose(r2, r1, rtol=0, atol=1e-9, equal_nan=True)
        assert np.array_equal(env.steps, ref.steps) and np.array_equal(env.episode, ref.episode), t
        d = d1.astype(bool)
        if auto_reset and d.any():
            wrapped += int((d & (ref.episode == 0)).sum())
            np.testing.assert_allclose(env.term_obs[d], ref.term_obs[d], rtol=0, atol=1e-9, equal_nan=True)
            for name in _STATE:
                assert np.array_equal(getattr(env, name)[d], getattr(ref, name)[d]), (t, name)
        if not auto_reset:
            assert np.array_equal(env.status, ref.status), t
    if auto_reset:
        print("%s at %s keys: %d resets wrapped the episode counter" % (shape.id, key, wrapped))
        assert wrapped >= 50
    else:
        assert (ref.status != 0).all()


@pytest.mark.parametrize("shape,key", _WIDE_MASKED_CASES, ids=["%s-%s" % (s.id, k) for s, k in _WIDE_MASKED_CASES])
def test_every_f64_shape_reset_masked_at_wide_keys_vs_oracle(g, O, monkeypatch, shape, key):
    """reset_masked() at the wide keys: three masked resets, the first two covering every even env (counters preset to
    2^32 - 2: the second wraps them to 0); re-drawn envs bit for bit, first observations 1e-9, the rest untouched."""
    _use_shape(g, monkeypatch, shape)
    E, N, off = H.WIDE_E, shape.n_traffic, H.WIDE_OFFSET[key]
    v = _shape_env(g, shape, E, seed=H.WIDE_SEED, env_offset=off)
    ref = O.OracleEnvs(E, N, seed=H.WIDE_SEED, env_offset=off, auto_reset=True)
    env = _engine(v)
    ref.reset()
    env.reset()
    pre = H.wide_preset(E)
    ref.episode[:] = _wide_episode0(E)
    v.episode.copy_(torch.as_tensor(ref.episode.view(np.int32), device="cuda:0"))
    rng = np.random.default_rng(6)
    for k, frac in enumerate((0.5, 0.2, 0.9)):
        mask = (rng.random(E) < frac) | (pre if k < 2 else False)
        before = {name: getattr(env, name).copy() for name in _STATE + ("steps",)}
        obs = env._np(v.reset_masked(torch.as_tensor(mask, device="cuda:0")))
        ref.episode[mask] += np.uint32(1)
        ref.reset_philox(mask.astype(np.uint8))
        for name in _STATE:
            got = getattr(env, name)
            assert np.array_equal(got[mask], getattr(ref, name)[mask]), (k, name)
            assert np.array_equal(got[~mask], before[name][~mask]), (k, name)
        assert np.array_equal(env.episode, ref.episode), k
        o_ref = ref.observe()
        np.testing.assert_allclose(obs[mask], o_ref[mask], rtol=0, atol=1e-9)
        ref.steps[~mask] = before["steps"][~mask]
        if k == 1:
            assert (env.episode[pre] == 0).all()


def test_reset_to_episode_at_the_campaign_wide_keys_vs_oracle(g, O, monkeypatch):
    """The encounters the Monte Carlo tests draw at THEIR wide keys (tests/monte_carlo_support.py: helpers.WIDE_SEED, the lane
    crossing 2^32 at local lane 37 of 70, counters 2^32 - 3 .. 2^32 - 1), by the route of the test above at the float64
    reference formulation with one aircraft: reset_to_episode(c) bit for bit against the oracle's draw of counter c, first
    observations 1e-9.  The campaign's reference and the campaign share the GPU reset; this holds what both drew to the CPU."""
    import monte_carlo_support as MS
    shape = next(s for s in _F64_EXACT if s.n_traffic == 1)
    E, N = MS.LANES, shape.n_traffic
    _use_shape(g, monkeypatch, shape, E)
    v = _shape_env(g, shape, E, seed=MS.WIDE_SEED, env_offset=MS.WIDE_LANE_OFFSET, config=dict(max_steps=150))
    ref = O.OracleEnvs(E, N, seed=MS.WIDE_SEED, env_offset=MS.WIDE_LANE_OFFSET, auto_reset=True, config=_oracle_config_from(O, v.config))
    env = _engine(v)
    ref.reset()
    every = np.ones(E, np.uint8)
    drawn = []
    for c in range(MS.WIDE_FIRST_EPISODE, MS.WIDE_FIRST_EPISODE + MS.EPISODES):
        obs = env._np(v.reset_to_episode(c))
        ref.episode[:] = np.uint32(c)
        ref.reset_philox(every)
        for name in _STATE:
            assert np.array_equal(getattr(env, name), getattr(ref, name)), (c, name)
        assert np.array_equal(env.episode, ref.episode) and (env.episode == c).all(), c
        np.testing.assert_allclose(obs, ref.observe(), rtol=0, atol=1e-9)
        drawn.append(env.trf_psi.copy())
    assert c == 2 ** 32 - 1 and not np.array_equal(drawn[0], drawn[1]) and not np.array_equal(drawn[1], drawn[2])


@pytest.mark.parametrize("key", tuple(H.WIDE_OFFSET))
@pytest.mark.parametrize("shape", _F32_SHAPES, ids=_ids(_F32_SHAPES))
def test_every_f32_shape_at_wide_keys_vs_f64_oracle(g, O, monkeypatch, shape, key):
    """Every float32 work shape at the wide keys against the float64 oracle (_f32_steps_vs_oracle, max_steps 40), in the
    window of helpers.wide_f32_window where resets wrap the preset counters: the fresh episodes within the float32
    bounds, the counters equal."""
    _use_shape(g, monkeypatch, shape)
    warmup, T = H.wide_f32_window(shape.n_traffic)
    tot = _f32_steps_vs_oracle(g, O, H.WIDE_E, shape.n_traffic, T, seed=H.WIDE_SEED, env_offset=H.WIDE_OFFSET[key],
                               config=_SHORT, warmup=warmup, episode0=_wide_episode0(H.WIDE_E))
    _print_f32_totals("at %s keys on %s, %d envs x %d steps after %d" % (key, shape.id, H.WIDE_E, T, warmup), tot)
    assert tot["finished"] > 0 and tot["wrapped"] >= 5, tot["wrapped"]


def test_f32_reset_names_the_same_episodes_at_wide_keys(g, O):
    """test_f32_reset_names_the_same_episodes at the wide keys (4096 envs x 8, the 2^32 crossing at env 2049, the even
    envs' counters at 2^32 - 2, max_steps 40 so that they wrap within 85 steps): reset() and the in-step reset within the
    float32 reset bounds of the oracle's draws, and reset_kernel on a twin bit for bit what the step drew."""
    E, N, T, off = 4096, 8, 85, 2 ** 32 - 2049
    cfg = g.ACAS2DConfig(n_traffic=N, **_SHORT)
    ref = O.OracleEnvs(E, N, seed=H.WIDE_SEED, env_offset=off, auto_reset=True, config=_oracle_config_from(O, cfg))
    bnd = H.f32_bounds(ref.cfg, _default_oracle_config())
    worst = dict(pos=0.0, psi=0.0)

    def close_to_oracle(env, sel):
        e = max(np.abs(env.trf_x[sel] - ref.trf_x[sel]).max(), np.abs(env.trf_y[sel] - ref.trf_y[sel]).max())
        worst["pos"] = max(worst["pos"], float(e))
        assert e < bnd["reset_pos"], e
        for k in ("trf_psi", "own_psi"):
            dpsi = np.abs(getattr(env, k)[sel] - getattr(ref, k)[sel])
            worst["psi"] = max(worst["psi"], float(np.minimum(dpsi, 360 - dpsi).max()))
            assert np.minimum(dpsi, 360 - dpsi).max() < bnd["reset_psi"], k
        assert np.array_equal(env.trf_v[sel], ref.trf_v[sel])

    kw = dict(device="cuda:0", dtype=torch.float32, auto_reset=True, seed=H.WIDE_SEED, env_offset=off, config=cfg)
    ref.reset()
    env = _engine(g.ACAS2DVecEnv(E, **kw))
    env.reset()
    close_to_oracle(env, np.ones(E, bool))
    ref.episode[:] = _wide_episode0(E)
    env.v.episode.copy_(torch.as_tensor(ref.episode.view(np.int32), device="cuda:0"))
    rng = np.random.default_rng(3)
    checked = wrapped = 0
    twin = g.ACAS2DVecEnv(E, **kw)
    for _ in range(T):
        a = rng.uniform(-1, 1, E).astype(np.float32).astype(np.float64)
        _, _, d1, _, _ = ref.step(a)
        _, _, d2, _, _ = env.step(a)
        both = (d1 != 0) & (d2 != 0) & (env.episode == ref.episode)
        if both.any():
            checked += int(both.sum())
            wrapped += int((both & (ref.episode == 0)).sum())
            close_to_oracle(env, both)
        fresh = torch.as_tensor(d2 != 0, device="cuda:0")
        if fresh.any():
            twin.episode.copy_(env.v.episode)
            twin._launch_reset(fresh.to(torch.uint8), do_init=1)
            for k in _STATE:
                assert torch.equal(getattr(twin, k)[fresh], getattr(env.v, k)[fresh]), k
            assert bits_equal(twin.outputs["obs"][fresh], env.v.outputs["obs"][fresh])
    print("f32 reset draws at wide keys: %d in-step resets checked (%d wrapped the counter); worst positions %.2e (bound "
          "%.2e), headings %.2e (bound %.0e)" % (checked, wrapped, worst["pos"], bnd["reset_pos"], worst["psi"],
                                                 bnd["reset_psi"]))
    assert checked > 500 and wrapped > 50


@pytest.mark.parametrize("shape", _PACKED, ids=_ids(_PACKED))
def test_every_packed_shape_rollout_equals_steps_at_wide_keys(g, monkeypatch, shape):
    """test_every_packed_shape_rollout_equals_steps at the wide keys ("mid" crossing, the even envs' counters at
    2^32 - 2: their second reset inside the 90 steps wraps them)."""
    _rollout_equals_steps(g, monkeypatch, shape, _SHORT, seed=H.WIDE_SEED, env_offset=H.WIDE_OFFSET["mid"],
                          episode0=_wide_episode0(H.WIDE_E))


# ---- 32-bit offset limits at scale ------------------------------------------------------------------------------------
# The float32 arena kernel addresses its state through 32-bit byte offsets and is admitted up to helpers.ARENA_BOUND;
# observation rows [E][D] and rollout outputs [T][E][D] pass 2^32 bytes and 2^31 elements at ordinary sizes.  These run
# there.  Device memory is checked first: a card without room skips, naming the bytes needed.
def _env_bytes(E, N, elem, term_obs=True, generations=1):
    """Device bytes of one ACAS2DVecEnv: state (`generations` of the per-step arrays), status, actions, step outputs."""
    D = 5 + 3 * N
    per_step = elem * (4 + 2 * N) + 4                     # own_x, own_y, own_psi, total_reward, trf_x, trf_y; steps
    return E * (generations * per_step + elem * (4 + 2 * N + 3 + D * (2 if term_obs else 1)) + 4 * 2 + 1 + 2)


def _need_device_bytes(n):
    torch.cuda.empty_cache()                              # (blocks an earlier test left in torch's cache count as free)
    free, _ = torch.cuda.mem_get_info()
    if free < n * 1.05:
        pytest.skip("needs %d bytes of free device memory, %d free" % (n * 1.05, free))
    torch.cuda.reset_peak_memory_stats()


def _print_peak(what):
    print("%s: peak device memory %.1f GB" % (what, torch.cuda.max_memory_allocated() / 1e9))


def _window_state(v, lo, hi):
    """The envs [lo, hi) of a float32 env as float64 numpy: what _check_f32_step_vs_oracle reads of its engine."""
    f = lambda t: t[lo:hi].double().cpu().numpy() if t.is_floating_point() else t[lo:hi].cpu().numpy()  # noqa: E731
    ns = types.SimpleNamespace(**{n: f(getattr(v, n)) for n in _STATE + ("steps", "total_reward")})
    ns.episode = v.episode[lo:hi].cpu().numpy().view(np.uint32)
    ns.term_obs = f(v.outputs["terminal_observation"])
    ns.ep_return, ns.ep_steps = f(v.outputs["episode_return"]), f(v.outputs["episode_steps"])
    return ns


def _f32_window_step_vs_oracle(O, v, before, lo, act, tot, t):
    """The float32 step just taken, over envs [lo, lo + len) of `v`, against the oracle stepped from `before` (their
    state before it) with env_offset = lo: _check_f32_step_vs_oracle."""
    n = len(before.steps)
    chk = O.OracleEnvs(n, v.n_traffic, seed=v.seed_value, env_offset=v.env_offset + lo, auto_reset=True,
                       config=_oracle_config_from(O, v.config))
    chk.set_state(np.stack([before.own_x, before.own_y, before.own_psi, before.own_v], 1),
                  np.stack([before.trf_x, before.trf_y, before.trf_psi, before.trf_v], -1),
                  np.stack([before.goal_x, before.goal_y], 1), before.steps)
    chk.total_reward[:] = before.total_reward
    chk.episode[:] = before.episode
    o, r, d, oc, _ = chk.step(act)
    after = _window_state(v, lo, lo + n)
    got = tuple(v.outputs[k][lo:lo + n].cpu().numpy() for k in ("obs", "reward", "done", "outcome"))
    got = (got[0].astype(np.float64), got[1].astype(np.float64), got[2].astype(np.uint8), got[3])
    _check_f32_step_vs_oracle(after, chk, (o, r, d, oc), got, v.n_traffic, tot, t)


_ARENA_SCALE = [(N, e_yes, True) for N, e_yes, _ in H.ARENA_BOUND if N != 2] + [(H.ARENA_BOUND[0][0], H.ARENA_BOUND[0][2], False)]


@pytest.mark.parametrize("N,E,admitted", _ARENA_SCALE, ids=["N%d-E%d" % (n, e) for n, e, _ in _ARENA_SCALE])
def test_arena_kernel_at_its_32_bit_size_bound(g, O, monkeypatch, N, E, admitted):
    """float32 at the arena kernel's largest admitted size (and, N = 8, the first rejected one, which takes the general
    kernel): 24 steps from reset() with episodes of 20 steps.  Against the general kernel (ACAS2D_NO_ARENA), every
    element of the state and the outputs bit for bit after every step: envs are independent and their episodes depend on
    (seed, global index, counter) only, so a twin of E / 4 envs at env_offset = lo steps envs [lo, lo + E / 4) exactly as
    the full launch does; the full env is re-run from reset() once per quarter, which keeps the two envs within ~36 GB.
    Against the float64 oracle (_check_f32_step_vs_oracle), in the first pass, over windows of 4 096 envs -- the first,
    those around the observation row that straddles byte 2^32, the last -- in every step."""
    monkeypatch.delenv("ACAS2D_SHAPE", raising=False)
    monkeypatch.delenv("ACAS2D_NO_ARENA", raising=False)
    Q = E // 4
    assert Q * 4 == E
    _need_device_bytes(_env_bytes(E, N, 4) + _env_bytes(Q, N, 4) + 4 * E)
    cfg = g.ACAS2DConfig(n_traffic=N, max_steps=20)
    a = g.ACAS2DVecEnv(E, device="cuda:0", dtype=torch.float32, seed=13, config=cfg, double_buffer=False)
    assert a.consecutive_layout == admitted
    D, W, T = a.obs_dim, 4096, 24
    cross = H.obs_row_crossing(D, 4)
    assert cross + W // 2 < E and E * D * 4 > 2 ** 32
    windows = (0, cross - W // 2, E - W)
    tot = _new_f32_totals()
    dones = 0
    for lo in range(0, E, Q):
        sl = slice(lo, lo + Q)
        b = g.ACAS2DVecEnv(Q, device="cuda:0", dtype=torch.float32, seed=13, env_offset=lo, config=cfg,
                           double_buffer=False)
        assert bits_equal(a.reset()[sl], b.reset())
        for k in ("terminal_observation", "episode_return", "episode_steps"):   # written where done only: start as b's
            a.outputs[k].zero_()
        gen = torch.Generator(device="cuda:0").manual_seed(12)
        for t in range(T):
            act = torch.rand(E, generator=gen, device="cuda:0") * 2 - 1
            before = [_window_state(a, w, w + W) for w in windows] if lo == 0 else None
            a.step(act)
            monkeypatch.setenv("ACAS2D_NO_ARENA", "1")
            assert not b.consecutive_layout
            b.step(act[sl])
            monkeypatch.delenv("ACAS2D_NO_ARENA")
            for k in ("obs", "reward", "done", "outcome", "terminal_observation", "episode_return", "episode_steps"):
                assert bits_equal(a.outputs[k][sl], b.outputs[k]), (lo, t, k)
            for name in _STATE + ("steps", "total_reward", "episode", "status"):
                assert bits_equal(getattr(a, name)[sl], getattr(b, name)), (lo, t, name)
            dones += int(b.outputs["done"].sum())
            if lo == 0:
                for w, bf in zip(windows, before):
                    _f32_window_step_vs_oracle(O, a, bf, w, act[w:w + W].double().cpu().numpy(), tot, t)
        del b
    _print_f32_totals("at %d x %d (%s kernel), 3 windows of %d envs over %d steps" %
                      (E, N, "arena" if admitted else "general", W, T), tot)
    _print_peak("arena bound %d x %d" % (E, N))
    assert dones > E and tot["finished"] > 2 * W


def test_f64_obs_past_4_gib_vs_oracle(g, O, monkeypatch):
    """float64, 20 000 000 envs x 8 (observations [E][29] of 4.6 GB), 45 auto-reset steps of episodes of 20 steps from
    reset(): the oracle over the 4 096 envs around the observation row that straddles byte 2^32 (env 18 512 790) and the
    last 4 096 (the last wave), env_offset = the window's start -- drawn states bit for bit, observations and rewards
    1e-9, masks and counters equal."""
    monkeypatch.delenv("ACAS2D_SHAPE", raising=False)
    E, N, T, W = 20_000_000, 8, 45, 4096
    _need_device_bytes(_env_bytes(E, N, 8) + 8 * E)
    cfg = g.ACAS2DConfig(n_traffic=N, max_steps=20)
    v = g.ACAS2DVecEnv(E, device="cuda:0", dtype=torch.float64, seed=13, config=cfg, double_buffer=False)
    cross = H.obs_row_crossing(v.obs_dim, 8)
    assert cross == 18512790 and E * v.obs_dim * 8 > 2 ** 32
    windows = (cross - W // 2, E - W)
    refs = [O.OracleEnvs(W, N, seed=13, env_offset=lo, auto_reset=True, config=_oracle_config_from(O, cfg))
            for lo in windows]
    obs = v.reset()
    for lo, ref in zip(windows, refs):
        o = ref.reset()
        np.testing.assert_allclose(obs[lo:lo + W].cpu().numpy(), o, rtol=0, atol=1e-9)
    gen = torch.Generator(device="cuda:0").manual_seed(13)
    dones = 0
    for t in range(T):
        act = torch.rand(E, generator=gen, device="cuda:0", dtype=torch.float64) * 2 - 1
        obs, rew, done, _ = v.step(act)
        for lo, ref in zip(windows, refs):
            sl = slice(lo, lo + W)
            o, r, d, oc, _ = ref.step(act[sl].cpu().numpy())
            assert np.array_equal(done[sl].cpu().numpy(), d != 0) and np.array_equal(v.outputs["outcome"][sl].cpu().numpy(), oc), t
            np.testing.assert_allclose(obs[sl].cpu().numpy(), o, rtol=0, atol=1e-9, equal_nan=True)
            np.testing.assert_allclose(rew[sl].cpu().numpy(), r, rtol=0, atol=1e-9, equal_nan=True)
            assert np.array_equal(v.steps[sl].cpu().numpy(), ref.steps) and np.array_equal(v.episode[sl].cpu().numpy().view(np.uint32), ref.episode)
            fin = d != 0
            dones += int(fin.sum())
            for name in _STATE:                                     # the fresh episodes: bit for bit
                assert np.array_equal(getattr(v, name)[sl].cpu().numpy()[fin], getattr(ref, name)[fin]), (t, name)
            for name in ("own_x", "own_y", "own_psi", "trf_x", "trf_y"):
                np.testing.assert_allclose(getattr(v, name)[sl].cpu().numpy(), getattr(ref, name), rtol=0, atol=1e-9)
    _print_peak("float64 obs past 4 GiB")
    assert dones > 2 * W


@pytest.mark.parametrize("dtype_name", ("float32", "float64"))
def test_rollout_outputs_past_2_to_the_31_elements_equal_steps(g, monkeypatch, dtype_name):
    """rollout() of 65 536 envs x 8 over 1 200 steps: its [T][E][29] observations pass 2^32 bytes (float32: step 565)
    and 2^31 elements (step 1 130); float32 also keeps the terminal observations.  Against a twin stepped 1 200 times,
    bit for bit at every step -- compared on the device, no second [T][E][D] copy -- and in the final state."""
    monkeypatch.delenv("ACAS2D_SHAPE", raising=False)
    dtype = getattr(torch, dtype_name)
    E, N, T = 65536, 8, 1200
    elem = 4 if dtype == torch.float32 else 8
    keep = dtype == torch.float32
    D = 5 + 3 * N
    _need_device_bytes(T * E * (D * elem * (2 if keep else 1) + elem * 3 + 6) + 2 * _env_bytes(E, N, elem, generations=2))
    assert T * E * D >= 2 ** 31 and (2 ** 31) // (E * D) < T
    a, b = (g.ACAS2DVecEnv(E, N, device="cuda:0", dtype=dtype, seed=13) for _ in range(2))
    assert bits_equal(a.reset(), b.reset())
    gen = torch.Generator(device="cuda:0").manual_seed(14)
    actions = torch.rand(T, E, generator=gen, device="cuda:0", dtype=dtype) * 2 - 1
    out = a.rollout(actions, keep_terminal_obs=keep)
    dones = late = 0
    for t in range(T):
        obs, rew, done, infos = b.step(actions[t])
        assert bits_equal(out["obs"][t], obs) and bits_equal(out["reward"][t], rew), t
        assert torch.equal(out["done"][t], done) and torch.equal(out["outcome"][t], infos.outcome), t
        assert bits_equal(out["episode_return"][t][done], infos.episode_return[done]), t
        assert bits_equal(out["episode_steps"][t][done], infos.episode_steps[done]), t
        if keep:
            assert bits_equal(out["terminal_observation"][t][done], infos.terminal_observation[done]), t
        n = int(done.sum())
        dones += n
        late += n if t * E * D >= 2 ** 31 else 0
    _print_peak("rollout %s past 2^31 elements" % dtype_name)
    assert late > 0 and dones > E
    _same_state(a, b)


def test_collector_outputs_past_2_to_the_31_elements_replay_on_a_twin(g, monkeypatch):
    """collect() of 65 536 envs x 8 float32 over 1 200 steps ([T + 1][E][29] observations past 2^31 elements): a twin
    stepped with its clipped actions reproduces every observation, reward and mask (helpers.replay_collect_on_twin)."""
    monkeypatch.delenv("ACAS2D_SHAPE", raising=False)
    E, N, T = 65536, 8, 1200
    D = 5 + 3 * N
    _need_device_bytes((T + 1) * E * D * 4 + T * E * 24 + 2 * _env_bytes(E, N, 4, generations=2))
    torch.manual_seed(1)
    pol = g.ActorCritic(D).to("cuda:0")
    with torch.no_grad():
        pol.action_net.weight.mul_(40.0)
    env, twin = (g.ACAS2DVecEnv(E, N, device="cuda:0", seed=13) for _ in range(2))
    env.reset()
    twin.reset()
    out = env.collect(pol, T, noise_seed=5, noise_step=0)
    assert out["obs"].numel() >= 2 ** 31
    assert H.replay_collect_on_twin(env, twin, out) > E
    _print_peak("collector past 2^31 elements")


# ---- hand-placed edge states on every work shape (tests/edge_states.py; tests/test_edge_states.py holds the batch to its
# labels on the CPU oracle) ------------------------------------------------------------------------------------------------
def _edge_config(O, name):
    """(ACAS2DConfig keywords, OracleConfig) of the configuration `name`: "default" or one of helpers.NONDEFAULT_CONFIGS."""
    import gym_acas2d_amd as g
    kw = {} if name == "default" else H.NONDEFAULT_CONFIGS[name]
    return kw, H.oracle_config(O, g.ACAS2DConfig(n_traffic=1, **kw))


_EDGE_BATCHES = {}


def _edge_batch(O, N, name):
    import edge_states as ES
    if (N, name) not in _EDGE_BATCHES:
        _EDGE_BATCHES[(N, name)] = ES.edge_batch(N, _edge_config(O, name)[1], seed=N)
    return _EDGE_BATCHES[(N, name)]


def _f32r(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


class _RolloutView:
    """Step t of a rollout() dict behind the engine attributes the checkers read (the state is the env's own)."""

    def __init__(self, env, out, t=0):
        self.env, self.out, self.t = env, out, t

    def __getattr__(self, name):
        key = {"term_obs": "terminal_observation", "ep_return": "episode_return", "ep_steps": "episode_steps"}.get(name)
        if key is None:
            return getattr(self.env, name)
        return GpuEngine._np(self.out[key][self.t])


def _rollout_outputs(out, t=0):
    d = out["done"][t].cpu().numpy().astype(np.uint8)
    return (GpuEngine._np(out["obs"][t]), GpuEngine._np(out["reward"][t]), d, out["outcome"][t].cpu().numpy())


def _check_f64_edge_step(b, env, ref, got, stepped, auto_reset, tot):
    """One float64 step of the edge batch against the oracle stepped from the same state: obs, reward, positions and
    headings to 1e-9, NaN exactly where the oracle has it (obs, reward, terminal observation, return), masks and outcome
    bit-exact outside the 1e-9 band -- in which exactly the placed envs lie --, the fresh episode of every finished env bit
    for bit.  At the mirror-heading slots only, the sign of d_cpa is exempt (its magnitude is not): v12x is an exact 0 or
    +-1 ulp there, a coin toss of the host's cos that the device's sincos -- in either formulation -- need not repeat
    (test_f64_edge_vectors)."""
    import edge_states as ES
    obs, rew, done, outcome = got
    o, r, d, oc = stepped
    band = ES.placed_in_band(b, ES.F64_BAND)
    assert not (((done != d) | (outcome != oc)) & ~band).any()
    same = (done == d) & (outcome == oc)
    tot["band"] += int(band.sum()); tot["band_differs"] += int((~same).sum())
    want = o.copy()
    ms = ES.labels(b, "mirror_slot").astype(int)
    coin = np.nonzero(ms >= 0)[0]
    col = 5 + 3 * ms[coin] + 1
    flip = (d[coin] == 0) & (np.sign(obs[coin, col]) != np.sign(want[coin, col]))
    want[coin[flip], col[flip]] *= -1.0
    tot["sign_flips"] = tot.get("sign_flips", 0) + int(flip.sum())
    assert np.array_equal(np.isnan(obs[same]), np.isnan(o[same])) and np.array_equal(np.isnan(rew), np.isnan(r))
    tot["nan"] += int(np.isnan(o[same]).sum())
    np.testing.assert_allclose(obs[same], want[same], rtol=0, atol=1e-9, equal_nan=True)
    np.testing.assert_allclose(rew[same], r[same], rtol=0, atol=1e-9, equal_nan=True)
    go = same & ((d == 0) | (not auto_reset))
    for name in ("own_x", "own_y", "own_psi", "trf_x", "trf_y", "trf_psi"):
        np.testing.assert_allclose(getattr(env, name)[go], getattr(ref, name)[go], rtol=0, atol=1e-9, err_msg=name)
    assert np.array_equal(env.steps[same], ref.steps[same]) and np.array_equal(env.episode[same], ref.episode[same])
    if not auto_reset:
        assert np.array_equal(env.status[same], ref.status[same])
        return
    fin = same & (d != 0)
    tot["finished"] += int(fin.sum())
    if fin.any():
        assert np.array_equal(np.isnan(env.term_obs[fin]), np.isnan(ref.term_obs[fin]))
        assert np.array_equal(np.isnan(env.ep_return[fin]), np.isnan(ref.ep_return[fin]))
        tot["nan"] += int(np.isnan(ref.term_obs[fin]).sum())
        np.testing.assert_allclose(env.term_obs[fin], ref.term_obs[fin], rtol=0, atol=1e-9, equal_nan=True)
        np.testing.assert_allclose(env.ep_return[fin], ref.ep_return[fin], rtol=0, atol=1e-9, equal_nan=True)
        assert np.array_equal(env.ep_steps[fin], ref.ep_steps[fin])
        for name in _STATE:
            assert np.array_equal(getattr(env, name)[fin], getattr(ref, name)[fin]), name


def _check_f32_edge_step(b, env, chk, got, stepped, tot, t=0):
    """_check_f32_step_vs_oracle with the float32 band (1e-3) holding exactly the placed envs, and on top: the NaN pattern
    of every slot exact (obs, reward; terminal observation and return where finished), every traffic heading the oracle's
    wrapped heading rounded to float32 (a hair below 0 wraps to 360 - 2^-40 in float64: 360.0f, what the float32 wrap
    gives), the player's within one float32 ulp of 360."""
    import edge_states as ES
    obs, rew, done, outcome = got
    o, r, d, oc = stepped
    go, fin = _check_f32_step_vs_oracle(env, chk, stepped, got, b.N, tot, t, in_band=ES.placed_in_band(b, ES.F32_BAND))
    same = go | fin
    assert np.array_equal(np.isnan(obs[same]), np.isnan(o[same])) and np.array_equal(np.isnan(rew[same]), np.isnan(r[same]))
    tot["nan"] = tot.get("nan", 0) + int(np.isnan(o[same]).sum())
    if chk.auto_reset and fin.any():
        assert np.array_equal(np.isnan(env.term_obs[fin]), np.isnan(chk.term_obs[fin]))
        assert np.array_equal(np.isnan(env.ep_return[fin]), np.isnan(chk.ep_return[fin]))
        tot["nan"] += int(np.isnan(chk.term_obs[fin]).sum())
    assert np.array_equal(env.trf_psi[go], _f32r(chk.trf_psi[go]))
    dpsi = np.abs(env.own_psi[go] - chk.own_psi[go])
    assert np.minimum(dpsi, 360 - dpsi).max() <= 3.1e-5


def _edge_rollout_equals_steps(g, shape, b, kw, state, T=3):
    """rollout(T) from the injected edge state == T step() calls bit for bit, the written-back headings included."""
    a = _shape_env(g, shape, len(b.case), config=kw, double_buffer=False)
    c = _shape_env(g, shape, len(b.case), config=kw, double_buffer=False)
    for v in (a, c):
        v.set_state(*state[:4], observe=False)
    gen = torch.Generator(device="cuda:0").manual_seed(6)
    actions = torch.rand(T, len(b.case), generator=gen, device="cuda:0", dtype=a.dtype) * 2 - 1
    actions[0] = torch.as_tensor(state[4], device="cuda:0", dtype=a.dtype)
    out = a.rollout(actions, keep_terminal_obs=True)
    for t in range(T):
        obs, rew, done, infos = c.step(actions[t])
        assert bits_equal(out["obs"][t], obs) and bits_equal(out["reward"][t], rew), t
        assert torch.equal(out["done"][t], done) and torch.equal(out["outcome"][t], infos.outcome), t
        for k, want in (("episode_return", infos.episode_return), ("episode_steps", infos.episode_steps),
                        ("terminal_observation", infos.terminal_observation)):
            assert bits_equal(out[k][t][done], want[done]), (t, k)
    _same_state(a, c)


_EDGE_CASES = [(s, "default") for s in H.SHAPES] + [(s, "small") for s in H.SHAPES if s.override is None]


@pytest.mark.parametrize("shape,config", _EDGE_CASES, ids=["%s-%s" % (s.id, c) for s, c in _EDGE_CASES])
def test_every_shape_on_edge_states_vs_oracle(g, O, monkeypatch, shape, config):
    """The edge batch of tests/edge_states.py -- a collision at every slot at +-1e-8 / 1e-2 / 5 px of the threshold (and
    0, +-1e-10: in the band), parallel flight (NaN d_cpa) and mirror headings at every slot, injected headings at every
    slot, goal thresholds, timeout precedence, heading wraps, off-plan states and odd speeds, each case at the first and
    the last env of a wave and in a partial last wave -- through every path of the work shape against the oracle: the
    latching step, the auto-reset step in place and double-buffered, float32 packed shapes in the consecutive-layout
    kernel and in the general one, and the fused rollout (T = 1 against the oracle, T = 3 bit for bit against steps)."""
    import edge_states as ES
    _use_shape(g, monkeypatch, shape)
    N = shape.n_traffic
    kw, ocfg = _edge_config(O, config)
    b = _edge_batch(O, N, config)
    E = len(b.case)
    f32 = shape.dtype == "float32"
    rnd = _f32r if f32 else (lambda a: np.asarray(a, np.float64))
    state = (rnd(b.own), rnd(b.trf), rnd(b.goal), b.steps)
    act = rnd(b.action)
    tot = dict(band=0, band_differs=0, nan=0, finished=0) if not f32 else _new_f32_totals()
    paths = []

    def oracle(auto_reset, n=E):
        ref = O.OracleEnvs(n, N, seed=21, env_offset=37, auto_reset=auto_reset, config=ocfg)
        ref.set_state(state[0][:n], state[1][:n], state[2][:n], state[3][:n])
        return ref, ref.step(act[:n])[:4]

    def check(env, ref, got, stepped, auto_reset, n=E):
        sub = b._replace(own=b.own[:n], case=b.case[:n]) if n != E else b
        if f32:
            _check_f32_edge_step(sub, env, ref, got, stepped, tot)
        else:
            _check_f64_edge_step(sub, env, ref, got, stepped, auto_reset, tot)

    for auto_reset, db in ((False, False), (True, False), (True, True)):
        ref, stepped = oracle(auto_reset)
        v = _shape_env(g, shape, E, auto_reset=auto_reset, config=kw, double_buffer=db)
        assert not v.consecutive_layout                   # E is not whole workgroups: the general kernel
        env = _engine(v)
        env.set_state(*state)
        check(env, ref, env.step(act)[:4], stepped, auto_reset)
        paths.append("latching" if not auto_reset else "double-buffered" if db else "in place")
    if f32 and shape.packed:                               # whole eight-workgroup groups: arena kernel and general kernel
        n = b.whole
        ref, stepped = oracle(True, n)
        for arena in (True, False):
            v = _shape_env(g, shape, n, config=kw)
            if arena:
                monkeypatch.delenv("ACAS2D_NO_ARENA", raising=False)
            else:
                monkeypatch.setenv("ACAS2D_NO_ARENA", "1")
            assert v.consecutive_layout == arena
            env = _engine(v)
            env.set_state(state[0][:n], state[1][:n], state[2][:n], state[3][:n])
            check(env, ref, env.step(act[:n])[:4], stepped, True, n)
            paths.append("arena" if arena else "general, whole groups")
        monkeypatch.delenv("ACAS2D_NO_ARENA", raising=False)
    if shape.packed:
        ref, stepped = oracle(True)
        v = _shape_env(g, shape, E, config=kw, double_buffer=False)
        env = _engine(v)
        env.set_state(*state)
        out = v.rollout(torch.as_tensor(act, device="cuda:0", dtype=v.dtype)[None], keep_terminal_obs=True)
        check(_RolloutView(env, out), ref, _rollout_outputs(out), stepped, True)
        _edge_rollout_equals_steps(g, shape, b, kw, state + (act,))
        paths.append("rollout")
    placed = ES.placed_in_band(b, ES.F32_BAND if f32 else ES.F64_BAND)
    print("edge states on %s (%s): %d envs, %d cases, paths %s; in-band rows %d per path (placed %d); NaN entries matched %d; "
          "mirror d_cpa signs exempted %d" % (shape.id, config, E, len(b.cases), ", ".join(paths),
                                              (tot["in_band"] if f32 else tot["band"]) // len(paths), int(placed.sum()),
                                              tot["nan"], tot.get("sign_flips", 0)))
    if f32:
        _print_f32_totals("edge states on %s (%s)" % (shape.id, config), tot)
    assert tot["nan"] > 0 and tot["finished"] > 0


def _edge_shape_groups():
    """(dtype_name, N, ACAS2D_SHAPE values) of every (dtype, formulation, N) with more than one work shape, plus the
    generic overrides of test_results_do_not_depend_on_the_work_shape (N = 8 and 64)."""
    extra = {("float32", 8): ("generic,4",), ("float32", 64): ("generic,16", "generic,64"),
             ("float64", 8): ("generic,4",), ("float64fast", 8): ("generic,4",)}
    groups = {}
    for s in H.SHAPES:
        groups.setdefault((s.dtype_name, s.n_traffic), []).append(s.override)
    return [(k[0], k[1], tuple(v) + extra.get(k, ())) for k, v in groups.items() if len(v) + len(extra.get(k, ())) > 1]


@pytest.mark.parametrize("dtype_name,N,shapes", _edge_shape_groups(), ids=["%s-N%d" % k[:2] for k in _edge_shape_groups()])
def test_edge_states_do_not_depend_on_the_work_shape(g, O, monkeypatch, dtype_name, N, shapes):
    """test_results_do_not_depend_on_the_work_shape on the edge batch: the latching and the auto-reset step of every work
    shape of (dtype, formulation, N) leave the same outputs and state, bit for bit."""
    dtype, cfg = _dtype_and_config(g, dtype_name, N)
    b = _edge_batch(O, N, "default")
    E = len(b.case)
    f = _f32r if dtype == torch.float32 else (lambda a: np.asarray(a, np.float64))
    ref = None
    for sh in shapes:
        if sh is None:
            monkeypatch.delenv("ACAS2D_SHAPE", raising=False)
        else:
            monkeypatch.setenv("ACAS2D_SHAPE", sh)
        got = []
        for auto_reset in (False, True):
            v = g.ACAS2DVecEnv(E, N, device="cuda:0", dtype=dtype, seed=21, env_offset=37, auto_reset=auto_reset, config=cfg)
            v.set_state(f(b.own), f(b.trf), f(b.goal), b.steps, observe=False)
            obs, rew, done, infos = v.step(torch.as_tensor(f(b.action), device="cuda:0", dtype=dtype))
            got += [obs.clone(), rew.clone(), done.clone(), infos.outcome.clone()]
            if auto_reset:
                got += [v.outputs[k].clone() for k in ("terminal_observation", "episode_return", "episode_steps")]
            got += [getattr(v, n).clone() for n in _STATE + ("steps", "total_reward", "episode", "status")]
        if ref is None:
            ref = got
        else:
            for k, (x, y) in enumerate(zip(ref, got)):
                assert bits_equal(x, y), (sh, k)
