"""The in-kernel policy, collector and evaluator at 8 to 64 traffic aircraft: acas2d_rollout_policy_group_f32,
acas2d_collect_group_f32, acas2d_evaluate_policies_group_f32 (`group=True` in the Python layers), where the G lanes that
share an env evaluate the SB3 MlpPolicy networks together.

CPU: the three symbols, their argument validation, the float32-only rule.  GPU (-m gpu):
  * N = 8, the one traffic count with both kernels: group=True (shape (4,2)) equals the thread-per-env launch (shape
    (8,1)) BIT FOR BIT in everything a launch writes -- the group kernel keeps the per-unit fma sequence and the head's
    summation order;
  * N = 16, 32, 64 (no thread-per-env kernel): actions, values, log-probabilities and noise against the float64
    references of learner_ref, NaN observations, a twin env replaying the launch bit for bit, in-kernel resets;
  * the K-policy evaluation at N = 64 against single-policy evaluations and the rollout they are read off;
  * PPOTrainer with the fused collector, evaluations and best-model keeping at N = 16.

Bounds are the project's own for these quantities (tests/test_learner_kernels.py): action and value 5e-6, eps and logp
1e-5, relative to max(1, |reference|); the deterministic action 1e-5 absolute.  Every criterion prints what it observed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import helpers as H
import learner_ref as R
import learner_support as LS

torch = pytest.importorskip("torch")
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP_N = (8, 16, 32, 64)                       # work shapes (4,2) (4,4) (4,8) (4,16)
SYMBOLS = ("acas2d_rollout_policy_group_f32", "acas2d_collect_group_f32", "acas2d_evaluate_policies_group_f32")


@pytest.fixture(scope="module")
def g():
    import gym_acas2d_amd as g
    return g


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_group_symbols_are_declared_exported_and_bound(g):
    header = open(os.path.join(ROOT, "include", "acas2d.h")).read()
    L = g.native.lib()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in g.native.EXPORTS
        fn = getattr(L, name)
        sibling = getattr(L, name.replace("_group", ""))
        assert fn.restype is C.c_int and fn.argtypes == sibling.argtypes, name
    assert L.acas2d_abi_version() == 7 == g.native.ABI_VERSION
    assert re.search(r"#define\s+ACAS2D_ABI_VERSION\s+7\b", header)


def test_group_entry_points_validate_without_a_gpu(g, monkeypatch):
    """Rejected with ACAS2D_EINVAL and a message, before any launch (the pointers are host addresses): a traffic count
    without a packed shape (5), one that belongs to the thread-per-env siblings (3), hidden != 64, a missing value net,
    and for the evaluation a state smaller than K x round_up(E, 64)."""
    L = g.native.lib()
    buf = (C.c_double * 8192)()
    a = (C.addressof(buf) + 15) & ~15
    st = g.native.CState(*([a] * 14))
    io = g.native.CStepIO(*([a] * 5 + [None] * 3))

    def pol(hidden=64):
        return g.native.CPolicy(*([a] * 6), hidden, 0)

    def ac(hidden=64, **none):
        f = {n: a for n, _ in g.native.CActorCritic._fields_[1:10]}
        f.update(none)
        return g.native.CActorCritic(pol(hidden), **f, noise_seed=7, noise_step=0)

    rp, cl, ev = (getattr(L, n) for n in SYMBOLS)

    def calls(N, hidden=64):
        cfg = g.ACAS2DConfig(n_traffic=N).to_c()
        yield "acas2d_rollout_policy_f32", rp(C.byref(cfg), C.byref(st), C.byref(io), C.byref(pol(hidden)), a, 4, 13, 0, 64, N, None)
        yield "acas2d_collect_f32", cl(C.byref(cfg), C.byref(st), C.byref(io), C.byref(ac(hidden)), a, 4, 13, 0, 64, N, None)
        yield "acas2d_evaluate_policies_f32", ev(C.byref(cfg), C.byref(st), 256, C.byref(pol(hidden)), 2, 100, a, 10, 13, 0, N,
                                                 a, a, a, None)

    monkeypatch.delenv("ACAS2D_SHAPE", raising=False)
    for N, words, override in ((5, ("no packed work shape",), None), (3, ("thread-per-env", "use %s"), None),
                               (6, ("no packed work shape",), None), (128, ("no packed work shape",), None),
                               (64, ("C=8 G=8",), "8,8"), (64, ("no packed work shape",), "generic,16")):
        if override:
            monkeypatch.setenv("ACAS2D_SHAPE", override)          # (read at every call)
        else:
            monkeypatch.delenv("ACAS2D_SHAPE", raising=False)
        for sibling, rc in calls(N):
            err = L.acas2d_last_error().decode()
            assert rc == -22, (N, sibling, rc, err)
            assert "n_traffic = %d" % N in err and "n_traffic in {8, 16, 32, 64}" in err, err
            for w in words:
                assert (w % sibling if "%s" in w else w) in err, (N, sibling, err)
    monkeypatch.delenv("ACAS2D_SHAPE", raising=False)
    for N in GROUP_N:
        for hidden in (32, 0, 65):
            for _, rc in calls(N, hidden):
                assert rc == -22 and (b"got hidden = %d" % hidden) in L.acas2d_last_error(), (N, hidden)
        cfg = g.ACAS2DConfig(n_traffic=N).to_c()
        for name in ("v1t", "vb1", "v2t", "vb2", "v3", "vb3", "log_std", "values", "logp"):
            assert cl(C.byref(cfg), C.byref(st), C.byref(io), C.byref(ac(**{name: None})), a, 4, 13, 0, 64, N, None) == -22, name
            assert b"the value net, log_std, values and logp are required" in L.acas2d_last_error(), name
        assert cl(C.byref(cfg), C.byref(st), C.byref(io), None, a, 4, 13, 0, 64, N, None) == -22
        assert b"NULL actor-critic" in L.acas2d_last_error()
        # K x round_up(E, 64) envs: 2 x 128 = 256 fit, 255 do not; 3 x 64 = 192 at E = 37
        for n_envs, K, E, need in ((255, 2, 100, 256), (191, 3, 37, 192), (0, 1, 1, 64)):
            assert ev(C.byref(cfg), C.byref(st), n_envs, C.byref(pol()), K, E, a, 10, 13, 0, N, a, a, a, None) == -22
            assert (b"need %d" % need) in L.acas2d_last_error(), (N, L.acas2d_last_error())
        # a lane reads its slice of a weight row as 16-byte vectors
        odd = g.native.CPolicy(a + 4, a, a, a, a, a, 64, 0)
        assert rp(C.byref(cfg), C.byref(st), C.byref(io), C.byref(odd), a, 4, 13, 0, 64, N, None) == -22
        assert b"16-byte aligned" in L.acas2d_last_error()


def test_group_launches_are_float32_only(g):
    """group=True on a float64 env raises ValueError before the library is touched."""
    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError("the library was asked for " + name)

    env = object.__new__(g.ACAS2DVecEnv)
    env.auto_reset, env.dtype, env._lib = True, torch.float64, Untouchable()
    with pytest.raises(ValueError, match="float32 only"):
        env.rollout_policy(None, 4, group=True)
    with pytest.raises(ValueError, match="float32 only"):
        env.collect(None, 4, group=True)
    z = np.zeros((4, 4))
    with pytest.raises(ValueError, match="float32 only"):
        g.evaluate_policies_fused([object()], z, np.zeros((4, 16, 4)), group=True)
    with pytest.raises(ValueError, match="float32 only"):
        g.evaluate_policy_fused(object(), z, np.zeros((4, 16, 4)), dtype=torch.float64, group=True)


# ---- GPU ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu(g):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    g.native.lib()
    return g


def _config(g, N, name="default", **kw):
    return g.ACAS2DConfig(n_traffic=N, **dict(H.NONDEFAULT_CONFIGS[name] if name != "default" else {}, **kw))


def _envs(g, N, E, count, cfg, **kw):
    return [g.ACAS2DVecEnv(E, N, device=DEV, dtype=torch.float32, config=cfg, **kw) for _ in range(count)]


_STATE = ("own_x", "own_y", "own_psi", "own_v", "goal_x", "goal_y", "trf_x", "trf_y", "trf_psi", "trf_v", "steps",
          "total_reward", "episode")


def _assert_launches_equal(a, b, env_a, env_b, keys):
    for k in keys:
        assert H.bits_equal(a[k], b[k]), k
    for name in _STATE:
        assert H.bits_equal(getattr(env_a, name), getattr(env_b, name)), name
    assert H.bits_equal(env_a.outputs["obs"], env_b.outputs["obs"])


_ROLLOUT_KEYS = ("actions", "obs", "reward", "done_u8", "outcome", "episode_return", "episode_steps", "terminal_observation")


# -- N = 8: the bridge between the two kernels, no tolerance
@pytest.mark.gpu
@pytest.mark.parametrize("cfg_name", ("default", "small"))
def test_group_rollout_policy_equals_thread_per_env_bit_for_bit(gpu, cfg_name):
    """rollout_policy(group=True) (shape (4,2)) against rollout_policy() (shape (8,1)) on a twin env, some envs starting
    in exact parallel flight (NaN observation, NaN action): actions, observations, rewards, masks, side channels and
    the final state, as bit patterns.  E = 1001: a partial wave in both shapes."""
    g = gpu
    N, E, T = 8, 1001, 100
    cfg = _config(g, N, cfg_name, **({"max_steps": 12} if cfg_name == "default" else {}))
    env, twin = _envs(g, N, E, 2, cfg, seed=21, env_offset=37)
    env.reset()
    twin.reset()
    rows = np.arange(5, E, 13)
    state, obs0 = LS.parallel_flight(env, rows)
    twin.set_state(*state, np.zeros(E, np.int32), observe=True)
    assert np.isnan(obs0[rows]).any(1).all()
    for kind in ("plain", "saturating"):
        for v in (env, twin):
            v.set_state(*state, np.zeros(E, np.int32), observe=True)
        pol = LS.scaled_actor(g, 5 + 3 * N, kind, obs0)
        a = env.rollout_policy(pol, T, keep_terminal_obs=True, group=True)
        b = twin.rollout_policy(pol, T, keep_terminal_obs=True)
        torch.cuda.synchronize()
        _assert_launches_equal(a, b, env, twin, _ROLLOUT_KEYS)
        assert torch.isnan(a["actions"][0, rows]).all() and int(a["done"].sum()) > E
    print("rollout_policy N=8 %s: group == thread-per-env over %d steps x %d envs, %d episodes finished"
          % (cfg_name, T, E, int(a["done"].sum())))


@pytest.mark.gpu
@pytest.mark.parametrize("cfg_name", ("default", "small"))
def test_group_collect_equals_thread_per_env_bit_for_bit(gpu, cfg_name):
    """collect(group=True) against collect() on a twin env, with a noise counter that wraps and global env indices on
    both sides of 2^32: raw actions, values, log-probabilities and everything rollout_policy() writes."""
    g = gpu
    N, E, T = 8, 1001, 100
    seed, nstep, off = 0x243F6A8885A308D3, 2 ** 32 - 5, 2 ** 32 - 259
    cfg = _config(g, N, cfg_name, **({"max_steps": 12} if cfg_name == "default" else {}))
    env, twin = _envs(g, N, E, 2, cfg, seed=21, env_offset=off)
    env.reset()
    twin.reset()
    rows = np.arange(3, E, 11)
    state, obs0 = LS.parallel_flight(env, rows)
    twin.set_state(*state, np.zeros(E, np.int32), observe=True)
    assert np.isnan(obs0[rows]).any(1).all()
    pol = LS.actor_critic(g, 5 + 3 * N)
    a = env.collect(pol, T, noise_seed=seed, noise_step=nstep, group=True)
    b = twin.collect(pol, T, noise_seed=seed, noise_step=nstep)
    torch.cuda.synchronize()
    _assert_launches_equal(a, b, env, twin, ("actions", "values", "logp", "obs", "reward", "done_u8", "outcome",
                                              "episode_return", "episode_steps"))
    assert int(a["done"].sum()) > E and torch.isfinite(a["actions"]).all()
    print("collect N=8 %s: group == thread-per-env over %d steps x %d envs, %d episodes finished"
          % (cfg_name, T, E, int(a["done"].sum())))


@pytest.mark.gpu
@pytest.mark.parametrize("cfg_name", ("default", "small"))
@pytest.mark.parametrize("E", (37, 100, 130))
def test_group_policy_set_equals_thread_per_env_bit_for_bit(gpu, E, cfg_name):
    """evaluate_policies_fused(K = 3, group=True) against the thread-per-env launch at N = 8."""
    g = gpu
    N = 8
    cfg = _config(g, N, cfg_name)
    own, trf, goal = H.parity_reset_states(cfg, 13, 0, E)
    pols = [LS.actor_critic(g, 5 + 3 * N, seed=s) for s in (1, 2, 3)]
    a = g.evaluate_policies_fused(pols, own, trf, goal, dtype=torch.float32, config=cfg, group=True)
    b = g.evaluate_policies_fused(pols, own, trf, goal, dtype=torch.float32, config=cfg)
    for k in ("outcome", "steps", "unfinished"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["total_reward"].view(np.uint64), b["total_reward"].view(np.uint64))
    assert a["outcome"].shape == (3, E) and (a["outcome"] != 0).all()


# -- N = 16, 32, 64 against float64
_WIDE = [(N, E) for N in (16, 32, 64) for E in (512, 510)]       # 510: a partial wave at every shape (64 / G = 16, 8, 4)
_WIDE_IDS = ["N%d-E%d" % c for c in _WIDE]


@pytest.mark.gpu
@pytest.mark.parametrize("N,E", _WIDE, ids=_WIDE_IDS)
def test_group_policy_actions_vs_float64(gpu, N, E):
    """rollout_policy(group=True): every action against clip(mean64, -1, 1) on the observation the kernel stepped from,
    for a plain, a saturating and a near-zero policy, with envs starting in exact parallel flight (NaN observation ->
    NaN action), across in-kernel resets (episodes of 12 steps)."""
    g = gpu
    D, T = 5 + 3 * N, 16
    rows = np.arange(5, E, 13)
    for kind in ("plain", "saturating", "small"):
        env, = _envs(g, N, E, 1, _config(g, N, max_steps=12), seed=21)
        env.reset()
        state, obs0 = LS.parallel_flight(env, rows)
        assert np.isnan(obs0[rows]).any(1).all()
        pol = LS.scaled_actor(g, D, kind, obs0)
        out = env.rollout_policy(pol, T, group=True)
        torch.cuda.synchronize()
        obs = np.concatenate([obs0[None], out["obs"][:T - 1].double().cpu().numpy()])
        ref = R.actor64(pol.actor_weights(), obs.reshape(T * E, D)).reshape(T, E)
        got = out["actions"].double().cpu().numpy()
        assert np.isnan(ref[0, rows]).all()
        assert np.array_equal(np.isnan(got), np.isnan(ref)), (kind, np.argwhere(np.isnan(got) != np.isnan(ref))[:5])
        fin = ~np.isnan(ref)
        worst = float(np.abs(got[fin] - ref[fin]).max())
        resets = int(out["done"].sum())
        print("rollout_policy group N=%d E=%d %s: worst |action - clip(mean64)| %.2e (bound 1e-5), %d resets"
              % (N, E, kind, worst, resets))
        assert worst < 1e-5, (kind, worst)
        assert resets >= E, resets
        z1, z2 = R.preactivations64(R.params64(pol), R.obs32(obs[fin]))
        if kind == "saturating":
            assert np.abs(z1).max() > 45 and np.abs(z2).max() > 45
        if kind == "small":
            assert max(np.abs(z1).max(), np.abs(z2).max()) < 0.1
        assert float((np.abs(ref[fin]) < 0.99).mean()) > 0.1, kind                # not everything clips


@pytest.mark.gpu
@pytest.mark.parametrize("N,E", _WIDE, ids=_WIDE_IDS)
def test_group_collector_vs_float64_and_twin_replay(gpu, N, E):
    """One collect(group=True) launch whose noise counter wraps (noise_step = 2^32 - 5, 24 steps), with half the envs at
    a global index >= 2^32, a key whose halves differ, and envs starting in exact parallel flight: actions = mean64 +
    exp(log_std) eps64, values = value64, logp = -eps64^2 / 2 - log_std - ln(2 pi) / 2; a twin env fed the launch's own
    clipped actions reproduces every observation, reward and mask bit for bit and ends in the same state."""
    g = gpu
    D, T = 5 + 3 * N, 24
    seed, nstep, off = 0x243F6A8885A308D3, 2 ** 32 - 5, 2 ** 32 - 259
    pol = LS.actor_critic(g, D)
    env, twin = _envs(g, N, E, 2, _config(g, N, max_steps=12), seed=21, env_offset=off)
    env.reset()
    twin.reset()
    rows = np.arange(3, E, 11)
    state, obs0 = LS.parallel_flight(env, rows)
    twin.set_state(*state, np.zeros(E, np.int32), observe=True)
    assert np.isnan(obs0[rows]).any(1).all() and not np.isnan(np.delete(obs0, rows, 0)).any()
    out = env.collect(pol, T, noise_seed=seed, noise_step=nstep, group=True)
    torch.cuda.synchronize()
    obs = out["obs"].double().cpu().numpy()
    p = R.params64(pol)
    mean, value = (x.reshape(T, E) for x in R.forward64(p, obs[:T].reshape(T * E, D), sample=True))
    eps = R.noise64(seed, nstep, off + np.arange(E), T)
    log_std = float(p["log_std"][0])
    act_ref = mean + np.exp(log_std) * eps
    logp_ref = -0.5 * eps ** 2 - log_std - R.LOG_SQRT_2PI
    act, val, logp = (out[k].double().cpu().numpy() for k in ("actions", "values", "logp"))
    eps_got = (act - mean) / np.exp(log_std)
    errs = {}
    for name, got, ref, tol in (("action", act, act_ref, 5e-6), ("value", val, value, 5e-6), ("eps", eps_got, eps, 1e-5),
                                ("logp", logp, logp_ref, 1e-5)):
        errs[name] = (float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max()), tol)
    print("collector group N=%d E=%d: " % (N, E) + ", ".join("%s %.2e (bound %.0e)" % (k, e, t) for k, (e, t) in errs.items()))
    for k, (e, t) in errs.items():
        assert e <= t, (k, e, t)
    # the NaN rows: mean and value of step 0 were taken on the zeroed input
    assert np.abs(val[0, rows] - value[0, rows]).max() <= 5e-6 * max(1.0, np.abs(value[0, rows]).max())
    assert np.abs(act[0, rows] - act_ref[0, rows]).max() <= 5e-6 * max(1.0, np.abs(act_ref[0, rows]).max())
    assert np.isfinite(act).all() and np.isfinite(val).all() and np.isfinite(logp).all()
    dones = H.replay_collect_on_twin(env, twin, out)
    assert dones >= E, dones                                                       # every env was reset in the kernel
    for name in _STATE:
        assert H.bits_equal(getattr(env, name), getattr(twin, name)), name


@pytest.mark.gpu
@pytest.mark.parametrize("N,E", _WIDE, ids=_WIDE_IDS)
def test_group_policy_rollout_replays_on_a_twin(gpu, N, E):
    """A twin env stepped with rollout_policy(group=True)'s actions reproduces every observation, reward, mask and side
    channel bit for bit and ends in the same state ("small" configuration: goals, collisions and timeouts)."""
    g = gpu
    T = 100
    cfg = _config(g, N, "small")
    env, twin = _envs(g, N, E, 2, cfg, seed=3, env_offset=37)
    env.reset()
    twin.reset()
    pol = LS.actor_critic(g, 5 + 3 * N)
    out = env.rollout_policy(pol, T, keep_terminal_obs=True, group=True)
    dones = 0
    for t in range(T):
        o, r, d, infos = twin.step(out["actions"][t])
        assert H.bits_equal(out["obs"][t], o) and H.bits_equal(out["reward"][t], r), t
        assert torch.equal(out["done"][t], d) and torch.equal(out["outcome"][t], infos.outcome), t
        assert H.bits_equal(out["terminal_observation"][t][d], infos.terminal_observation[d]), t
        assert H.bits_equal(out["episode_return"][t][d], infos.episode_return[d]), t
        assert torch.equal(out["episode_steps"][t][d], infos.episode_steps[d]), t
        dones += int(d.sum())
    for name in _STATE:
        assert H.bits_equal(getattr(env, name), getattr(twin, name)), name
    print("rollout_policy group N=%d E=%d under \"small\": twin replay exact, %d episodes finished" % (N, E, dones))
    assert dones >= E


# -- the K-policy evaluation at N = 64
@pytest.mark.gpu
@pytest.mark.parametrize("cfg_name", ("default", "small"))
@pytest.mark.parametrize("E", (37, 100, 130))
def test_group_policy_set_rows_equal_single_policy_evaluations(gpu, E, cfg_name):
    """K = 3 at N = 64: row k equals evaluate_policy_fused(policies[k], group=True) -- the first `done` of a
    rollout_policy(group=True) run of the same episodes -- bit for bit in outcome, steps and total_reward."""
    g = gpu
    N = 64
    cfg = _config(g, N, cfg_name)
    own, trf, goal = H.parity_reset_states(cfg, 13, 0, E)
    pols = [LS.actor_critic(g, 5 + 3 * N, seed=s) for s in (1, 2, 3)]
    got = g.evaluate_policies_fused(pols, own, trf, goal, dtype=torch.float32, config=cfg, group=True)
    assert got["outcome"].shape == (3, E) and got["unfinished"].shape == (3,)
    for k, pol in enumerate(pols):
        want = g.evaluate_policy_fused(pol, own, trf, goal, dtype=torch.float32, config=cfg, group=True)
        assert np.array_equal(got["outcome"][k], want["outcome"]) and np.array_equal(got["steps"][k], want["steps"]), k
        assert np.array_equal(got["total_reward"][k].view(np.uint64), want["total_reward"].view(np.uint64)), k
        assert int(got["unfinished"][k]) == want["unfinished"], k
    assert (got["outcome"] != 0).all()
    assert len({got["total_reward"][k].tobytes() for k in range(3)}) == 3          # the policies do play differently


# -- the trainer
@pytest.mark.gpu
def test_trainer_collects_evaluates_and_checkpoints_at_16_traffic(gpu, tmp_path):
    """256 envs x 16 traffic, float32: PPOTrainer(collector="fused", updater="graphs") takes the group launches by
    itself; three iterations of learn() with eval_every and save_dir leave evaluations.npz with finite scores and a
    best_model.zip that load_sb3_policy reads back and that reproduces its recorded evaluation."""
    import random
    g = gpu
    venv = g.ACAS2DVecEnv(256, 16, device=DEV, dtype=torch.float32, seed=13)
    tr = g.PPOTrainer(venv, g.PPOConfig(n_steps=32, batch_size=1024, n_epochs=2, seed=13), collector="fused", updater="graphs")
    per_it = 256 * 32
    hist = tr.learn(3 * per_it, log=None, eval_every=per_it, eval_episodes=10, eval_seed=7, save_dir=str(tmp_path))
    its = [r for r in hist if not r.get("eval")]
    evals = [r for r in hist if r.get("eval")]
    assert len(its) == 3 and len(evals) == 3
    ev = np.load(tmp_path / "results" / "evaluations.npz")
    assert ev["timesteps"].tolist() == [per_it, 2 * per_it, 3 * per_it]
    assert ev["results"].shape == ev["ep_lengths"].shape == (3, 10)
    assert np.isfinite(ev["results"]).all() and (ev["ep_lengths"] > 0).all()
    assert [r["mean_reward"] for r in evals] == ev["results"].mean(1).tolist()
    best = g.load_sb3_policy(tmp_path / "best_model.zip")
    assert best.obs_dim == 53
    rng = random.Random(7)
    episodes = [g.reset_parity.draw_episodes(venv.config, 10, rng) for _ in range(3)]
    k = int(np.argmax(ev["results"].mean(1)))
    again = g.evaluate_policies_fused([best], *episodes[k], dtype=torch.float32, group=True)
    assert np.array_equal(again["total_reward"][0].view(np.uint64), ev["results"][k].view(np.uint64))
    with pytest.raises(ValueError, match="16, 32, 64"):
        g.PPOTrainer(g.ACAS2DVecEnv(64, 5, device=DEV, dtype=torch.float32), collector="fused")
