"""Scoring sets of policies in one launch (acas2d_evaluate_policies_*, policy.evaluate_policies_fused), writing SB3
policy zips (policy.save_sb3_policy), and the evaluation / checkpoint callbacks of PPOTrainer.learn() -- the workflow of
the reference's training_main.py:28-52 (EvalCallback + CheckpointCallback) and checkpoint_testing_main.py.

CPU: the zip round trip and the argument validation of the two new entry points.  GPU (-m gpu): every row of a K-policy
launch equals evaluate_policy_fused() of that policy bit for bit, at every thread-per-env instantiation; the reference's
recorded score; routing of many policies; NaN episodes; the step budget; the trainer callbacks."""
import io
import os
import random
import zipfile

import numpy as np
import pytest
import torch

import helpers as H
import learner_ref as R
import scoring_rejections_support as SR

DEV = "cuda:0"
FIXTURE = os.path.join(H.GOLDEN, "ref_policy_best_model.npz")


@pytest.fixture(scope="module")
def g():
    import gym_acas2d_amd as g
    return g


def _bits_equal(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_save_sb3_policy_round_trip(g, tmp_path):
    """The reference's trained policy, loaded into ActorCritic and saved: policy.pth holds exactly the fixture's 13
    tensors (keys, shapes, dtypes, bits), the version member says 1.1.0, and both loaders read it back bit for bit."""
    fx = np.load(FIXTURE, allow_pickle=False)
    tensors = {k: fx[k] for k in fx.files if k != "sb3_version"}
    assert len(tensors) == 13
    ac = g.ActorCritic(8)
    ac.load_sb3_state_dict(tensors)
    path = g.save_sb3_policy(ac, tmp_path / "sub" / "model.zip")
    with zipfile.ZipFile(path) as z:
        assert set(z.namelist()) == {"policy.pth", "_stable_baselines3_version"}
        assert z.read("_stable_baselines3_version").decode() == "1.1.0"
        sd = torch.load(io.BytesIO(z.read("policy.pth")), map_location="cpu", weights_only=True)
    assert set(sd) == set(tensors)
    for k, want in tensors.items():
        got = sd[k].numpy()
        assert got.shape == want.shape and got.dtype == want.dtype == np.float32, k
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), k
    pol = g.load_sb3_policy(path)
    ref = g.load_sb3_policy(FIXTURE)
    for a, b in zip(pol.actor_weights(), ref.actor_weights()):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    ac2 = g.ActorCritic(8)
    ac2.load_sb3_state_dict(sd)
    for (k, a), (_, b) in zip(ac2.state_dict().items(), ac.state_dict().items()):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), k


def test_evaluate_policies_validation_is_in_the_golden_grid(g):
    """acas2d_evaluate_policies_* reject every bad argument with ACAS2D_EINVAL and a message, before any launch:
    tests/test_scoring_rejections_host.py holds them to the whole text of each.  Here: that its grid has them, and the one
    call it does not make."""
    for dt in ("f32", "f64"):
        SR.covered("acas2d_evaluate_policies_" + dt)
    # a traffic count between two thread-per-env shapes
    assert SR.call(g, "acas2d_evaluate_policies_f32", 8, {"n": 6}) == (
        SR.EINVAL, "acas2d_evaluate_policies: n_traffic = 6 has no thread-per-env shape for this element type")


# ---- GPU ------------------------------------------------------------------------------------------------------------
def _random_actor(g, D, seed):
    """An actor whose actions do not all saturate or vanish (a fresh ActorCritic's head is scaled by 0.01)."""
    torch.manual_seed(seed)
    pol = g.ActorCritic(D)
    with torch.no_grad():
        pol.action_net.weight.mul_(40.0)
    return pol


def _three_policies(g, N):
    D = 5 + 3 * N
    if N != 1:
        return [_random_actor(g, D, s) for s in (1, 2, 3)]
    ref = g.load_sb3_policy(FIXTURE)
    fx = np.load(FIXTURE, allow_pickle=False)
    pert = g.ActorCritic(D)
    pert.load_sb3_state_dict({k: fx[k] for k in fx.files if k != "sb3_version"})
    with torch.no_grad():
        gen = torch.Generator().manual_seed(5)
        for p in pert.mlp_extractor.policy_net.parameters():
            p.add_(1e-3 * torch.randn(p.shape, generator=gen))
    torch.manual_seed(11)
    return [ref, pert, g.ActorCritic(D)]


def _assert_rows_equal(got, k, want):
    assert np.array_equal(got["outcome"][k], want["outcome"]), k
    assert np.array_equal(got["steps"][k], want["steps"]), k
    assert _bits_equal(got["total_reward"][k], want["total_reward"]), k
    assert int(got["unfinished"][k]) == want["unfinished"], k


_CONFIGS = ("default", "small")


@pytest.mark.gpu
@pytest.mark.parametrize("cfg_name", _CONFIGS)
@pytest.mark.parametrize("E", (37, 100, 130))
@pytest.mark.parametrize("kern", R.POLICY_KERNELS, ids=[R.kernel_id(k) for k in R.POLICY_KERNELS])
def test_policy_set_rows_equal_single_policy_evaluations(g, kern, E, cfg_name):
    """K = 3 policies in one launch: row k == evaluate_policy_fused(policies[k]) bit for bit in outcome, steps and
    total_reward, at every thread-per-env instantiation.  E = 37 (a partial wave and padding), 100 (padding within the
    second wave), 130 (a policy spanning three waves)."""
    dtype, fast, N = kern
    cfg = g.ACAS2DConfig(n_traffic=N, fast_math=fast, **(H.NONDEFAULT_CONFIGS[cfg_name] if cfg_name != "default" else {}))
    own, trf, goal = H.parity_reset_states(cfg, 13, 0, E)
    pols = _three_policies(g, N)
    dt = getattr(torch, dtype)
    got = g.evaluate_policies_fused(pols, own, trf, goal, dtype=dt, config=cfg)
    assert got["outcome"].shape == (3, E) and got["unfinished"].shape == (3,)
    for k, pol in enumerate(pols):
        _assert_rows_equal(got, k, g.evaluate_policy_fused(pol, own, trf, goal, dtype=dt, config=cfg))
    assert (got["outcome"] != 0).all()


@pytest.mark.gpu
def test_policy_set_reproduces_the_reference_policy_evaluation(g):
    """float64 EXACT, the reference's trained policy twice plus another on the 100 test episodes: rows 0 and 1 are the
    reference's recorded evaluation (mean return 1210.069, mean length 704.35, 100 goals), held as tightly as the
    single-policy rollout holds it, and equal to each other bit for bit."""
    own, trf, goal = H.parity_reset_states(g.ACAS2DConfig(), 13, 0, 100)
    ref = g.load_sb3_policy(FIXTURE)
    got = g.evaluate_policies_fused([ref, FIXTURE, _random_actor(g, 8, 4)], own, trf, goal)
    for k in (0, 1):
        assert (got["outcome"][k] == 1).all() and got["unfinished"][k] == 0
        H.assert_matches_reference_policy_eval(got["total_reward"][k], got["steps"][k], got["path_length"][k], tol=1e-4)
    assert _bits_equal(got["total_reward"][0], got["total_reward"][1]) and np.array_equal(got["steps"][0], got["steps"][1])
    assert not np.array_equal(got["steps"][2], got["steps"][0])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ("float32", "float64"))
def test_policy_set_routes_each_policy_to_its_rows(g, dtype):
    """K = 40 policies x 100 episodes (40 x 128 envs: 40 workgroups): permuting the policy list permutes the rows."""
    own, trf, goal = H.parity_reset_states(g.ACAS2DConfig(), 13, 0, 100)
    pols = [_random_actor(g, 8, 100 + i) for i in range(40)]
    dt = getattr(torch, dtype)
    base = g.evaluate_policies_fused(pols, own, trf, goal, dtype=dt)
    assert len({base["steps"][k].tobytes() for k in range(40)}) > 20          # the policies do play differently
    perm = np.random.default_rng(0).permutation(40)
    got = g.evaluate_policies_fused([pols[i] for i in perm], own, trf, goal, dtype=dt)
    for r, k in enumerate(perm):
        assert np.array_equal(got["outcome"][r], base["outcome"][k]) and np.array_equal(got["steps"][r], base["steps"][k])
        assert _bits_equal(got["total_reward"][r], base["total_reward"][k]), (r, k)


@pytest.mark.gpu
@pytest.mark.parametrize("N", (1, 3))
def test_policy_set_nan_episodes_match_single_policy_evaluations(g, N):
    """Episodes starting in exact parallel flight (NaN d_cpa, NaN actions): outcome, steps and the NaN pattern of the
    returns equal evaluate_policy_fused's, row by row."""
    E = 24
    own, trf, goal = H.parity_reset_states(g.ACAS2DConfig(n_traffic=N), 13, 0, E)
    rows = np.array([0, 5, 11, 17])
    trf[rows, 0, 2], trf[rows, 0, 3] = own[rows, 2], own[rows, 3]
    pols = _three_policies(g, N)[:2]
    got = g.evaluate_policies_fused(pols, own, trf, goal)
    nan_seen = False
    for k, pol in enumerate(pols):
        want = g.evaluate_policy_fused(pol, own, trf, goal)
        assert np.array_equal(got["outcome"][k], want["outcome"]) and np.array_equal(got["steps"][k], want["steps"]), k
        assert np.array_equal(np.isnan(got["total_reward"][k]), np.isnan(want["total_reward"])), k
        assert _bits_equal(got["total_reward"][k], want["total_reward"]), k
        nan_seen |= bool(np.isnan(want["total_reward"][rows]).any())
    print("NaN returns among the parallel-flight rows:", nan_seen)


@pytest.mark.gpu
@pytest.mark.parametrize("kern", (("float32", True, 1), ("float64", False, 3)), ids=("float32-N1", "float64-N3"))
def test_policy_set_step_budget(g, kern):
    """A budget far above max_steps + 1 changes nothing; a short one leaves episodes unfinished (outcome 0) exactly
    where evaluate_policy_fused(max_steps=...) does."""
    dtype, fast, N = kern
    cfg = g.ACAS2DConfig(n_traffic=N, fast_math=fast)
    own, trf, goal = H.parity_reset_states(cfg, 13, 0, 100)
    pols = _three_policies(g, N)
    dt = getattr(torch, dtype)
    full = g.evaluate_policies_fused(pols, own, trf, goal, dtype=dt, config=cfg)
    long = g.evaluate_policies_fused(pols, own, trf, goal, dtype=dt, config=cfg, max_steps=4 * cfg.max_steps)
    for key in ("outcome", "steps", "unfinished"):
        assert np.array_equal(full[key], long[key]), key
    assert _bits_equal(full["total_reward"], long["total_reward"])
    short = g.evaluate_policies_fused(pols, own, trf, goal, dtype=dt, config=cfg, max_steps=700)
    assert short["unfinished"].sum() > 0 and (short["unfinished"] < 100).any()
    for k, pol in enumerate(pols):
        want = g.evaluate_policy_fused(pol, own, trf, goal, dtype=dt, config=cfg, max_steps=700)
        _assert_rows_equal(short, k, want)
        assert np.array_equal(short["outcome"][k] == 0, want["outcome"] == 0)


def _train(g, collector, tmp, evaluate):
    venv = g.ACAS2DVecEnv(64, 1, device=DEV, dtype=torch.float32, seed=13)
    tr = g.PPOTrainer(venv, g.PPOConfig(n_steps=64, batch_size=1024, n_epochs=2, seed=13), collector=collector)
    snaps = []

    def log(rec):
        if not rec.get("eval"):
            snaps.append({k: v.detach().clone() for k, v in tr.policy.state_dict().items()})
    kw = dict(eval_every=4096, eval_episodes=10, eval_seed=7, save_dir=str(tmp), checkpoint_every=8192) if evaluate else {}
    hist = tr.learn(4 * 64 * 64, log=log, **kw)
    return tr, hist, snaps


@pytest.mark.gpu
@pytest.mark.parametrize("collector", ("fused", "graphs"))
def test_trainer_evaluation_and_checkpoints(g, tmp_path, collector):
    """learn(eval_every=, checkpoint_every=, save_dir=): evaluations.npz in EvalCallback's layout (the reference's
    fixture's keys, dtypes and ranks), best_model.zip reproducing the best recorded mean on the recorded episodes,
    checkpoints named by timesteps -- and the same parameters after every iteration as the run without them."""
    tr, hist, snaps = _train(g, collector, tmp_path, True)
    _, hist0, snaps0 = _train(g, collector, tmp_path / "unused", False)
    assert not (tmp_path / "unused").exists()
    assert len(snaps) == len(snaps0) == 4 and len(hist0) == 4 and not any(r.get("eval") for r in hist0)
    for it, (a, b) in enumerate(zip(snaps, snaps0)):
        for k in a:
            assert torch.equal(a[k], b[k]), (it, k)

    fx = np.load(os.path.join(H.GOLDEN, "ref_training_evaluations.npz"))
    ev = np.load(tmp_path / "results" / "evaluations.npz")
    assert set(ev.files) == set(fx.files)
    for k in fx.files:
        assert ev[k].dtype == fx[k].dtype and ev[k].ndim == fx[k].ndim, k
    assert ev["timesteps"].tolist() == [4096, 8192, 12288, 16384]
    assert ev["results"].shape == ev["ep_lengths"].shape == (4, 10)
    evals = [r for r in hist if r.get("eval")]
    assert [r["timesteps"] for r in evals] == ev["timesteps"].tolist()
    assert [r["mean_reward"] for r in evals] == ev["results"].mean(1).tolist()

    # the recorded episodes: the eval stream of random.Random(eval_seed), 10 games per evaluation
    rng = random.Random(7)
    episodes = [g.reset_parity.draw_episodes(tr.venv.config, 10, rng) for _ in range(4)]
    best = int(np.argmax(ev["results"].mean(1)))                  # the first of equal maxima: "strictly greater"
    own, trf, goal = episodes[best]
    again = g.evaluate_policies_fused([str(tmp_path / "best_model.zip")], own, trf, goal, dtype=torch.float32)
    assert _bits_equal(again["total_reward"][0], ev["results"][best])
    assert float(again["total_reward"][0].mean()) == float(ev["results"][best].mean())
    assert np.array_equal(again["steps"][0].astype(np.int64) - 1, ev["ep_lengths"][best])
    assert sorted(os.listdir(tmp_path / "checkpoints")) == ["model_16384_steps.zip", "model_8192_steps.zip"]
    # the last checkpoint is the final policy
    last = g.load_sb3_policy(tmp_path / "checkpoints" / "model_16384_steps.zip")
    for a, b in zip(last.actor_weights(), tr.policy.actor_weights()):
        assert torch.equal(a, b.cpu())
