"""Monte Carlo campaigns on the GPU (acas2d_monte_carlo_*, policy.MonteCarlo): the accumulators of a campaign against the
existing entries folded on the host (tests/monte_carlo_support.py) -- integers exactly, the per-lane arrays bit for bit --
and the properties a campaign is used for: chaining, resuming, common random numbers, reproducibility, regenerating an
encounter.  70 lanes x 3 episodes, K = 3 (two policies and the all-zero one), 16 bins, at every shape family and under
two configs."""
import numpy as np
import pytest
import torch

import monte_carlo_support as S

pytestmark = pytest.mark.gpu
SHAPES = pytest.mark.parametrize("s", S.SHAPES, ids=[S.shape_id(s) for s in S.SHAPES])
EVERY_SHAPE = pytest.mark.parametrize("s", S.SHAPES + S.MORE_SHAPES, ids=[S.shape_id(s) for s in S.SHAPES + S.MORE_SHAPES])


@pytest.fixture(scope="module")
def g():
    import gym_acas2d_amd as g
    return g


_RAN = {}


def ran(g, s):
    """The accumulators of one fresh campaign of [a, b, zero] after run(EPISODES), computed once per shape."""
    if s not in _RAN:
        acc = S.campaign(g, s).run(S.EPISODES).accumulators()
        for a in acc.values():
            a.setflags(write=False)
        _RAN[s] = acc
    return _RAN[s]


def same(g, got, want):
    bad = S.mismatches(g, got, want)
    assert not bad, {k: (np.asarray(got[k]).ravel()[:6], np.asarray(want[k]).ravel()[:6]) for k in bad}


@EVERY_SHAPE
def test_equals_the_existing_entries_bit_for_bit(g, s):
    """reset_to_episode(c) + evaluate_policies_fused(safety=True) for c = 0, 1, 2, folded by records.monte_carlo_reduce():
    the in-kernel redraw, the restart of the statistics and the folding, all at once -- at every compiled float32 work shape
    (S.MORE_SHAPES: the three the property tests below leave out)."""
    ref = S.reference(g, s)
    assert ref["outcome_count"].sum(1).tolist() == [S.LANES * S.EPISODES] * 3       # (the reference itself: test below)
    same(g, ran(g, s), ref)


def test_the_reference_is_not_vacuous(g):
    """Asserted on the reference side.  Per shape: exactly 70 x 3 episodes per policy (padding lanes count nothing) and
    nothing unfinished; across the parametrisation: every outcome, losses of separation, a histogram that spreads."""
    seen = np.zeros(4, np.int64)
    los = bins = 0
    for s in S.SHAPES + S.MORE_SHAPES:
        ref = S.reference(g, s)
        assert ref["outcome_count"].sum(1).tolist() == ref["sep_hist"].sum(1).tolist() == [S.LANES * S.EPISODES] * 3, S.shape_id(s)
        assert ref["outcome_count"][:, 0].tolist() == [0, 0, 0]
        assert ref["lane_worst_sep"].shape == (3, S.LANES) and np.isfinite(ref["lane_worst_sep"]).all()
        seen += ref["outcome_count"].sum(0)
        los += int(ref["los_episodes"].sum())
        bins = max(bins, int((ref["sep_hist"] > 0).sum(1).max()))
        if s.max_steps == 150:
            assert ref["outcome_count"][:, 3].sum() > 0, S.shape_id(s)              # the short config does time out
    assert (seen[1:] > 0).all() and los > 0 and bins >= 2, (seen, los, bins)


@pytest.mark.parametrize("dtype", (torch.float32, torch.float64), ids=("f32", "f64"))
@pytest.mark.parametrize("N", (1, 8))
def test_reset_to_episode_names_the_engines_episodes(g, dtype, N):
    """reset_to_episode(2) == reset() and two reset_masked(all), bit for bit: state, counters and first observation."""
    E = S.LANES
    a = g.ACAS2DVecEnv(E, N, device=S.DEV, dtype=dtype, seed=S.SEED)
    b = g.ACAS2DVecEnv(E, N, device=S.DEV, dtype=dtype, seed=S.SEED)
    obs_a = a.reset_to_episode(2)
    b.reset()
    every = torch.ones(E, dtype=torch.uint8, device=S.DEV)
    b.reset_masked(every)
    obs_b = b.reset_masked(every)
    for name in ("own_x", "own_y", "own_psi", "own_v", "goal_x", "goal_y", "trf_x", "trf_y", "trf_psi", "trf_v", "steps",
                 "total_reward", "episode", "status"):
        assert S.bits_equal(getattr(a, name).cpu().numpy(), getattr(b, name).cpu().numpy()), name
    assert S.bits_equal(obs_a.cpu().numpy(), obs_b.cpu().numpy())
    assert a.episode.cpu().numpy().tolist() == [2] * E
    # ... per env, and the counter 0 is reset()'s
    ctr = np.arange(E) % 3
    c = g.ACAS2DVecEnv(E, N, device=S.DEV, dtype=dtype, seed=S.SEED)
    c.reset_to_episode(ctr)
    pick = torch.as_tensor(ctr == 2, device=S.DEV)
    assert S.bits_equal(c.trf_psi[pick].cpu().numpy(), a.trf_psi[pick].cpu().numpy())
    b.reset()
    assert S.bits_equal(c.own_psi[torch.as_tensor(ctr == 0, device=S.DEV)].cpu().numpy(),
                        b.own_psi[torch.as_tensor(ctr == 0, device=S.DEV)].cpu().numpy())
    assert not S.bits_equal(a.trf_psi.cpu().numpy(), b.trf_psi.cpu().numpy())             # (the counters do draw apart)
    with pytest.raises(ValueError):
        c.reset_to_episode(-1)
    with pytest.raises(ValueError):
        c.reset_to_episode(np.zeros(E + 1, np.int64))


@SHAPES
def test_chaining(g, s):
    """run(2) then run(1) is run(3); one episode per launch is eight per launch."""
    same(g, S.campaign(g, s).run(2).run(1).accumulators(), ran(g, s))
    same(g, S.campaign(g, s).run(S.EPISODES, per_launch=1).accumulators(), ran(g, s))


@SHAPES
def test_first_episode_survives_a_state_dict(g, s):
    """run(5), state_dict(), a new campaign, load_state_dict(), run(2): the reference folded over counters 0 .. 6."""
    first = S.campaign(g, s).run(5)
    sd = first.state_dict()
    assert sd["first_episode"] == 5
    second = S.campaign(g, s).load_state_dict(sd).run(2)
    assert second.first_episode == 7
    same(g, second.accumulators(), S.reference(g, s, counters=7))


@SHAPES
def test_common_random_numbers(g, s):
    """Every policy meets the same encounters whatever its row and however many rows there are."""
    a, b, zero = S.policies(g, s)
    abz = ran(g, s)
    zba = S.campaign(g, s, pols=[zero, b, a]).run(S.EPISODES).accumulators()
    same(g, {k: v[[2, 1, 0]] for k, v in zba.items()}, abz)
    alone = S.campaign(g, s, pols=[b]).run(S.EPISODES).accumulators()
    same(g, alone, {k: v[[1]] for k, v in abz.items()})


@SHAPES
def test_reproducible(g, s):
    same(g, S.campaign(g, s).run(S.EPISODES).accumulators(), ran(g, s))


def test_refusals(g):
    """Refused before anything is launched, in the library's words (acas2d_last_error) or the package's."""
    f32 = S.Shape(torch.float32, True, 1, False, 1000)
    with pytest.raises(RuntimeError, match=r"acas2d_monte_carlo: episodes_per_lane = 0 \(at least 1\)"):
        S.campaign(g, f32).run(0)
    with pytest.raises(RuntimeError, match=r"acas2d_monte_carlo: n_bins = 0 \(at least 1\)"):
        g.MonteCarlo(S.policies(g, f32), S.LANES, n_bins=0, hist_max=100.0, device=S.DEV).run(1)
    with pytest.raises(ValueError, match="float32 only"):
        g.MonteCarlo(S.policies(g, f32), S.LANES, dtype=torch.float64, group=True, device=S.DEV)
    with pytest.raises(RuntimeError, match="acas2d_monte_carlo_group: n_traffic = 3 takes the thread-per-env shape C=3 G=1: "
                                           "use acas2d_monte_carlo_f32"):
        g.MonteCarlo([S.zero_policy(3)], S.LANES, group=True, n_traffic=3, device=S.DEV).run(1)
    with pytest.raises(RuntimeError, match="acas2d_monte_carlo: n_traffic = 16 has no thread-per-env shape"):
        g.MonteCarlo([S.zero_policy(16)], S.LANES, n_traffic=16, device=S.DEV).run(1)
    with pytest.raises(ValueError, match="policy must be the SB3 MlpPolicy actor 8 -> 64 -> 64 -> 1"):
        g.MonteCarlo([S.zero_policy(3)], S.LANES, n_traffic=1, device=S.DEV)
    mc = S.campaign(g, f32)
    with pytest.raises(RuntimeError):
        mc.run(0)
    assert mc.first_episode == 0 and mc.accumulators()["outcome_count"].sum() == 0       # a refusal leaves the campaign alone


@SHAPES
def test_encounter_closes_the_loop(g, s):
    """Each policy's closest encounter, regenerated from (lane, counter) and scored by the stats evaluator, has exactly
    that minimum separation."""
    mc = S.campaign(g, s).run(S.EPISODES)
    acc = ran(g, s)
    for k, top in enumerate(mc.worst(1)):
        (lane, counter, sep), = top
        assert sep == acc["lane_worst_sep"][k].min() and acc["lane_worst_sep"][k, lane] == sep
        assert counter == acc["lane_worst_episode"][k, lane] and 0 <= counter < S.EPISODES
        own, trf, goal = mc.encounter(lane, counter)
        assert own.shape == (1, 4) and trf.shape == (1, s.N, 4) and goal.shape == (1, 2)
        res = g.evaluate_policies_fused(S.policies(g, s), own, trf, goal, dtype=s.dtype, device=S.DEV, config=S.config(g, s),
                                        group=s.group, safety=True)
        assert S.bits_equal(res["min_separation"][k, :1], np.asarray([sep], S.npdt(s)))
    three = mc.worst(3)
    assert [len(t) for t in three] == [3, 3, 3] and all(t[0][2] <= t[1][2] <= t[2][2] for t in three)


def test_summary_of_a_campaign(g):
    """summary() is records.monte_carlo_summary() of the accumulators; the zero policy is a row like any other."""
    s = S.SHAPES[0]
    mc = S.campaign(g, s).run(S.EPISODES)
    got, want = mc.summary(baseline=2), g.records.monte_carlo_summary(ran(g, s), baseline=2, hist_max=mc.hist_max)
    assert mc.hist_max == 4.0 * S.config(g, s).safe_distance
    for k, v in want.items():
        assert np.array_equal(np.asarray(got[k]), np.asarray(v), equal_nan=True), k
    assert got["episodes"].tolist() == [S.LANES * S.EPISODES] * 3 and got["risk_ratio"][2] == 1.0
    assert got["hist_edges"][-1] == mc.hist_max and len(got["hist_edges"]) == S.N_BINS + 1
