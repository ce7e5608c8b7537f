"""Pilot response delay and actuation lag on the GPU (acas2d_evaluate_policies_delayed_*, acas2d_monte_carlo_delayed_*;
policy.DelayedDisturbance): the clipped action reaches the aircraft `delay` steps late and through a first-order lag, in front
of the actuator's error.  Everything bit for bit.

  1  the delayed evaluator against the host loop of tests/response_support.py: noise_scoring_support.host_loop() with a delay
     queue and records.response_lag_step() in front of records.disturb_action() -- no other new arithmetic;
  2  delay 0 and lag 0: the correlated entries' bits, evaluator and campaign;
  3  the action that never arrives: with zero sigmas and delay = max_steps, or lag = 1, every policy's row is the all-zero
     policy's row of the PLAIN stats evaluator -- an anchor that shares no code with the host loop;
  4  the delayed campaign against reset_to_episode(c) + that evaluator folded by records.monte_carlo_reduce(), where lanes of
     one wave restart their delay lines and lags at different steps;
  5  the properties a campaign is used for (chaining: what one launch leaves in the ring the next must not read);
  6  refusals.

The evaluator and the campaign fill their ring with NaN, so a slot read before the episode at hand wrote it, or another env's
column, ends as a NaN flown and fails 1 to 4.  70 episodes / lanes: a full wave and a partial one thread per env, 18 waves at
the (4, 16) group shape."""
import numpy as np
import pytest
import torch

import eval_stats_support as ES
import monte_carlo_support as MS
import noise_scoring_support as NS
import response_support as RS
from noise_scoring_support import CAMPAIGN, CORRELATED, EVAL_IDS, EVAL_SHAPES, NOISE_EPISODE, RHO, SIGMAS, fused, ran, reference, same
from response_support import BOTH, DELAY, LAG, NEUTRAL, NOMINAL

pytestmark = pytest.mark.gpu
DEV = ES.DEV
F32 = torch.float32
THREE = ((1, False), (8, False), (16, True))               # (1), (8) and (16, group)
THREE_IDS = [NS.shape_id(s) for s in THREE]


@pytest.fixture(scope="module")
def g():
    import gym_acas2d_amd as g
    return g


# ---- 1: the evaluator against a host loop ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", EVAL_SHAPES, ids=EVAL_IDS)
def test_delayed_and_lagged_evaluator_equals_the_host_loop(g, shape):
    assert g.policy.evaluate_policies_entry(F32, shape[1], True, disturbed=True, delayed=True) == \
        "acas2d_evaluate_policies_delayed%s_f32" % ("_group" if shape[1] else "")
    RS.evaluator_equals_the_host_loop(g, BOTH, shape)


@pytest.mark.parametrize("shape", THREE, ids=THREE_IDS)
@pytest.mark.parametrize("fl", (DELAY, LAG), ids=lambda fl: fl.name)
def test_delay_or_lag_alone_equals_the_host_loop(g, fl, shape):
    RS.evaluator_equals_the_host_loop(g, fl, shape)


# ---- 2: the neutral values ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", THREE, ids=THREE_IDS)
def test_no_delay_and_no_lag_is_the_correlated_evaluator(g, shape):
    N, group = shape
    want = fused(g, N, group, disturbance=CORRELATED.disturbance(g), noise_episode=NOISE_EPISODE)
    got = fused(g, N, group, disturbance=NEUTRAL.disturbance(g), noise_episode=NOISE_EPISODE)
    assert set(got) == set(want) and len(want) >= 11
    for k in want:
        assert ES.bits_equal(got[k], want[k]), k
    assert (want["outcome"] != 0).all()


@pytest.mark.parametrize("shape", THREE, ids=THREE_IDS)
def test_no_delay_and_no_lag_is_the_correlated_campaign(g, shape):
    s = MS.Shape(F32, True, shape[0], shape[1], 150)
    mc = NS.campaign(g, NEUTRAL, s)
    assert mc.entry == "acas2d_monte_carlo_delayed%s_f32" % ("_group" if s.group else "")
    want = ran(g, CORRELATED, s)
    same(g, mc.run(MS.EPISODES).accumulators(), want)
    assert want["outcome_count"].sum(1).tolist() == [MS.LANES * MS.EPISODES] * 3


# ---- 3: the action that never arrives -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", THREE, ids=THREE_IDS)
@pytest.mark.parametrize("response", (dict(delay=150), dict(lag=1.0), dict(delay=150, lag=1.0)), ids=("delay", "lag", "both"))
def test_an_action_that_never_arrives_is_the_unequipped_aircraft(g, response, shape):
    """Zero sigmas; delay = max_steps of the 150-step config (an episode plays at most 150 steps: the oldest is 149 steps old), or
    lag = 1 (gain 0).  The aircraft flies 0 at every step whatever the network says: the plain stats evaluator's row of the
    all-zero policy on the same encounters."""
    s = MS.Shape(F32, True, shape[0], shape[1], 150)
    cfg = MS.config(g, s)
    assert cfg.max_steps == 150
    v = g.ACAS2DVecEnv(MS.LANES, s.N, device=DEV, dtype=F32, seed=MS.SEED, config=cfg)
    v.reset_to_episode(0)
    own, trf, goal = g.policy.read_state(v)
    plain = MS.per_counter(g, s)[0]                            # [a, b, zero] by acas2d_evaluate_policies_stats_*, counter 0
    assert (plain["outcome"] != 0).all() and (plain["outcome"][2] == 3).any()                 # ... some by timeout: all 150 steps
    assert not ES.bits_equal(plain["max_abs_a_lat"][0], plain["max_abs_a_lat"][2])            # the networks do steer
    never = g.DelayedDisturbance.normalised(**RS.ZERO_SIGMAS, **RHO, **response)
    got = g.evaluate_policies_fused(MS.policies(g, s), own, trf, goal, dtype=F32, device=DEV, config=cfg, group=s.group,
                                    safety=True, disturbance=never)
    assert set(got) == set(plain)
    for key in plain:
        for k in range(3):
            assert ES.bits_equal(np.asarray(got[key])[k], np.asarray(plain[key])[2]), (key, k)


# ---- 4: the campaign against the evaluator ---------------------------------------------------------------------------------------------
@NS.CAMPAIGN_EVERY_SHAPE
def test_delayed_campaign_equals_the_delayed_evaluator(g, s):
    ref = reference(g, BOTH, s)
    assert ref["outcome_count"].sum(1).tolist() == [MS.LANES * MS.EPISODES] * 3
    assert ref["outcome_count"][:, 0].tolist() == [0, 0, 0] and np.isfinite(ref["lane_worst_sep"]).all()
    same(g, ran(g, BOTH, s), ref)
    assert MS.mismatches(g, ran(g, BOTH, s), ran(g, CORRELATED, s))                        # (and it is not the correlated campaign)


@pytest.mark.parametrize("s", [MS.Shape(F32, True, 1, False, 150), MS.Shape(F32, True, 16, True, 150)], ids=MS.shape_id)
def test_nominal_delayed_campaign_equals_the_evaluator(g, s):
    ref = reference(g, NOMINAL, s)
    assert ref["outcome_count"].sum(1).tolist() == [MS.LANES * MS.EPISODES] * 3 and np.isfinite(ref["lane_worst_sep"]).all()
    same(g, ran(g, NOMINAL, s), ref)
    plain = MS.reference(g, s)                                 # the delay alone moves the networks' rows, not the zero policy's
    assert MS.mismatches(g, {k: v[[0]] for k, v in ref.items()}, {k: v[[0]] for k, v in plain.items()})
    same(g, {k: v[[2]] for k, v in ref.items()}, {k: v[[2]] for k, v in plain.items()})


# ---- 5: the properties a campaign is used for -------------------------------------------------------------------------------------------
@CAMPAIGN
def test_delayed_chaining(g, s):
    """run(2).run(1) and three launches of one episode: every launch but the first finds the last one's actions in the ring."""
    NS.chaining(g, BOTH, s)


@CAMPAIGN
def test_delayed_campaign_survives_a_state_dict(g, s):
    mine = BOTH.disturbance(g)
    others = (None, NS.WHITE.disturbance(g), CORRELATED.disturbance(g),
              g.DelayedDisturbance.from_dict(dict(mine.to_dict(), delay=4)), g.DelayedDisturbance.from_dict(dict(mine.to_dict(), lag=0.5)))
    NS.survives_a_state_dict(g, BOTH, s, others, foreign=CORRELATED.disturbance(g), fields=dict(RHO, delay=5, lag=0.75))


@CAMPAIGN
def test_delayed_common_random_numbers(g, s):
    NS.common_random_numbers(g, BOTH, s)


@CAMPAIGN
def test_delayed_encounter_closes_the_loop(g, s):
    NS.encounter_closes_the_loop(g, BOTH, s)                  # (its replay keyword arguments carry the delay and the lag)


# ---- 6: refusals -------------------------------------------------------------------------------------------------------------------------
def forged(g, **fields):
    """A DelayedDisturbance with fields its constructor refuses: what only the C entry can still turn away."""
    d = BOTH.disturbance(g)
    for k, v in fields.items():
        object.__setattr__(d, k, v)
    return d


def test_refusals(g):
    s = MS.Shape(F32, True, 1, False, 1000)
    for bad, words in ((dict(delay=-1), r"delay_steps = -1 \(0 to 32767\)"), (dict(delay=32768), r"delay_steps = 32768 \(0 to 32767\)"),
                       (dict(lag=1.5), r"lag = 1\.5 \(in \[0, 1\]\)"), (dict(lag=float("nan")), r"lag = nan \(in \[0, 1\]\)")):
        with pytest.raises(ValueError, match="delay = |lag = "):
            g.DelayedDisturbance.normalised(**SIGMAS, **RHO, **bad)
        mc = MS.campaign(g, s, disturbance=BOTH.disturbance(g))
        mc.disturbance = forged(g, **bad)                       # (the campaign sized its ring by the honest one)
        with pytest.raises(RuntimeError, match="acas2d_monte_carlo_delayed: " + words):
            mc.run(1)
        assert mc.first_episode == 0 and mc.accumulators()["outcome_count"].sum() == 0      # a refusal leaves the campaign alone
    # the siblings' rejections under the entry's own name, a bad rho in front of a bad lag
    with pytest.raises(RuntimeError, match=r"acas2d_monte_carlo_delayed: rho_sep = .* \(each in \[0, 1\]\)"):
        mc = MS.campaign(g, s, disturbance=BOTH.disturbance(g))
        mc.disturbance = forged(g, rho_sep=2.0, lag=3.0)
        mc.run(1)
    with pytest.raises(RuntimeError, match=r"acas2d_monte_carlo_delayed: episodes_per_lane = 0 \(at least 1\)"):
        NS.campaign(g, BOTH, s).run(0)
    eps = ES.episodes(ES.config(g, 1))
    with pytest.raises(ValueError, match="float32 only"):
        g.MonteCarlo([MS.zero_policy(1)], MS.LANES, dtype=torch.float64, disturbance=BOTH.disturbance(g), device=DEV)
    with pytest.raises(ValueError, match="float32 only"):
        g.evaluate_policies_fused([MS.zero_policy(1)], eps.own, eps.trf, eps.goal, dtype=torch.float64, device=DEV,
                                  disturbance=BOTH.disturbance(g))
    with pytest.raises(RuntimeError, match="acas2d_monte_carlo_delayed_group: n_traffic = 3 takes the thread-per-env shape C=3 G=1: "
                                           "use acas2d_monte_carlo_delayed_f32"):
        g.MonteCarlo([MS.zero_policy(3)], MS.LANES, group=True, n_traffic=3, disturbance=BOTH.disturbance(g), device=DEV).run(1)
    # the collectors know no response
    v = g.ACAS2DVecEnv(64, 1, device=DEV, dtype=F32, auto_reset=True)
    v.reset()
    with pytest.raises(ValueError, match="white-noise only"):
        v.collect(g.ActorCritic(8), 2, disturbance=BOTH.disturbance(g))
    with pytest.raises(ValueError, match="know no response delay or lag"):
        g.CorrelatedDisturbanceSet(BOTH.disturbance(g))
