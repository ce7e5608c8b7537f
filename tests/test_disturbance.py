"""Sensor noise and actuator disturbance on the GPU (acas2d_evaluate_policies_disturbed_*, acas2d_monte_carlo_disturbed_*,
acas2d_disturbance_draw_f32; policy.Disturbance):

  1  the draws against the float64 specification of records.disturbance_normals(), and their first two moments;
  2  all four standard deviations 0: the undisturbed entries' bits;
  3  the disturbed evaluator against a host loop with no new arithmetic -- per step the observation of a latching env,
     records.disturb_observation() with the normals of the draw entry, the project's in-kernel network through a one-step
     rollout_policy() on a scratch env, records.disturb_action(), the latching step with record_trace=True, and
     records.episode_safety() on the trace;
  4  the disturbed campaign against reset_to_episode(c) + that evaluator folded by records.monte_carlo_reduce(), and the
     properties a campaign is used for;
  5  a network of zeros ignores its input: sensor noise alone leaves the all-zero policy's row as it is;
  6  refusals.

The shapes, the host loop, the campaign's reference and the campaign properties are tests/noise_scoring_support.py's, shared
with tests/test_correlated.py; WHITE is this file's flavour of them.  2, 3 and the campaign's equality with the evaluator run
at all nine compiled work shapes; 3 and that equality also under SATURATING, where the clamps of disturbed() decide every
step.

70 episodes / lanes: one full wave and a partial one thread per env, 18 waves at the (4, 16) group shape."""
import math

import numpy as np
import pytest
import torch

import eval_stats_support as ES
import helpers as H
import monte_carlo_support as MS
import noise_scoring_support as NS
from noise_scoring_support import CAMPAIGN, CAMPAIGN_SHAPES, EVAL_IDS, EVAL_SHAPES, WHITE, fused, ran, reference, same

pytestmark = pytest.mark.gpu
DEV = ES.DEV
F32 = torch.float32

# acas2d_disturbance_draw_f32 against records.disturbance_normals(): the largest absolute difference MEASURED on an MI355X
# over the sample of test_draws_against_the_specification (printed by it), and the bound: four times that,
# rounded up to one digit.  The difference is the hardware's approximate float32 log, sqrt, sin and cos and the float32
# products against float64 libm; the factor covers inputs the sample does not hold.
DRAW_MEASURED = 1.01e-5          # 1.009757e-05, at a cosine near its zero (|z| 0.0028)
DRAW_TOL = 5e-5
# That figure was taken against uniforms (k + 0.5) / 2^24 in float64.  The kernels form k + 0.5 in float32, where from k = 2^23
# on it is a tie that goes to the even neighbour; next to u = 1 the radius sqrt(-2 ln u) is all rounding, and k = 2^24 - 1
# gives u = 1 and the normal 0.  The wider sample of the test below met such a block (seed 7, lane 2^32 + 2, episode 2^32 - 1,
# step 45, slot 4: 0 against 1.95e-4), beyond the bound.  records.disturbance_normals() now rounds the uniform as the kernels
# do; against it the largest difference over the sample is 6.95e-7.  The bound stays where it was.


@pytest.fixture(scope="module")
def g():
    import gym_acas2d_amd as g
    return g


def the_disturbance(g):
    return WHITE.disturbance(g)


# ---- 1: the draws -----------------------------------------------------------------------------------------------------------------
def test_draws_against_the_specification(g):
    """... at both first lanes (the second crosses 2^32 inside the block), and -- the root of everything the noisy kernels
    are held to at wide keys -- also under a seed whose high word is not 0 and at the last episode counter."""
    worst, blocks = 0.0, 0
    for seed in (7, H.WIDE_SEED):
        for first_lane in (0, (1 << 32) - 3):
            for episode in (0, 5, (1 << 32) - 1):
                got = g.policy.disturbance_draw(seed, first_lane, 70, episode, 0, 121, 9, device=DEV)
                assert got.shape == (121, 70, 9, 3) and got.dtype == np.float32
                lanes = first_lane + np.arange(70, dtype=np.uint64)
                words = g.records.disturbance_words(seed, lanes[None, :, None], episode, np.arange(121)[:, None, None],
                                                    np.arange(9)[None, None, :])
                want = g.records.disturbance_normals(words)
                want[:, :, 0, 1:] = 0.0                                # the actuator slot: its normal and two zeros
                assert (got[:, :, 0, 1:] == 0.0).all()
                worst = max(worst, float(np.abs(got.astype(np.float64) - want).max()))
                blocks += 1
    print("\nacas2d_disturbance_draw_f32 against the float64 specification: largest absolute difference %.3e over %d normals "
          "(bound %r)" % (worst, blocks * 121 * 70 * (8 * 3 + 1), DRAW_TOL))
    assert worst <= DRAW_TOL


def test_draws_are_standard_normal(g):
    """2^20 draws per channel (1 024 lanes x 1 024 steps): |mean| < 5 / sqrt(n), |variance - 1| < 5 sqrt(2 / n)."""
    z = g.policy.disturbance_draw(11, 0, 1024, 0, 0, 1024, 2, device=DEV).astype(np.float64)
    n = 1 << 20
    for name, x in (("actuator", z[:, :, 0, 0]), ("sep", z[:, :, 1, 0]), ("cpa", z[:, :, 1, 1]), ("closing", z[:, :, 1, 2])):
        assert x.size == n and np.isfinite(x).all(), name
        assert abs(x.mean()) < 5 / math.sqrt(n), (name, x.mean())
        assert abs(x.var() - 1.0) < 5 * math.sqrt(2 / n), (name, x.var())


def test_draws_do_not_depend_on_how_they_are_asked_for(g):
    """A block is a function of (seed, lane, episode, step, slot): windows of lanes, steps and slots cut the same values."""
    whole = g.policy.disturbance_draw(7, 0, 70, 5, 0, 40, 9, device=DEV)
    part = g.policy.disturbance_draw(7, 64, 6, 5, 30, 10, 3, device=DEV)
    assert ES.bits_equal(part, whole[30:40, 64:70, :3])
    assert not ES.bits_equal(whole, g.policy.disturbance_draw(8, 0, 70, 5, 0, 40, 9, device=DEV))
    assert not ES.bits_equal(whole, g.policy.disturbance_draw(7, 0, 70, 4, 0, 40, 9, device=DEV))


# ---- 2: zero is identity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", EVAL_SHAPES, ids=EVAL_IDS)
def test_zero_disturbance_is_the_stats_evaluator(g, shape):
    N, group = shape
    plain = fused(g, N, group)
    zero = fused(g, N, group, disturbance=g.policy.Disturbance(seed=99), noise_episode=3)
    assert set(zero) == set(plain) and len(plain) >= 11
    for k in plain:
        assert ES.bits_equal(zero[k], plain[k]), k
    assert (plain["outcome"] != 0).all()


@pytest.mark.parametrize("shape", EVAL_SHAPES, ids=EVAL_IDS)
def test_zero_disturbance_is_the_undisturbed_campaign(g, shape):
    s = MS.Shape(F32, True, shape[0], shape[1], 150)
    plain = MS.campaign(g, s).run(MS.EPISODES).accumulators()
    zero = MS.campaign(g, s, disturbance=g.policy.Disturbance(seed=99)).run(MS.EPISODES).accumulators()
    assert not MS.mismatches(g, zero, plain)
    assert plain["outcome_count"].sum(1).tolist() == [MS.LANES * MS.EPISODES] * 3


# ---- 3: the evaluator against a host loop -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", EVAL_SHAPES, ids=EVAL_IDS)
def test_disturbed_evaluator_equals_the_host_loop(g, shape):
    N, group = shape
    rows = NS.loop_reference(g, WHITE, N, group)
    # teeth, on the reference alone: the disturbance moves the hardest manoeuvre of at least half of the episodes
    plain = ES.reference(g, F32, True, N)
    for k, row in enumerate(rows):
        assert (row[0] != 0).all(), "an episode of the reference did not finish"
        moved = int((ES.bits(row[3]["max_a_lat"]) != ES.bits(plain.stats["max_a_lat"][k])).sum())
        assert 2 * moved >= ES.E, (k, moved)
    NS.evaluator_equals_the_host_loop(g, WHITE, shape)


@NS.WIDE_EVAL_PARAMS
def test_disturbed_evaluator_equals_the_host_loop_at_wide_keys(g, shape):
    """The noise lane crossing 2^32 at episode 37 of the 70, the noise seed helpers.WIDE_SEED, the counter 2^32 - 1."""
    NS.evaluator_at_wide_keys(g, WHITE, shape)


@NS.SATURATING_EVAL
def test_saturating_evaluator_equals_the_host_loop(g, shape):
    NS.saturating_evaluator_equals_the_host_loop(g, NS.SATURATING, shape)


# ---- 4: the campaign against the evaluator ---------------------------------------------------------------------------------------------
@NS.CAMPAIGN_EVERY_SHAPE
def test_disturbed_campaign_equals_the_disturbed_evaluator(g, s):
    ref = reference(g, WHITE, s)
    assert ref["outcome_count"].sum(1).tolist() == [MS.LANES * MS.EPISODES] * 3
    same(g, ran(g, WHITE, s), ref)
    assert MS.mismatches(g, ran(g, WHITE, s), MS.reference(g, s))           # (and it is not the undisturbed campaign)


def test_saturating_campaign_equals_the_saturating_evaluator(g):
    s = NS.SATURATING_CAMPAIGN_SHAPE
    ref = reference(g, NS.SATURATING, s)
    assert ref["outcome_count"].sum(1).tolist() == [MS.LANES * MS.EPISODES] * 3
    same(g, ran(g, NS.SATURATING, s), ref)
    assert MS.mismatches(g, ran(g, NS.SATURATING, s), ran(g, WHITE, s))     # (and it is not the campaign under the small sigmas)


def test_the_campaign_reference_is_not_vacuous(g):
    seen = np.zeros(4, np.int64)
    for s in CAMPAIGN_SHAPES:
        ref = reference(g, WHITE, s)
        assert ref["outcome_count"].sum(1).tolist() == ref["sep_hist"].sum(1).tolist() == [MS.LANES * MS.EPISODES] * 3, MS.shape_id(s)
        assert ref["outcome_count"][:, 0].tolist() == [0, 0, 0]
        assert np.isfinite(ref["lane_worst_sep"]).all()
        seen += ref["outcome_count"].sum(0)
        if s.max_steps == 150:
            assert ref["outcome_count"][:, 3].sum() > 0, MS.shape_id(s)
    assert (seen[1:] > 0).all(), seen                                  # goals, collisions and timeouts


@NS.WIDE_CAMPAIGN
def test_disturbed_campaign_at_wide_keys(g, s):
    """monte_carlo_support.WIDE with the noise seed WIDE_SEED too: the lane's OWN counter names its noise (the reference
    plays counter c under noise_episode = c, up to 2^32 - 1), and the replay keywords of encounter() name the 64-bit lane."""
    NS.campaign_at_wide_keys(g, WHITE, s)


@CAMPAIGN
def test_disturbed_chaining(g, s):
    NS.chaining(g, WHITE, s)


@CAMPAIGN
def test_disturbed_campaign_survives_a_state_dict(g, s):
    NS.survives_a_state_dict(g, WHITE, s, others=(None, g.policy.Disturbance.normalised(**dict(NS.SIGMAS, seed=8))), foreign=None)


@CAMPAIGN
def test_disturbed_common_random_numbers(g, s):
    NS.common_random_numbers(g, WHITE, s)


@CAMPAIGN
def test_disturbed_encounter_closes_the_loop(g, s):
    NS.encounter_closes_the_loop(g, WHITE, s)


# ---- 5: a network of zeros ignores its input -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", CAMPAIGN_SHAPES[:3], ids=[MS.shape_id(s) for s in CAMPAIGN_SHAPES[:3]])
def test_sensor_noise_alone_leaves_the_zero_policy_alone(g, s):
    sensors = g.policy.Disturbance.normalised(sep=0.3, cpa=0.5, closing=0.2, action=0.0, seed=21)
    got = MS.campaign(g, s, disturbance=sensors).run(MS.EPISODES).accumulators()
    plain = MS.reference(g, s)
    same(g, {k: v[[2]] for k, v in got.items()}, {k: v[[2]] for k, v in plain.items()})
    assert MS.mismatches(g, {k: v[[0]] for k, v in got.items()}, {k: v[[0]] for k, v in plain.items()})   # a real network does see it


# ---- 6: refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals(g):
    D = g.policy.Disturbance
    s = MS.Shape(F32, True, 1, False, 1000)
    for bad in (D.normalised(sep=-0.1), D.normalised(cpa=float("nan")), D.normalised(closing=float("inf")), D.normalised(action=-1.0)):
        mc = MS.campaign(g, s, disturbance=bad)
        with pytest.raises(RuntimeError, match=r"acas2d_monte_carlo_disturbed: s_sep = .* \(each finite and at least 0\)"):
            mc.run(1)
        assert mc.first_episode == 0 and mc.accumulators()["outcome_count"].sum() == 0      # a refusal leaves the campaign alone
        with pytest.raises(RuntimeError, match=r"acas2d_evaluate_policies_disturbed: s_sep = .* \(each finite and at least 0\)"):
            fused(g, 1, False, disturbance=bad)
    with pytest.raises(RuntimeError, match=r"acas2d_monte_carlo_disturbed: episodes_per_lane = 0 \(at least 1\)"):
        NS.campaign(g, WHITE, s).run(0)
    long = g.ACAS2DConfig(n_traffic=1, max_steps=(1 << 20) - 1)
    with pytest.raises(RuntimeError, match="acas2d_monte_carlo_disturbed: max_steps = 1048575 .*the step field of the noise counter"):
        g.MonteCarlo([MS.zero_policy(1)], MS.LANES, config=long, disturbance=the_disturbance(g), device=DEV).run(1)
    eps = ES.episodes(ES.config(g, 1))
    with pytest.raises(RuntimeError, match="acas2d_evaluate_policies_disturbed: max_steps = 1048575 "):
        g.evaluate_policies_fused([MS.zero_policy(1)], eps.own, eps.trf, eps.goal, dtype=F32, device=DEV, config=long,
                                  max_steps=120, disturbance=the_disturbance(g))
    with pytest.raises(ValueError, match="float32 only"):
        g.MonteCarlo([MS.zero_policy(1)], MS.LANES, dtype=torch.float64, disturbance=the_disturbance(g), device=DEV)
    with pytest.raises(ValueError, match="float32 only"):
        g.evaluate_policies_fused([MS.zero_policy(1)], eps.own, eps.trf, eps.goal, dtype=torch.float64, device=DEV,
                                  disturbance=the_disturbance(g))
    with pytest.raises(RuntimeError, match="acas2d_monte_carlo_disturbed_group: n_traffic = 3 takes the thread-per-env shape C=3 G=1: "
                                           "use acas2d_monte_carlo_disturbed_f32"):
        g.MonteCarlo([MS.zero_policy(3)], MS.LANES, group=True, n_traffic=3, disturbance=the_disturbance(g), device=DEV).run(1)
    with pytest.raises(RuntimeError, match="acas2d_monte_carlo_disturbed: n_traffic = 16 has no thread-per-env shape"):
        g.MonteCarlo([MS.zero_policy(16)], MS.LANES, n_traffic=16, disturbance=the_disturbance(g), device=DEV).run(1)
    with pytest.raises(RuntimeError, match=r"acas2d_disturbance_draw: n_slots = 66 \(at most 65"):
        g.policy.disturbance_draw(7, 0, 4, 0, 0, 4, 66, device=DEV)
    with pytest.raises(RuntimeError, match="acas2d_disturbance_draw: first_step = 1048575 \\+ n_steps = 2 exceeds the step field"):
        g.policy.disturbance_draw(7, 0, 4, 0, (1 << 20) - 1, 2, 2, device=DEV)
