"""Shared by tests/test_disturbance.py and tests/test_correlated.py: the shapes, the host loop the noisy evaluators are held
to, the campaign's reference and the properties a campaign is used for -- once each, for every error model.

A Flavour names an error model and builds its test disturbance; the cached helpers are keyed by its name.  WHITE and
CORRELATED have the same sigmas, so the white campaign is the correlated one's at every rho 0 and both files share its run;
SATURATING and SATURATING_CORRELATED are their twins under sigmas of two box widths, where the clamps decide every step.

References (no new arithmetic, no tolerance):
  evaluator  host_loop(): per step the observation of a latching env, records.disturb_observation() with the errors of the
             draw entry's normals, the project's in-kernel network through a one-step rollout_policy() on a scratch env,
             records.disturb_action(), the latching step with record_trace=True, and records.episode_safety() on the trace;
  campaign   monte_carlo_support.per_counter() under the flavour's disturbance -- reset_to_episode(c) + the noisy evaluator
             with noise_episode = c -- folded by records.monte_carlo_reduce().
One of each per (flavour, shape), computed once and left unchanged."""
from collections import namedtuple

import numpy as np
import pytest
import torch

import edge_observations as EO
import eval_stats_support as ES
import monte_carlo_support as MS

DEV = ES.DEV
F32 = torch.float32
# (n_traffic, group)
# all nine compiled work shapes (C, G): (1,1) (3,1) (8,1) (4,4) (4,16) (2,1) (4,1) (4,2) (4,8)
EVAL_SHAPES = ((1, False), (3, False), (8, False), (16, True), (64, True), (2, False), (4, False), (8, True), (32, True))
CAMPAIGN_SHAPES = [MS.Shape(F32, True, n, grp, max_steps) for max_steps in (1000, 150) for n, grp in ((1, False), (8, False), (16, True))]
# the other six work shapes, for the equality with the evaluator alone, under the short config
CAMPAIGN_MORE = [MS.Shape(F32, True, n, grp, 150) for n, grp in ((2, False), (3, False), (4, False), (8, True), (32, True), (64, True))]
NOISE_EPISODE = 5
SIGMAS = dict(sep=0.05, cpa=0.1, closing=0.1, action=0.3, seed=7)
# most of what the actor reads lies at an end of its box, and most of what is flown is +-1: the clamps decide every step
SATURATING_SIGMAS = dict(sep=2.0, cpa=4.0, closing=4.0, action=4.0, seed=7)
SATURATING_EVAL_SHAPES = ((3, False), (16, True))
SATURATING_CAMPAIGN_SHAPE = MS.Shape(F32, True, 8, False, 150)
RHO = dict(rho_sep=0.9, rho_cpa=1.0, rho_closing=0.0, rho_action=0.5)


def rho_of_slots(dist, N):
    """[N + 1, 3]: the coefficient of every value of a lane's draw -- slot 0 the actuator's normal (and two zeros), slot n + 1
    traffic n's three channels."""
    return np.asarray([[dist.rho_action, 0.0, 0.0]] + [list(dist.rho)] * N, np.float32)


def correlated_series(g, dist, N):
    """The host loop's series under `dist`: the errors the normals drive, scanned from the episode's first step
    (game.steps == 1) on."""
    return lambda normals: np.concatenate([normals[:1], g.records.correlated_errors(normals[1:], rho_of_slots(dist, N))])


# disturbance(g): the flavour's one test disturbance; errors(g, dist, N): host_loop()'s `errors` under it, or None
Flavour = namedtuple("Flavour", "name disturbance errors", defaults=(None,))
WHITE = Flavour("white", lambda g: g.Disturbance.normalised(**SIGMAS))
CORRELATED = Flavour("correlated", lambda g: g.CorrelatedDisturbance.normalised(**SIGMAS, **RHO), correlated_series)
SATURATING = Flavour("saturating", lambda g: g.Disturbance.normalised(**SATURATING_SIGMAS))
SATURATING_CORRELATED = Flavour("saturating-correlated", lambda g: g.CorrelatedDisturbance.normalised(**SATURATING_SIGMAS, **RHO),
                                correlated_series)


def reseeded(dist, seed):
    """`dist` under another noise seed."""
    return type(dist).from_dict(dict(dist.to_dict(), seed=seed))


def at_wide_seed(fl):
    """The flavour under monte_carlo_support.WIDE_SEED (both halves of the noise key non-zero and distinct)."""
    return Flavour(fl.name + "@wide-seed", lambda g: reseeded(fl.disturbance(g), MS.WIDE_SEED), fl.errors)


# the noisy evaluators' wide keys: the noise lane crosses 2^32 at episode 37 of the 70 (monte_carlo_support.WIDE_LANE_OFFSET),
# the seed is WIDE_SEED and the counter the last one
WIDE_NOISE_EPISODE = 2 ** 32 - 1
WIDE_EVAL = dict(env_offset=MS.WIDE_LANE_OFFSET, seed=MS.WIDE_SEED, noise_episode=WIDE_NOISE_EPISODE)
WIDE_EVAL_SHAPES = ((1, False), (8, False), (16, True))
WIDE_CAMPAIGN_SHAPES = [MS.Shape(F32, True, n, grp, 150) for n, grp in ((1, False), (16, True))]


def shape_id(s):
    return "N%d%s" % (s[0], "-group" if s[1] else "")


EVAL_IDS = [shape_id(s) for s in EVAL_SHAPES]
CAMPAIGN = pytest.mark.parametrize("s", CAMPAIGN_SHAPES, ids=[MS.shape_id(s) for s in CAMPAIGN_SHAPES])
WIDE_EVAL_PARAMS = pytest.mark.parametrize("shape", WIDE_EVAL_SHAPES, ids=[shape_id(s) for s in WIDE_EVAL_SHAPES])
WIDE_CAMPAIGN = pytest.mark.parametrize("s", WIDE_CAMPAIGN_SHAPES, ids=[MS.shape_id(s) for s in WIDE_CAMPAIGN_SHAPES])
CAMPAIGN_EVERY_SHAPE = pytest.mark.parametrize("s", CAMPAIGN_SHAPES + CAMPAIGN_MORE,
                                               ids=[MS.shape_id(s) for s in CAMPAIGN_SHAPES + CAMPAIGN_MORE])
SATURATING_EVAL = pytest.mark.parametrize("shape", SATURATING_EVAL_SHAPES, ids=[shape_id(s) for s in SATURATING_EVAL_SHAPES])


def fused(g, N, group, **kw):
    cfg = ES.config(g, N)
    eps = ES.episodes(cfg)
    return g.evaluate_policies_fused(ES.two_policies(g, N), eps.own, eps.trf, eps.goal, dtype=F32, device=DEV, config=cfg,
                                     group=group, safety=True, **kw)


def same(g, got, want):
    bad = MS.mismatches(g, got, want)
    assert not bad, {k: (np.asarray(got[k]).ravel()[:6], np.asarray(want[k]).ravel()[:6]) for k in bad}


# ---- the evaluator against a host loop -------------------------------------------------------------------------------------------------
def host_loop(g, cfg, eps, policy, dist, noise_episode, group, errors=None, seen=None, env_offset=0):
    """One policy's reference rows [E] by the per-step path: (outcome, steps, total_reward, stats dict, summary dict).
    Episode i reads the noise of lane env_offset + i.
    `errors`: from the drawn normals [step, lane, slot, 3] to the series the loop indexes; None: the normals themselves,
    the white model.  `seen`: a list that takes, per step, (the rows the actor read, the actions flown) of the envs still
    playing."""
    E, N = ES.E, cfg.n_traffic
    n_steps = cfg.max_steps + 1
    zero = np.zeros(E, np.int32)
    # the normals of every step an episode can reach, from the draw entry: [step, lane, slot, 3] -- and the errors they drive
    normals = g.policy.disturbance_draw(dist.seed, env_offset, E, noise_episode, 0, cfg.max_steps + 2, N + 1, device=DEV)
    series = normals if errors is None else errors(normals)
    r = g.ACAS2DVecEnv(E, N, device=DEV, dtype=F32, auto_reset=False, record_trace=True, config=cfg)
    r.set_state(eps.own, eps.trf, eps.goal, zero, observe=True)
    scratch = g.ACAS2DVecEnv(E, N, device=DEV, dtype=F32, auto_reset=True, config=cfg)
    scratch.reset()
    cols = [r.trace.clone()]
    active = np.ones(E, bool)
    outcome, steps, ret, t0 = np.zeros(E, np.uint8), np.zeros(E, np.int32), np.zeros(E, np.float32), np.zeros(E, np.int64)
    lane = np.arange(E)
    assert (r.steps.cpu().numpy() == 1).all()                          # every episode starts at game.steps == 1
    for t in range(n_steps):
        obs = r.outputs["obs"].cpu().numpy()
        at = r.steps.cpu().numpy()                                     # game.steps before this step
        z = series[np.minimum(at, series.shape[0] - 1), lane]         # [E, N + 1, 3] (latched envs: unused)
        noisy = g.records.disturb_observation(obs, dist.sigma, z[:, 1:])
        scratch.outputs["obs"].copy_(torch.as_tensor(noisy, device=DEV))
        action = scratch.rollout_policy(policy, 1, group=group)["actions"][0].cpu().numpy()
        flown = g.records.disturb_action(action, dist.s_action, z[:, 0, 0])
        if seen is not None:
            seen.append((noisy[active], flown[active]))
        _, _, done, infos = r.step(torch.as_tensor(flown, device=DEV))
        cols.append(r.trace.clone())
        fin = active & done.cpu().numpy()
        outcome[fin] = infos.outcome.cpu().numpy()[fin]
        steps[fin] = r.steps.cpu().numpy()[fin]
        ret[fin] = r.total_reward.cpu().numpy()[fin]
        t0[fin] = t
        active &= ~fin
        if not active.any():
            break
    trace = torch.stack(cols).cpu().numpy()
    names = list(g.vec_env.TRACE_COLUMNS)
    c_sep, c_lat, c_dev = names.index("d_sep"), names.index("a_lat"), names.index("d_dev")
    keys = ("min_sep", "min_sep_step", "los_steps", "max_a_lat", "max_dev", "sum_dev")
    stats = {k: np.zeros(E, np.int32 if k in ("min_sep_step", "los_steps") else np.float32) for k in keys}
    summary = {k: np.zeros(E, np.int32 if k in ("min_separation_step", "los_steps") else np.float32) for k in g.records.SAFETY_KEYS}
    for i in np.nonzero(~active)[0]:
        n = t0[i] + 2
        assert n == steps[i]
        one = g.records.episode_safety(trace[:n, i, c_sep], trace[:n, i, c_lat], trace[:n, i, c_dev], cfg.safe_distance, np.float32)
        for k in keys:
            stats[k][i] = one[k]
        for k, val in g.records.safety_summary(one, int(steps[i])).items():
            summary[k][i] = val
    return outcome, steps, ret, stats, summary


_LOOP, _RAN, _SEEN = {}, {}, {}


def disturbance_of(g, fl, seed=None):
    """The flavour's disturbance, under its own seed or `seed`."""
    return fl.disturbance(g) if seed is None else reseeded(fl.disturbance(g), seed)


def loop_reference(g, fl, N, group, env_offset=0, seed=None, noise_episode=NOISE_EPISODE):
    """host_loop()'s rows of eval_stats_support's two policies under the flavour's disturbance at NOISE_EPISODE -- or at the
    keys given: the first noise lane, the noise seed, the counter."""
    key = (fl.name, N, group) + (() if (env_offset, seed, noise_episode) == (0, None, NOISE_EPISODE) else (env_offset, seed, noise_episode))
    if key not in _LOOP:
        cfg = ES.config(g, N)
        eps = ES.episodes(cfg)
        dist = disturbance_of(g, fl, seed)
        errors = fl.errors and fl.errors(g, dist, N)
        seen = _SEEN[key] = []
        _LOOP[key] = [host_loop(g, cfg, eps, pol, dist, noise_episode, group, errors, seen, env_offset) for pol in ES.two_policies(g, N)]
    return _LOOP[key]


def loop_seen(g, fl, N, group):
    """(rows read [n, 5 + 3 N], actions flown [n]) over every step either policy played in loop_reference()."""
    loop_reference(g, fl, N, group)
    seen = _SEEN[fl.name, N, group]
    return np.concatenate([s[0] for s in seen]), np.concatenate([s[1] for s in seen])


def saturating_evaluator_equals_the_host_loop(g, fl, shape):
    """Under the saturating sigmas -- asserted first, on the reference alone: every episode finished and the clamps decide
    (edge_observations.check_saturated).  Every episode flies a +-1 at some step, so max_abs_a_lat is the limit under every
    noise counter: the counter shows in the mean deviation, which the whole flown path makes."""
    N, group = shape
    limit = np.float32(ES.config(g, N).to_c().acc_lat_limit)
    for row in loop_reference(g, fl, N, group):
        assert (row[0] != 0).all(), "an episode of the reference did not finish"
        assert (row[4]["max_abs_a_lat"] == limit).all()
    EO.check_saturated(*loop_seen(g, fl, N, group), g.records.OBSERVATION_BOX)
    evaluator_equals_the_host_loop(g, fl, shape, counter_shows_in="mean_abs_deviation")


def evaluator_equals_the_host_loop(g, fl, shape, counter_shows_in="max_abs_a_lat", env_offset=0, seed=None, noise_episode=NOISE_EPISODE):
    """The fused evaluator's rows against loop_reference()'s, bit for bit; another noise counter gives another
    `counter_shows_in`."""
    N, group = shape
    dist = disturbance_of(g, fl, seed)
    got = fused(g, N, group, disturbance=dist, noise_episode=noise_episode, env_offset=env_offset)
    for k, (outcome, steps, ret, stats, summary) in enumerate(loop_reference(g, fl, N, group, env_offset, seed, noise_episode)):
        assert np.array_equal(got["outcome"][k], outcome) and np.array_equal(got["steps"][k], steps), k
        assert ES.bits_equal(got["total_reward"][k].astype(np.float32), ret), k
        for key in g.records.SAFETY_KEYS:
            assert ES.bits_equal(got[key][k], summary[key]), (k, key)
    # the counter is part of the noise
    other = fused(g, N, group, disturbance=dist, noise_episode=(noise_episode + 1) % 2 ** 32, env_offset=env_offset)
    assert not ES.bits_equal(other[counter_shows_in], got[counter_shows_in])


def evaluator_at_wide_keys(g, fl, shape):
    """The evaluator against the host loop at WIDE_EVAL.  Teeth first, on the reference alone: against the host loop at the
    default keys a float statistic moves in at least half of the episodes, on both sides of the crossing."""
    N, group = shape
    floats = [k for k in g.records.SAFETY_KEYS if k not in ("min_separation_step", "los_steps")]
    for k, (wide, plain) in enumerate(zip(loop_reference(g, fl, N, group, **WIDE_EVAL), loop_reference(g, fl, N, group))):
        assert (wide[0] != 0).all(), "an episode of the reference did not finish"
        moved = np.zeros(ES.E, bool)
        for key in floats:
            moved |= ES.bits(wide[4][key]) != ES.bits(plain[4][key])
        assert 2 * int(moved.sum()) >= ES.E and moved[:MS.WIDE_CROSSING].any() and moved[MS.WIDE_CROSSING:].any(), (k, int(moved.sum()))
    evaluator_equals_the_host_loop(g, fl, shape, **WIDE_EVAL)


# ---- the campaign against the evaluator ------------------------------------------------------------------------------------------------
def per_counter(g, fl, s):
    """The flavour's evaluator's result dicts of [a, b, zero] for counters 0 .. EPISODES - 1 at shape s."""
    return MS.per_counter(g, s, fl)


def reference(g, fl, s, rows=None):
    return MS.reference(g, s, rows=rows, fl=fl)


def campaign_at_wide_keys(g, fl, s):
    """monte_carlo_support.campaign_at_wide_keys() under the flavour at WIDE_SEED: the campaign's seed is the noise seed too.
    The campaign and its reference, the noisy evaluator, form the noise lane with the same code, so the reference is anchored
    first: policy a's row of the last counter, 2^32 - 1, against host_loop() on the encounters drawn for it, whose normals
    come from the draw entry at the 64-bit lanes."""
    wide, last = at_wide_seed(fl), 2 ** 32 - 1
    cfg, dist = MS.config(g, s), at_wide_seed(fl).disturbance(g)
    v = g.ACAS2DVecEnv(MS.LANES, s.N, device=DEV, dtype=F32, seed=MS.WIDE_SEED, env_offset=MS.WIDE_LANE_OFFSET, config=cfg)
    v.reset_to_episode(last)
    assert MS.LANES == ES.E                                       # host_loop() plays eval_stats_support's number of episodes
    outcome, steps, ret, _, summary = host_loop(g, cfg, ES.Episodes(*g.policy.read_state(v), None), MS.policies(g, s)[0], dist, last,
                                                s.group, wide.errors and wide.errors(g, dist, s.N), env_offset=MS.WIDE_LANE_OFFSET)
    res = MS.per_counter(g, s, wide, **MS.WIDE)[-1]
    assert (outcome != 0).all() and np.array_equal(res["outcome"][0], outcome) and np.array_equal(res["steps"][0], steps)
    assert ES.bits_equal(res["total_reward"][0].astype(np.float32), ret)
    for key in g.records.SAFETY_KEYS:
        assert ES.bits_equal(res[key][0], summary[key]), key
    MS.campaign_at_wide_keys(g, s, fl=wide, default=fl)


def campaign(g, fl, s, **kw):
    return MS.campaign(g, s, disturbance=fl.disturbance(g), **kw)


def ran(g, fl, s):
    """The accumulators of the flavour's campaign after EPISODES episodes in one launch."""
    if (fl.name, s) not in _RAN:
        acc = campaign(g, fl, s).run(MS.EPISODES).accumulators()
        for a in acc.values():
            a.setflags(write=False)
        _RAN[fl.name, s] = acc
    return _RAN[fl.name, s]


# ---- the properties a campaign is used for ----------------------------------------------------------------------------------------------
def chaining(g, fl, s):
    same(g, campaign(g, fl, s).run(2).run(1).accumulators(), ran(g, fl, s))
    same(g, campaign(g, fl, s).run(MS.EPISODES, per_launch=1).accumulators(), ran(g, fl, s))      # (ran: per_launch >= EPISODES)


def survives_a_state_dict(g, fl, s, others, foreign, fields=None):
    """... and another disturbance is another campaign: a campaign under any of `others` (None: undisturbed) refuses the
    state, and this one refuses the state of a campaign under `foreign`.  `fields`: what the state's disturbance must say
    beyond to_dict(), as float32."""
    first = campaign(g, fl, s).run(2)
    sd = first.state_dict()
    assert sd["first_episode"] == 2 and sd["disturbance"] == fl.disturbance(g).to_dict()
    assert all(sd["disturbance"][k] == np.float32(v) for k, v in (fields or {}).items())
    second = campaign(g, fl, s).load_state_dict(sd).run(1)
    assert second.first_episode == 3
    same(g, second.accumulators(), ran(g, fl, s))
    for other in others:
        with pytest.raises(ValueError, match="disturbance"):
            MS.campaign(g, s, disturbance=other).load_state_dict(sd)
    with pytest.raises(ValueError, match="disturbance"):
        campaign(g, fl, s).load_state_dict(MS.campaign(g, s, disturbance=foreign).state_dict())


def common_random_numbers(g, fl, s):
    """Policy b alone meets the encounters AND the errors it meets among [a, b, zero]."""
    b = MS.policies(g, s)[1]
    alone = campaign(g, fl, s, pols=[b]).run(MS.EPISODES).accumulators()
    same(g, alone, {k: v[[1]] for k, v in ran(g, fl, s).items()})


def encounter_closes_the_loop(g, fl, s):
    mc = campaign(g, fl, s).run(MS.EPISODES)
    acc = ran(g, fl, s)
    assert mc.summary()["disturbance"] == fl.disturbance(g).to_dict()
    for k, top in enumerate(mc.worst(1)):
        (lane, counter, sep), = top
        assert sep == acc["lane_worst_sep"][k].min() and counter == acc["lane_worst_episode"][k, lane]
        own, trf, goal, replay = mc.encounter(lane, counter)
        assert replay == {"disturbance": fl.disturbance(g), "noise_episode": counter, "env_offset": lane}
        res = g.evaluate_policies_fused(MS.policies(g, s), own, trf, goal, dtype=F32, device=DEV, config=MS.config(g, s),
                                        group=s.group, safety=True, **replay)
        assert ES.bits_equal(res["min_separation"][k, :1], np.asarray([sep], np.float32))
