"""The collectors under time-correlated and biased errors on the GPU (acas2d_collect_set_correlated_f32 / _group_f32;
ACAS2DVecEnv.collect(disturbance=) / collect_set(disturbances=) with a policy.CorrelatedDisturbanceSet, the trainers):

  1  every rho 0: the white disturbed collector's bits, and the held state stays zero;
  2  correlated, against the white collector's host loop (test_collect_disturbed.host_loop) with the errors in the normals' place:
     per-env held arrays advanced by records.correlated_step() with first = (steps == 1) -- no other new arithmetic; the final
     held state too -- also under sigmas of two box widths, and (2b) on test_collect_disturbed's injected rows in two
     consecutive one-step launches, the second of which reads the state: what is held is the error, not the clamped entry;
  3  one launch of 16 steps is two of 8 and sixteen of 1: a launch boundary is no episode boundary, and the extra pass for
     obs_read[T] commits nothing;
  4  member k of two with different rho is the one-member launch on its envs; a white member beside a correlated one is the
     white collector;  5  thread-per-env and group shape agree at eight aircraft;
  6  gae_fused on obs_read[T] returns the bits of the next collection's values[0];
  7  rho_action = 1, no sensor noise, an actor that returns 0 without spread: within an episode every step flies the same
     action disturb_action(0, s, z_1) -- the per-step env that is sent it returns the launch's rows and ends in its state, and
     its a_lat (a latching env's trace) is one value per episode;
  8  the trainers: a rho-0 set trains the white run's bits, a correlated run repeats itself, a PBT exploit step leaves the
     members' coefficients and the held state where they were, and the set goes through a trainer's state_dict().

The shapes, the policies, the env and the white references are test_collect_disturbed's: 70 envs for one member (two waves
thread per env, one of them partial), 2 x 64 for two, 16 steps, max_steps = 5 -- every env is reset three times inside a
launch, and episodes straddle every cut.  The test disturbance has the white one's sigmas with rho 0.9 / 1 / 0 / 0.5 on
sep / cpa / closing / action."""
import json

import numpy as np
import pytest
import torch

import edge_observations as EO
import eval_stats_support as ES
import test_collect_disturbed as CD

pytestmark = pytest.mark.gpu
DEV, F32 = ES.DEV, torch.float32
T, E1, EM = CD.T, CD.E1, CD.EM
NOISE_SEED, NOISE_STEP = CD.NOISE_SEED, CD.NOISE_STEP
RHO = dict(rho_sep=0.9, rho_cpa=1.0, rho_closing=0.0, rho_action=0.5)
SIGMAS = dict(sep=0.05, cpa=0.1, closing=0.1, action=0.3, seed=7)          # test_collect_disturbed.noisy()'s


@pytest.fixture(scope="module")
def g():
    import gym_acas2d_amd as g
    return g


def corr(g, **kw):
    return g.CorrelatedDisturbance.normalised(**{**SIGMAS, **RHO, **kw})


_RUNS = {}


def csolo(g, N, group, dist, E=E1, offset=0, seed=1, key=NOISE_SEED, cuts=(T,), episodes=False):
    """collect() of `cuts` steps in a row on a fresh env under a fresh one-member CorrelatedDisturbanceSet of `dist`: one
    host dict per piece (test_collect_disturbed.host's, plus "held": the state after the piece).  Cached, left alone."""
    name = (N, group, dist, E, offset, seed, key, cuts) + ((episodes,) if episodes else ())
    if name not in _RUNS:
        env, pol = CD.make_env(g, E, N, offset, episodes), CD.policy(g, N, seed)
        ds = g.CorrelatedDisturbanceSet(dist, 1)
        outs, at = [], NOISE_STEP
        for n in cuts:
            d = CD.host(env.collect(pol, n, noise_seed=key, noise_step=at, group=group, disturbance=ds), env)
            d["held"] = ds.held_numpy()
            outs.append(d)
            at += n
        assert ds.held.shape == (3 * N + 1, E)
        _RUNS[name] = outs[0] if len(cuts) == 1 else outs
    return _RUNS[name]


def cpair(g, N, group, dists):
    """collect_set() of two members (policies 1 and 2, keys 21 and 22) on 2 x 64 envs under a two-member set."""
    name = ("pair", N, group, tuple(dists))
    if name not in _RUNS:
        env = CD.make_env(g, 2 * EM, N)
        pset = g.ActorCriticSet.from_members([CD.policy(g, N, 1), CD.policy(g, N, 2)], device=DEV)
        ds = g.CorrelatedDisturbanceSet(list(dists), 2)
        d = CD.host(env.collect_set(pset, T, [NOISE_SEED, NOISE_SEED + 1], noise_step=NOISE_STEP, group=group, disturbances=ds), env)
        d["held"] = ds.held_numpy()
        _RUNS[name] = d
    return _RUNS[name]


ALL = ("obs_read",) + CD.KEYS + tuple("state." + n for n in CD.STATE)


# ---- 1: every rho 0 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", CD.ALL_SHAPES, ids=[CD.shape_id(s) for s in CD.ALL_SHAPES])
def test_zero_rho_is_the_white_collector(g, shape):
    N, group = shape
    white = CD.solo(g, N, group, "noisy")
    CD.every_env_was_reset(white, E1)
    for dist in (corr(g, rho_sep=0.0, rho_cpa=0.0, rho_closing=0.0, rho_action=0.0), CD.noisy(g)):     # rho 0 by name; a Disturbance
        got = csolo(g, N, group, dist)
        assert set(got) == set(white) | {"held"}
        for k in ALL:
            assert ES.bits_equal(got[k], white[k]), k
        assert got["held"].shape == (3 * N + 1, E1) and not ES.bits(got["held"]).any()       # +0.0 everywhere: never written


# ---- 2: against the host loop -----------------------------------------------------------------------------------------------------
class Errors:
    """test_collect_disturbed.normals_for() with the errors in the normals' place: per-env held arrays advanced by
    records.correlated_step(), first = (steps == 1).  A channel with rho 0 or with nothing drawn keeps its held value; the
    call for the row past the last step (`commits` calls were before it) forms its errors and commits nothing."""

    def __init__(self, g, dist, E, N, commits):
        self.g, self.dist, self.commits, self.calls = g, dist, commits, 0
        self.rho = np.asarray(dist.rho, np.float32)
        self.held_s, self.held_a = np.zeros((E, N, 3), np.float32), np.zeros(E, np.float32)
        self.white, self.steps = [], []

    def __call__(self, g, seed, offset, episode, steps, N):
        R, d = g.records, self.dist
        z = CD_NORMALS(g, seed, offset, episode, steps, N)
        self.white.append(z.copy())
        self.steps.append(steps.copy())
        first = steps == 1
        out = z.copy()
        commit = self.calls < self.commits
        self.calls += 1
        if d.s_sep != 0 or d.s_cpa != 0 or d.s_closing != 0:
            e = R.correlated_step(self.held_s, z[:, 1:], self.rho, first[:, None, None])
            out[:, 1:] = e
            if commit:
                self.held_s = np.where(self.rho == 0, self.held_s, e)
        if d.s_action != 0:
            e = R.correlated_step(self.held_a, z[:, 0, 0], np.float32(d.rho_action), first)
            out[:, 0, 0] = e
            if commit and d.rho_action != 0:
                self.held_a = e
        return out

    def held(self):
        E, N, _ = self.held_s.shape
        return np.concatenate([self.held_s.reshape(E, 3 * N).T, self.held_a[None]]).astype(np.float32)


CD_NORMALS = CD.normals_for


def correlated_host_loop(g, monkeypatch, N, group, dist, **keys):
    err = Errors(g, dist, E1, N, T)
    monkeypatch.setattr(CD, "normals_for", err)
    ref = CD.host_loop(g, N, group, dist, **keys)
    monkeypatch.undo()
    assert err.calls == T + 1
    ref["held"] = err.held()
    return ref, err


def held_rows_of(N):
    """Which rows of the final held state are not all +0.0 under RHO: rho_closing = 0 holds nothing."""
    return [True, True, False] * N + [True]


@pytest.mark.parametrize("shape", CD.LOOP_SHAPES, ids=[CD.shape_id(s) for s in CD.LOOP_SHAPES])
def test_correlated_collector_equals_the_host_loop(g, monkeypatch, shape):
    N, group = shape
    dist = corr(g)
    ref, err = correlated_host_loop(g, monkeypatch, N, group, dist)
    # teeth, on the reference alone: every env was reset inside the launch, and the rows read differ from the white model's
    # rows of the same true observations at more than half of the (t, env) whose steps > 1 -- a kernel that ignores the state
    # cannot pass
    CD.every_env_was_reset(ref, E1)
    later = np.stack(err.steps) > 1                                                   # [T + 1, E]
    white_rows = np.stack([g.records.disturb_observation(ref["obs"][t], dist.sigma, err.white[t][:, 1:]) for t in range(T + 1)])
    moved = (ES.bits(white_rows) != ES.bits(ref["obs_read"])).any(-1)
    assert int(later.sum()) >= E1 and 2 * int((moved & later).sum()) > int(later.sum()), (int(moved.sum()), int(later.sum()))
    assert not moved[~later].any()                                                    # an episode's first step: z itself
    assert ES.bits(ref["held"]).any(1).tolist() == held_rows_of(N)                    # rho_closing = 0 holds nothing
    got = csolo(g, N, group, dist)
    for k in ALL + ("held",):
        assert ES.bits_equal(got[k], ref[k]), k
    # ... which the white collector does not give
    assert not ES.bits_equal(got["obs_read"], CD.solo(g, N, group, "noisy")["obs_read"])


@pytest.mark.parametrize("shape", CD.WIDE_SHAPES, ids=[CD.shape_id(s) for s in CD.WIDE_SHAPES])
def test_correlated_collector_equals_the_host_loop_at_wide_keys(g, monkeypatch, shape):
    """test_collect_disturbed's wide keys -- the global env index crossing 2^32 at env 37, the noise seed helpers.WIDE_SEED,
    the even envs' counters preset to 2^32 - 2 -- in one launch of 16 steps and in two of 8: at the cut the preset envs play
    the episode 2^32 - 1, so the held state crosses a launch inside the episode after which the counter wraps."""
    N, group = shape
    dist = corr(g, seed=CD.MS.WIDE_SEED)
    ref, err = correlated_host_loop(g, monkeypatch, N, group, dist, **CD.WIDE)
    CD.preset_counters_wrapped(ref, E1)
    assert ES.bits(ref["held"]).any(1).tolist() == held_rows_of(N)
    assert ES.bits(ref["held"])[:, :CD.MS.WIDE_CROSSING].any() and ES.bits(ref["held"])[:, CD.MS.WIDE_CROSSING:].any()
    got = csolo(g, N, group, dist, **CD.WIDE)
    for k in ALL + ("held",):
        assert ES.bits_equal(got[k], ref[k]), k
    h = T // 2
    first, second = csolo(g, N, group, dist, cuts=(h, h), **CD.WIDE)
    pre = CD.H.wide_preset(E1)
    top = pre & (first["state.episode"].view(np.uint32) == 2 ** 32 - 1) & (first["state.steps"] > 1)
    assert top.any()                                                      # mid-episode at the last counter, with state to carry
    assert ES.bits(first["held"])[:, top].any(0).all()
    for k in CD.KEYS[1:]:
        assert ES.bits_equal(np.concatenate([first[k], second[k]]), ref[k]), k
    assert ES.bits_equal(first["obs"], ref["obs"][:h + 1]) and ES.bits_equal(second["obs"], ref["obs"][h:])
    assert ES.bits_equal(first["obs_read"], ref["obs_read"][:h + 1]) and ES.bits_equal(second["obs_read"], ref["obs_read"][h:])
    for k in tuple("state." + n for n in CD.STATE) + ("held",):
        assert ES.bits_equal(second[k], ref[k]), k


@pytest.mark.parametrize("shape", CD.SATURATING_SHAPES, ids=[CD.shape_id(s) for s in CD.SATURATING_SHAPES])
def test_saturating_correlated_collector_equals_the_host_loop(g, monkeypatch, shape):
    """Sigmas of two box widths: the clamps decide most entries and most actions, and the state is the error, not the entry."""
    N, group = shape
    dist = corr(g, **EO.SATURATING)
    ref, err = correlated_host_loop(g, monkeypatch, N, group, dist)
    CD.every_env_was_reset(ref, E1)
    EO.check_saturated(ref["obs_read"], ref["flown"], g.records.OBSERVATION_BOX)      # teeth, on the reference alone
    assert ES.bits(ref["held"]).any(1).tolist() == held_rows_of(N)
    got = csolo(g, N, group, dist)
    for k in ALL + ("held",):
        assert ES.bits_equal(got[k], ref[k]), k


# ---- 2b: hand-placed entries in the row the launch reads ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", CD.INJECTED, ids=[CD.injected_id(c) for c in CD.INJECTED])
def test_injected_rows_meet_the_reference(g, case):
    """test_collect_disturbed's injected rows through a CorrelatedDisturbanceSet with RHO, in two consecutive one-step
    collections, each with a freshly injected row: the second reads the held state.  The state is compared after each."""
    (N, group), name = case
    dist = corr(g, **EO.DISTURBANCES[name])
    ds = g.CorrelatedDisturbanceSet(dist, 1)
    err = Errors(g, dist, E1, N, 2)
    CD.injected_rows_meet_the_reference(g, (N, group), dist, launches=2, draw=err, dset=ds, vanishing=name == "vanishing",
                                        held=lambda: (ds.held_numpy(), err.held()))
    # (an env the first step finished -- a fresh draw can start inside a collision -- starts afresh, steps == 1 again: the
    #  others, at least a tenth of the envs, read the state)
    assert err.calls == 2 and (err.steps[0] == 1).all() and set(err.steps[1].tolist()) <= {1, 2}
    assert 10 * int((err.steps[1] == 2).sum()) >= E1
    sensors, held = any(dist.sigma), err.held()
    assert ES.bits(held).any(1).tolist() == [sensors, sensors, False] * N + [dist.s_action != 0]
    if name == "saturating":
        # what is held is the unclamped error e_t, not what the clamp left of the entry
        assert 10 * int((np.abs(held[:-1]) > 1).sum()) >= held[:-1].size


# ---- 3: cuts ------------------------------------------------------------------------------------------------------------------------
# (the pieces of one step also at (4,1) and at (4,8): eight envs per wave there, so the last wave of the 70 holds six -- lanes
#  past the last env neither load nor store held state)
CUTS = [(2, (3, False)), (2, (16, True)), (16, (3, False)), (16, (16, True)), (16, (4, False)), (16, (32, True))]


@pytest.mark.parametrize("pieces,shape", CUTS, ids=["%d-%s" % (p, CD.shape_id(s)) for p, s in CUTS])
def test_one_launch_is_its_pieces(g, shape, pieces):
    N, group = shape
    whole = csolo(g, N, group, corr(g))
    n = T // pieces
    parts = csolo(g, N, group, corr(g), cuts=(n,) * pieces)
    for k in CD.KEYS[1:]:
        assert ES.bits_equal(np.concatenate([p[k] for p in parts]), whole[k]), k
    for i, p in enumerate(parts):
        assert ES.bits_equal(p["obs"], whole["obs"][i * n:(i + 1) * n + 1]), i
        assert ES.bits_equal(p["obs_read"], whole["obs_read"][i * n:(i + 1) * n + 1]), i
        if i + 1 < pieces:                                    # the row formed without committing is the row the next launch forms
            assert ES.bits_equal(p["obs_read"][n], parts[i + 1]["obs_read"][0]), i
    CD.same(parts[-1], whole, keys=["state." + s for s in CD.STATE])
    assert ES.bits_equal(parts[-1]["held"], whole["held"])
    # the state moves between the pieces (it is not the last launch alone that writes it)
    assert not ES.bits_equal(parts[0]["held"], whole["held"])


# ---- 4: members ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ((1, False), (8, False), (16, True)), ids=["N1", "N8", "N16-group"])
def test_members_are_independent(g, shape):
    N, group = shape
    d0 = corr(g)
    d1 = g.CorrelatedDisturbance.normalised(sep=0.02, cpa=0.0, closing=0.2, action=0.1, seed=7, rho_sep=0.3, rho_cpa=0.9,
                                            rho_closing=1.0, rho_action=0.0)
    both = cpair(g, N, group, (d0, d1))
    CD.every_env_was_reset(both, 2 * EM)
    for k, d in enumerate((d0, d1)):
        alone = csolo(g, N, group, d, E=EM, offset=k * EM, seed=1 + k, key=NOISE_SEED + k)
        CD.same(both, alone, cols=slice(k * EM, (k + 1) * EM))
        assert ES.bits_equal(both["held"][:, k * EM:(k + 1) * EM], alone["held"])
    assert not ES.bits(both["held"][-1, EM:]).any() and ES.bits(both["held"][-1, :EM]).all()     # rho_action: 0 beside 0.5
    # a white member beside a correlated one: the white collector's columns, and no state
    w = g.Disturbance.normalised(sep=0.02, cpa=0.0, closing=0.2, action=0.1, seed=7)
    mixed = cpair(g, N, group, (d0, w))
    white = CD.solo(g, N, group, w, E=EM, offset=EM, seed=2, key=NOISE_SEED + 1)
    CD.same(mixed, white, cols=slice(EM, 2 * EM))
    assert not ES.bits(mixed["held"][:, EM:]).any()
    CD.same(mixed, csolo(g, N, group, d0, E=EM, offset=0, seed=1, key=NOISE_SEED), cols=slice(0, EM))


# ---- 5: work shape ----------------------------------------------------------------------------------------------------------------
def test_work_shape_does_not_matter(g):
    a, b = csolo(g, 8, False, corr(g)), csolo(g, 8, True, corr(g))
    CD.same(a, b)
    assert ES.bits_equal(a["held"], b["held"]) and ES.bits(a["held"]).any()


# ---- 6: the bootstrap value -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (1, 8))
def test_bootstrap_value_is_the_next_collections_first(g, N):
    env, pol = CD.make_env(g, E1, N), CD.policy(g, N)
    ds = g.CorrelatedDisturbanceSet(corr(g), 1)
    one = env.collect(pol, T, noise_seed=NOISE_SEED, noise_step=NOISE_STEP, disturbance=ds)
    _, _, last = g.gae_fused(one["reward"], one["values"], one["done"], None, critic=pol, obs_last=one["obs_read"][T])
    last = last.cpu().numpy().copy()
    read_T = one["obs_read"][T].cpu().numpy().copy()
    two = env.collect(pol, T, noise_seed=NOISE_SEED, noise_step=NOISE_STEP + T, disturbance=ds)
    assert ES.bits_equal(read_T, two["obs_read"][0].cpu().numpy())
    assert ES.bits_equal(last, two["values"][0].cpu().numpy())
    # ... which the true observation's value is not
    _, _, true = g.gae_fused(one["reward"], one["values"], one["done"], None, critic=pol, obs_last=one["obs"][T])
    assert 2 * int((ES.bits(true.cpu().numpy()) != ES.bits(last)).sum()) >= E1


# ---- 7: a bias on the actuator ----------------------------------------------------------------------------------------------------
def test_full_actuator_correlation_is_a_constant_action(g):
    """rho_action = 1, no sensor noise, an actor whose mean is 0 and whose spread is 0 (log_std = -inf: the raw action is
    fma(0, eps, 0)): the env flies disturb_action(0, s, z_1) at every step of an episode, z_1 the actuator's normal of the
    episode's first step.  The collector has no a_lat output; the per-step env that is sent that action -- a_lat = action x
    the limit -- returns the launch's observations, rewards and outcomes and ends in its state, bit for bit."""
    N = 1
    bias = g.CorrelatedDisturbance.normalised(action=0.3, seed=7, rho_action=1.0)
    pol = CD.policy(g, N)
    with torch.no_grad():
        pol.action_net.weight.zero_()
        pol.action_net.bias.zero_()
        pol.log_std.fill_(-float("inf"))
    env, r = CD.make_env(g, E1, N), CD.make_env(g, E1, N)
    ds = g.CorrelatedDisturbanceSet(bias, 1)
    out = CD.host(env.collect(pol, T, noise_seed=NOISE_SEED, noise_step=NOISE_STEP, disturbance=ds), env)
    assert not out["actions"].any()                           # the buffer keeps the raw action: 0
    assert ES.bits_equal(out["obs_read"], out["obs"])         # no sensor noise
    # ... and a latching env with record_trace, put into r's state in front of every step, gives that step's a_lat
    lat = g.ACAS2DVecEnv(E1, N, device=DEV, dtype=F32, auto_reset=False, record_trace=True,
                         config=g.ACAS2DConfig(n_traffic=N, max_steps=CD.MAX_STEPS))
    col = list(g.vec_env.TRACE_COLUMNS).index("a_lat")
    flown, a_lat = [], []
    for t in range(T):
        episode = r.episode.cpu().numpy().view(np.uint32)
        z1 = CD.normals_for(g, bias.seed, 0, episode, np.ones(E1, np.int32), N)[:, 0, 0]
        a = g.records.disturb_action(np.zeros(E1, np.float32), bias.s_action, z1)
        flown.append(a)
        lat.set_state(*g.policy.read_state(r), steps=r.steps.cpu().numpy(), observe=False)
        seen = lat.step(torch.as_tensor(a, device=DEV))[0].cpu().numpy()
        a_lat.append(lat.trace.cpu().numpy()[:, col].copy())
        going = out["done_u8"][t] == 0                        # (a finished env's next row is its fresh episode's; at
                                                              #  max_steps = 5 whole steps have none going)
        assert ES.bits_equal(out["obs"][t + 1][going], seen[going]), t                      # the launch flew THIS a_lat
        obs, rew, done, infos = r.step(torch.as_tensor(a, device=DEV))
        assert ES.bits_equal(out["obs"][t + 1], obs.cpu().numpy()), t
        assert ES.bits_equal(out["reward"][t], rew.cpu().numpy()), t
        assert np.array_equal(out["done_u8"][t], done.cpu().numpy().astype(np.uint8)), t
        assert np.array_equal(out["outcome"][t], infos.outcome.cpu().numpy()), t
    for n in CD.STATE:
        assert ES.bits_equal(out["state." + n], getattr(r, n).cpu().numpy()), n
    flown = np.stack(flown)
    assert (flown != 0).all() and (np.abs(flown) < 1).any()
    CD.every_env_was_reset(out, E1)
    changed = ES.bits(flown[1:]) != ES.bits(flown[:-1])
    assert changed.any(0).all()                               # a new episode flies another action ...
    assert np.array_equal(changed, out["done_u8"][:-1] != 0)  # ... and nothing else changes it
    # the per-step env's a_lat: one value per episode, as test_correlated.py reads the evaluator's -- it moves where an episode
    # ended and nowhere else, and is the flown action x the limit
    a_lat = np.stack(a_lat)
    assert (a_lat != 0).all() and np.array_equal(ES.bits(a_lat[1:]) != ES.bits(a_lat[:-1]), out["done_u8"][:-1] != 0)
    assert ES.bits_equal(a_lat, (flown * np.float32(g.ACAS2DConfig().to_c().acc_lat_limit)).astype(np.float32))
    # held: z_1 of the episode the last step was played in (rho 1 carries it, q = 0), and nothing on the sensors' rows
    assert ES.bits_equal(ds.held_numpy()[-1], z1)
    assert not ES.bits(ds.held_numpy()[:-1]).any()
    # ... where the white actuator noise of the same sigma and seed flies something else
    white = CD.host(CD.make_env(g, E1, N).collect(pol, T, noise_seed=NOISE_SEED, noise_step=NOISE_STEP,
                                                  disturbance=g.Disturbance.normalised(action=0.3, seed=7)))
    assert not ES.bits_equal(white["reward"], out["reward"])


# ---- 8: the trainers --------------------------------------------------------------------------------------------------------------
def test_rho_zero_trains_the_white_bits(g):
    d = CD.noisy(g)
    a = CD.two_iterations(CD.solo_trainer(g, gae="kernel", disturbance=d))
    b = CD.two_iterations(CD.solo_trainer(g, gae="kernel", disturbance=g.CorrelatedDisturbanceSet(d, 1)))
    assert a.keys() == b.keys() and all(ES.bits_equal(a[k], b[k]) for k in a)
    a = CD.two_iterations(CD.population(g, gae="kernel", disturbances=d))
    b = CD.two_iterations(CD.population(g, gae="kernel", disturbances=g.CorrelatedDisturbanceSet(d, 2)))
    assert a.keys() == b.keys() and all(ES.bits_equal(a[k], b[k]) for k in a)


def test_correlated_training_repeats_itself(g):
    white = CD.two_iterations(CD.solo_trainer(g, gae="kernel", disturbance=CD.noisy(g)))
    a, b = (CD.two_iterations(CD.solo_trainer(g, gae="kernel", disturbance=g.CorrelatedDisturbanceSet(corr(g), 1))) for _ in range(2))
    assert all(ES.bits_equal(a[k], b[k]) for k in a) and not all(ES.bits_equal(a[k], white[k]) for k in a)
    ds = [corr(g), g.CorrelatedDisturbance.normalised(sep=0.1, action=0.1, seed=7, rho=0.99)]
    a, b = (CD.two_iterations(CD.population(g, gae="kernel", disturbances=g.CorrelatedDisturbanceSet(ds, 2))) for _ in range(2))
    assert all(ES.bits_equal(a[k], b[k]) for k in a)


def test_pbt_exploit_leaves_the_coefficients_and_the_state(g):
    K = 4
    ms = [g.CorrelatedDisturbance.normalised(sep=0.02 * k, action=0.1 * k, seed=7, rho_sep=0.25 * k, rho_action=0.2 * k) for k in range(K)]
    ds = g.CorrelatedDisturbanceSet(ms, K)
    # (max_steps = 5: episodes end inside the first collection, so there is a score to exploit by)
    tr = CD.population(g, g.PBTTrainer, K, config=g.ACAS2DConfig(n_traffic=1, max_steps=CD.MAX_STEPS),
                       pbt=g.PBTConfig(ready_every=1, fraction=0.25, seed=3), disturbances=ds)
    assert tr.disturbances is ds
    rows, corr_rows = ds.rows.copy(), ds.corr_rows.copy()
    tr.collect()
    held = ds.held_numpy()
    assert held.shape == (4, K * EM) and not ES.bits(held[:, :EM]).any() and ES.bits(held[0, EM:]).all()
    tr.update()                                               # ready_every = 1: followed by exploit()
    recs = [r for r in tr.history if "exploit" in r]
    assert len(recs) == K and sum(r["exploit"] is not None for r in recs) == 1
    assert np.array_equal(ds.rows, rows) and ES.bits_equal(ds.corr_rows, corr_rows)
    assert [d.to_dict() for d in ds.members] == [d.to_dict() for d in ms]
    assert ES.bits_equal(ds.held_numpy(), held)               # the state is the envs': nothing of it is copied
    # the set in the trainer's state: plain numbers with the rho keys, read back, another correlation refused
    sd = json.loads(json.dumps(tr.state_dict()))
    assert sd == {"disturbance": ds.state_dict()} and sd["disturbance"]["members"][2]["rho_sep"] == 0.5
    tr.load_state_dict(sd)
    sd["disturbance"]["members"][2]["rho_sep"] = 0.75
    with pytest.raises(ValueError, match="goes on under the noise it was started with"):
        tr.load_state_dict(sd)
    # the held state across a restart: put back into a fresh set on a fresh env
    again = g.CorrelatedDisturbanceSet(ms, K)
    again.load_held(held)
    assert ES.bits_equal(again.bind(CD.make_env(g, K * EM, 1)).cpu().numpy(), held)
