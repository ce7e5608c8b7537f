"""The collectors under sensor noise and actuator disturbance on the GPU (acas2d_collect_set_disturbed_f32 / _group_f32;
ACAS2DVecEnv.collect(disturbance=), collect_set(disturbances=), the trainers' disturbance=):

  1  all four standard deviations 0: the plain collectors' bits, and obs_read is the true observation;
  2  disturbed, against a host loop with no new arithmetic -- per step the true observation and (episode, steps) of a
     per-step env, records.disturb_observation() on the draw entry's normals (= obs_read[t], bit for bit), the project's own
     networks and sampler through a one-step undisturbed collect() on that row, records.disturb_action(), the env step --
     also under sigmas of two box widths, and (2b) on rows whose traffic entries are tests/edge_observations.py's table: the
     ends of the boxes and their neighbours, both zeros, denormals, +-FLT_MAX, +-inf and NaN under one channel at a time, a
     saturating, a vanishing and an overflowing disturbance -- the handle on the device function disturbed();
  3  member k of two with different sigmas is the one-member launch on its envs; a zero member beside a noisy one is the
     plain collector;  4  thread-per-env and group shape agree at eight aircraft;  5  one launch of 16 steps is two of 8;
  6  gae_fused on obs_read[T] returns the bits of the next collection's values[0];
  7  after PPOTrainer(disturbance=).collect() the buffer holds what the actor read: torch's log-probability on b_obs agrees
     with b_logp, on the true observations it does not;
  8  the trainers: a zero disturbance trains the undisturbed run's bits, a disturbed run repeats itself, a PBT exploit step
     leaves the members' sigmas where they were.

70 envs for one member (two waves thread per env, one of them partial), 2 x 64 for two, 16 steps, and max_steps = 5: every env
times out and is reset inside every launch, three times in 16 steps.  1 and 2b run at all nine compiled work shapes, 2 at
every one but (4,2), which 4 holds to (8,1)."""
import numpy as np
import pytest
import torch

import edge_observations as EO
import eval_stats_support as ES
import helpers as H
import monte_carlo_support as MS

pytestmark = pytest.mark.gpu
DEV = ES.DEV
F32 = torch.float32
T, E1, EM = 16, 70, 64
MAX_STEPS = 5
NOISE_SEED, NOISE_STEP = 21, 3
KEYS = ("obs", "actions", "values", "logp", "reward", "done_u8", "outcome", "episode_return", "episode_steps")
STATE = ("own_x", "own_y", "own_psi", "trf_x", "trf_y", "trf_psi", "trf_v", "steps", "total_reward", "episode")
# (n_traffic, group)
# the host loop: every compiled work shape but (4,2), which test_work_shape_does_not_matter holds to (8,1)
LOOP_SHAPES = ((1, False), (3, False), (8, False), (16, True), (64, True), (2, False), (4, False), (32, True))
# all nine compiled work shapes (C, G): (1,1) (3,1) (8,1) (4,4) (4,16) (2,1) (4,1) (4,8) (4,2)
ALL_SHAPES = LOOP_SHAPES + ((8, True),)
SATURATING_SHAPES = ((3, False), (16, True))
# the injected rows: every disturbance of edge_observations at three shapes, the saturating one at all nine
INJECTED = ([(s, name) for s in ((1, False), (3, False), (16, True)) for name in EO.DISTURBANCES] +
            [(s, "saturating") for s in ALL_SHAPES if s not in ((1, False), (3, False), (16, True))])
# torch's log-probability against the collector's: the bound of the fused-collector test (test_ppo.py: largest and mean
# absolute difference)
LOGP_MAX, LOGP_MEAN = 2e-3, 2e-5


def shape_id(s):
    return "N%d%s" % (s[0], "-group" if s[1] else "")


@pytest.fixture(scope="module")
def g():
    import gym_acas2d_amd as g
    return g


def noisy(g, seed=7):
    return g.Disturbance.normalised(sep=0.05, cpa=0.1, closing=0.1, action=0.3, seed=seed)


def saturating(g):
    return g.Disturbance.normalised(**EO.SATURATING, seed=EO.SEED)


def injected_id(case):
    return "%s-%s" % (shape_id(case[0]), case[1])


def make_env(g, E, N, offset=0, episodes=False):
    """episodes: the even envs' episode counters start at helpers.WIDE_EPISODE = 2^32 - 2, so that their second reset wraps
    the counter to 0 inside a launch."""
    cfg = g.ACAS2DConfig(n_traffic=N, max_steps=MAX_STEPS)
    env = g.ACAS2DVecEnv(E, N, device=DEV, dtype=F32, seed=13, env_offset=offset, config=cfg)
    if episodes:
        env.reset_to_episode(np.where(H.wide_preset(E), H.WIDE_EPISODE, 0))
    else:
        env.reset()
    return env


def policy(g, N, seed=1, head=20.0):
    """A randomly initialised ActorCritic whose action head is scaled up: the mean moves with the observation."""
    torch.manual_seed(seed)
    pol = g.ActorCritic(5 + 3 * N)
    with torch.no_grad():
        pol.action_net.weight.mul_(head)
    return pol


def host(out, env=None):
    d = {k: out[k].cpu().numpy() for k in KEYS + (("obs_read",) if "obs_read" in out else ())}
    if env is not None:
        d.update({"state." + n: getattr(env, n).cpu().numpy() for n in STATE})
    return d


def every_env_was_reset(d, E):
    """The launch went through the in-step reset in every env, and the episode field of the counter moved."""
    assert d["done_u8"].shape == (T, E) and (d["done_u8"].sum(0) >= 1).all()
    assert (d["state.episode"].view(np.uint32) >= 1).all()


def same(a, b, keys=None, cols=slice(None)):
    for k in keys or [k for k in a if k in b]:
        x = a[k][cols] if k.startswith("state.") else a[k][:, cols]
        assert ES.bits_equal(x, b[k]), k


_RUNS = {}


def solo(g, N, group, dist="noisy", E=E1, offset=0, seed=1, key=NOISE_SEED, cuts=(T,), episodes=False):
    """collect() of `cuts` steps in a row on a fresh env (cached: a reference is computed once and left alone)."""
    name = (N, group, dist, E, offset, seed, key, cuts) + ((episodes,) if episodes else ())
    if name not in _RUNS:
        env, pol = make_env(g, E, N, offset, episodes), policy(g, N, seed)
        d = ({"noisy": noisy(g), "zero": g.Disturbance(seed=99), "saturating": saturating(g), None: None}[dist]
             if isinstance(dist, (str, type(None))) else dist)
        outs, at = [], NOISE_STEP
        for n in cuts:
            outs.append(host(env.collect(pol, n, noise_seed=key, noise_step=at, group=group,
                                         **({} if d is None else {"disturbance": d})), env))
            at += n
        torch.cuda.synchronize()
        _RUNS[name] = outs[0] if len(cuts) == 1 else outs
    return _RUNS[name]


def pair(g, N, group, dists):
    """collect_set() of two members (policies 1 and 2, keys 21 and 22) on 2 x 64 envs."""
    name = ("pair", N, group, tuple(dists) if dists is not None else None)
    if name not in _RUNS:
        env = make_env(g, 2 * EM, N)
        pset = g.ActorCriticSet.from_members([policy(g, N, 1), policy(g, N, 2)], device=DEV)
        kw = {} if dists is None else {"disturbances": list(dists)}
        _RUNS[name] = host(env.collect_set(pset, T, [NOISE_SEED, NOISE_SEED + 1], noise_step=NOISE_STEP, group=group, **kw), env)
    return _RUNS[name]


# ---- 1: zero is identity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=[shape_id(s) for s in ALL_SHAPES])
def test_zero_sigmas_are_the_plain_collectors(g, shape):
    N, group = shape
    plain, zero = solo(g, N, group, None), solo(g, N, group, "zero")
    every_env_was_reset(plain, E1)
    assert set(zero) == set(plain) | {"obs_read"}
    same(plain, zero)
    assert ES.bits_equal(zero["obs_read"], plain["obs"])          # rows 0 .. T-1: [obs_in, obs[:-1]]; row T: the next one
    plain2, zero2 = pair(g, N, group, None), pair(g, N, group, (g.Disturbance(seed=5), g.Disturbance(seed=5)))
    every_env_was_reset(plain2, 2 * EM)
    same(plain2, zero2)
    assert ES.bits_equal(zero2["obs_read"], plain2["obs"])


# ---- 2: against a host loop -----------------------------------------------------------------------------------------------------
def normals_for(g, seed, offset, episode, steps, N):
    """[E, N + 1, 3]: the draw entry's normals of (offset + i, episode[i], steps[i], every slot)."""
    E = episode.shape[0]
    z = np.zeros((E, N + 1, 3), np.float32)
    for e in np.unique(episode):
        block = g.policy.disturbance_draw(seed, offset, E, int(e), 0, int(steps.max()) + 1, N + 1, device=DEV)
        rows = np.nonzero(episode == e)[0]
        z[rows] = block[steps[rows], rows]
    return z


def host_loop(g, N, group, dist, E=E1, offset=0, episodes=False):
    r, scratch, pol = make_env(g, E, N, offset, episodes), make_env(g, E, N, offset), policy(g, N)
    rows = {k: [] for k in ("obs_read", "actions", "values", "logp", "flown", "reward", "done_u8", "outcome", "obs",
                            "episode_return", "episode_steps")}
    rows["obs"].append(r.outputs["obs"].cpu().numpy().copy())

    def read_row():
        true = r.outputs["obs"].cpu().numpy()
        z = normals_for(g, dist.seed, offset, r.episode.cpu().numpy().view(np.uint32), r.steps.cpu().numpy(), N)
        return g.records.disturb_observation(true, dist.sigma, z[:, 1:]), z[:, 0, 0]

    for t in range(T):
        read, z_act = read_row()
        rows["obs_read"].append(read)
        scratch.outputs["obs"].copy_(torch.as_tensor(read, device=DEV))
        one = scratch.collect(pol, 1, noise_seed=NOISE_SEED, noise_step=NOISE_STEP + t, group=group)
        raw = one["actions"][0].cpu().numpy()
        flown = g.records.disturb_action(np.clip(raw, np.float32(-1), np.float32(1)), dist.s_action, z_act)
        obs, rew, done, infos = r.step(torch.as_tensor(flown, device=DEV))
        fin = done.cpu().numpy()
        for k, v in (("actions", raw), ("values", one["values"][0].cpu().numpy()), ("logp", one["logp"][0].cpu().numpy()),
                     ("flown", flown), ("reward", rew.cpu().numpy()), ("done_u8", fin.astype(np.uint8)),
                     ("outcome", infos.outcome.cpu().numpy()), ("obs", obs.cpu().numpy()),
                     ("episode_return", np.where(fin, infos.episode_return.cpu().numpy(), np.float32(0))),
                     ("episode_steps", np.where(fin, infos.episode_steps.cpu().numpy(), np.int32(0)))):
            rows[k].append(np.array(v, copy=True))
    rows["obs_read"].append(read_row()[0])                     # what the next launch's first step reads
    out = {k: np.stack(v) for k, v in rows.items()}
    out.update({"state." + n: getattr(r, n).cpu().numpy() for n in STATE})
    return out


@pytest.mark.parametrize("shape", LOOP_SHAPES, ids=[shape_id(s) for s in LOOP_SHAPES])
def test_disturbed_collector_equals_the_host_loop(g, shape):
    N, group = shape
    ref = host_loop(g, N, group, noisy(g))
    every_env_was_reset(ref, E1)
    # teeth, first: what the env was sent differs from the undisturbed run's in at least half of the envs (step 0: same state)
    plain = solo(g, N, group, None)
    sent_plain = np.clip(plain["actions"][0], np.float32(-1), np.float32(1))
    moved = int((ES.bits(ref["flown"][0]) != ES.bits(sent_plain)).sum())
    assert 2 * moved >= E1, moved
    assert 2 * int((ES.bits(ref["obs_read"][0]) != ES.bits(ref["obs"][0])).any(-1).sum()) >= E1
    got = solo(g, N, group, "noisy")
    for k in ("obs_read",) + KEYS + tuple("state." + n for n in STATE):
        assert ES.bits_equal(got[k], ref[k]), k
    # the seed is part of the noise
    other = solo(g, N, group, noisy(g, seed=8))
    assert not ES.bits_equal(other["obs_read"], got["obs_read"]) and not ES.bits_equal(other["reward"], got["reward"])


# the collectors' wide keys: the noise lane -- here the global env index -- crosses 2^32 at env 37 of the 70
# (monte_carlo_support.WIDE_LANE_OFFSET), the noise seed is helpers.WIDE_SEED, and the even envs' counters are preset
WIDE_SHAPES = ((1, False), (16, True))
WIDE = dict(offset=MS.WIDE_LANE_OFFSET, episodes=True)


def preset_counters_wrapped(ref, E):
    """On the reference alone: every env was reset at least three times inside the launch, so every preset counter went
    through 2^32 - 1 to 0 -- the counters end at the number of resets, the preset ones two below it."""
    pre, dones = H.wide_preset(E), ref["done_u8"].astype(np.int64).sum(0)
    end = ref["state.episode"].view(np.uint32).astype(np.int64)
    assert ref["done_u8"].shape == (T, E) and (dones >= 3).all()
    assert np.array_equal(end[pre], dones[pre] - 2) and np.array_equal(end[~pre], dones[~pre])


@pytest.mark.parametrize("shape", WIDE_SHAPES, ids=[shape_id(s) for s in WIDE_SHAPES])
def test_disturbed_collector_equals_the_host_loop_at_wide_keys(g, shape):
    N, group = shape
    dist = noisy(g, seed=MS.WIDE_SEED)
    ref = host_loop(g, N, group, dist, **WIDE)
    preset_counters_wrapped(ref, E1)
    assert (ES.bits(ref["obs_read"]) != ES.bits(ref["obs"])).any(-1).any(0).all()     # every env reads noise, on both sides of the crossing
    got = solo(g, N, group, dist, **WIDE)
    for k in ("obs_read",) + KEYS + tuple("state." + n for n in STATE):
        assert ES.bits_equal(got[k], ref[k]), k


@pytest.mark.parametrize("shape", SATURATING_SHAPES, ids=[shape_id(s) for s in SATURATING_SHAPES])
def test_saturating_collector_equals_the_host_loop(g, shape):
    """Sigmas of two box widths: the clamps of disturbed() decide most entries of every row and most actions."""
    N, group = shape
    ref = host_loop(g, N, group, saturating(g))
    every_env_was_reset(ref, E1)
    EO.check_saturated(ref["obs_read"], ref["flown"], g.records.OBSERVATION_BOX)      # teeth, on the reference alone
    got = solo(g, N, group, "saturating")
    for k in ("obs_read",) + KEYS + tuple("state." + n for n in STATE):
        assert ES.bits_equal(got[k], ref[k]), k


# ---- 2b: hand-placed entries in the row the launch reads ---------------------------------------------------------------------------
def injected_rows_meet_the_reference(g, shape, dist, launches=1, draw=None, dset=None, held=None, vanishing=False):
    """One-step collections whose first row carries edge_observations' table in its traffic columns, written into
    env.outputs["obs"] where the collector reads it.  Per launch, no new arithmetic: obs_read[0] is
    records.disturb_observation() of that row under `draw` (normals_for's signature: the normals, or the errors in their
    place) at the env's (global lane, episode, steps); actions / values / logp [0] are the undisturbed one-step collect() on
    the reference's row (the host loop's own step: the networks' NaN scrub is theirs); the env is sent
    records.disturb_action() of the clipped action, so obs[1], reward and done are a per-step env's.  Bit for bit, but a NaN
    of the reference may be any NaN.  dset: what collect() takes as disturbance= (default dist); held(): (the launch's,
    the reference's) error state after each launch."""
    N, group = shape
    boxes = g.records.OBSERVATION_BOX
    env, r, scratch, pol = make_env(g, E1, N), make_env(g, E1, N), make_env(g, E1, N), policy(g, N)
    draw = draw or normals_for
    for at in range(launches):
        row = EO.inject(r.outputs["obs"].cpu().numpy(), boxes, shift=3 * at)
        assert ES.bits_equal(row[:, :5], env.outputs["obs"].cpu().numpy()[:, :5])     # the own-ship five: as the env left them
        z = draw(g, dist.seed, 0, r.episode.cpu().numpy().view(np.uint32), r.steps.cpu().numpy(), N)
        read = g.records.disturb_observation(row, dist.sigma, z[:, 1:])
        EO.check_reference(row, read, dist.sigma, boxes, vanishing)               # on the reference alone
        scratch.outputs["obs"].copy_(torch.as_tensor(read, device=DEV))
        one = scratch.collect(pol, 1, noise_seed=NOISE_SEED, noise_step=NOISE_STEP + at, group=group)
        raw = one["actions"][0].cpu().numpy()
        flown = g.records.disturb_action(np.clip(raw, np.float32(-1), np.float32(1)), dist.s_action, z[:, 0, 0])
        assert np.isfinite(raw).all() and (np.abs(flown) <= 1).all()
        env.outputs["obs"].copy_(torch.as_tensor(row, device=DEV))
        got = host(env.collect(pol, 1, noise_seed=NOISE_SEED, noise_step=NOISE_STEP + at, group=group,
                               disturbance=dist if dset is None else dset))
        assert EO.same_but_for_nan_bits(got["obs_read"][0], read), at
        assert ES.bits_equal(got["obs"][0], row), at                              # the true row: as it was written
        for k in ("actions", "values", "logp"):
            assert ES.bits_equal(got[k][0], one[k][0].cpu().numpy()), (at, k)
        obs, rew, done, _ = r.step(torch.as_tensor(flown, device=DEV))
        assert ES.bits_equal(got["obs"][1], obs.cpu().numpy()) and ES.bits_equal(got["reward"][0], rew.cpu().numpy()), at
        assert np.array_equal(got["done_u8"][0], done.cpu().numpy().astype(np.uint8)), at
        if held is not None:
            ours, theirs = held()
            assert ES.bits_equal(ours, theirs), at


@pytest.mark.parametrize("case", INJECTED, ids=[injected_id(c) for c in INJECTED])
def test_injected_rows_meet_the_reference(g, case):
    shape, name = case
    dist = g.Disturbance.normalised(**EO.DISTURBANCES[name], seed=EO.SEED)
    injected_rows_meet_the_reference(g, shape, dist, vanishing=name == "vanishing")


# ---- 3: members -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ((1, False), (8, False), (16, True)), ids=["N1", "N8", "N16-group"])
def test_members_are_independent(g, shape):
    N, group = shape
    d0 = noisy(g)
    d1 = g.Disturbance.normalised(sep=0.02, cpa=0.0, closing=0.2, action=0.1, seed=7)
    both = pair(g, N, group, (d0, d1))
    every_env_was_reset(both, 2 * EM)
    for k, d in enumerate((d0, d1)):
        alone = solo(g, N, group, d, E=EM, offset=k * EM, seed=1 + k, key=NOISE_SEED + k)
        same(both, alone, cols=slice(k * EM, (k + 1) * EM))
    # a zero member beside a noisy one: the plain collector's columns, and the true rows
    mixed = pair(g, N, group, (d0, g.Disturbance(seed=7)))
    plain = solo(g, N, group, None, E=EM, offset=EM, seed=2, key=NOISE_SEED + 1)
    same(mixed, plain, cols=slice(EM, 2 * EM))
    assert ES.bits_equal(mixed["obs_read"][:, EM:], plain["obs"])
    same(mixed, solo(g, N, group, d0, E=EM, offset=0, seed=1, key=NOISE_SEED), cols=slice(0, EM))


# ---- 4, 5: work shape, cutting --------------------------------------------------------------------------------------------------
def test_work_shape_does_not_matter(g):
    same(solo(g, 8, False, "noisy"), solo(g, 8, True, "noisy"))


@pytest.mark.parametrize("shape", ((3, False), (16, True)), ids=["N3", "N16-group"])
def test_one_launch_is_two_halves(g, shape):
    N, group = shape
    whole = solo(g, N, group, "noisy")
    first, second = solo(g, N, group, "noisy", cuts=(T // 2, T // 2))
    h = T // 2
    for k in KEYS[1:]:
        assert ES.bits_equal(np.concatenate([first[k], second[k]]), whole[k]), k
    assert ES.bits_equal(first["obs"], whole["obs"][:h + 1]) and ES.bits_equal(second["obs"], whole["obs"][h:])
    assert ES.bits_equal(first["obs_read"], whole["obs_read"][:h + 1]) and ES.bits_equal(second["obs_read"], whole["obs_read"][h:])
    same(second, whole, keys=["state." + n for n in STATE])


# ---- 6: the bootstrap value ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (1, 8))
def test_bootstrap_value_is_the_next_collections_first(g, N):
    env, pol = make_env(g, E1, N), policy(g, N)
    d = noisy(g)
    one = env.collect(pol, T, noise_seed=NOISE_SEED, noise_step=NOISE_STEP, disturbance=d)
    _, _, last = g.gae_fused(one["reward"], one["values"], one["done"], None, critic=pol, obs_last=one["obs_read"][T])
    last = last.cpu().numpy().copy()
    two = env.collect(pol, T, noise_seed=NOISE_SEED, noise_step=NOISE_STEP + T, disturbance=d)
    assert ES.bits_equal(last, two["values"][0].cpu().numpy())
    # ... which the true observation's value is not
    _, _, true = g.gae_fused(one["reward"], one["values"], one["done"], None, critic=pol, obs_last=one["obs"][T])
    assert 2 * int((ES.bits(true.cpu().numpy()) != ES.bits(last)).sum()) >= E1


# ---- 7: the buffer holds what the actor read ---------------------------------------------------------------------------------
def test_buffer_holds_what_the_actor_read(g):
    N = 3
    venv = g.ACAS2DVecEnv(E1, N, device=DEV, dtype=F32, seed=13)
    pol = policy(g, N, head=100.0)
    d = g.Disturbance.normalised(sep=0.05, cpa=0.05, closing=0.05, action=0.2, seed=7)
    tr = g.PPOTrainer(venv, g.PPOConfig(n_steps=T, batch_size=256, n_epochs=1, seed=3), policy=pol, collector="fused",
                      updater="fused", gae="kernel", disturbance=d)
    tr.collect()
    torch.cuda.synchronize()
    true = tr._fused_out["obs"][:T].to(F32)
    with torch.no_grad():
        def logp_on(obs):
            mean, _ = tr.policy.forward(torch.nan_to_num(obs, nan=0.0, posinf=0.0, neginf=0.0).reshape(T * E1, -1))
            return g.ppo._normal_logp(mean, tr.policy.log_std, tr.b_act.reshape(T * E1, 1)).reshape(T, E1)
        read_err = (logp_on(tr.b_obs) - tr.b_logp).abs()
        true_err = (logp_on(true) - tr.b_logp).abs()
    print("\nlogp on b_obs against b_logp: max %.3e mean %.3e; on the true observations: %.1f %% of the samples beyond %.0e"
          % (float(read_err.max()), float(read_err.mean()), 100 * float((true_err > LOGP_MAX).float().mean()), LOGP_MAX))
    assert float(read_err.max()) < LOGP_MAX and float(read_err.mean()) < LOGP_MEAN
    assert 2 * int((true_err > LOGP_MAX).sum()) >= T * E1
    # self.obs stays the true observation, the bootstrap row is the disturbed one
    assert torch.equal(tr.obs, torch.nan_to_num(tr._fused_out["obs"][T]))
    assert torch.equal(tr.obs_boot, torch.nan_to_num(tr._fused_out["obs_read"][T])) and not torch.equal(tr.obs_boot, tr.obs)


# ---- 8: the trainers ---------------------------------------------------------------------------------------------------------
def params_of(tr):
    if hasattr(tr, "policy_set"):
        return {k: v.detach().cpu().numpy().copy() for k, v in tr.policy_set.params.items()}
    return {k: v.detach().cpu().numpy().copy() for k, v in tr.policy.state_dict().items()}


def two_iterations(tr):
    """(PPOTrainer draws its minibatch permutations from torch's global generator, whose state after the graph captures is
    not the same in every trainer of a process: seeded here, as the fused-update tests seed it.)"""
    for it in range(2):
        tr.collect()
        torch.manual_seed(99 + it)
        tr.update()
    torch.cuda.synchronize()
    return params_of(tr)


def solo_trainer(g, **kw):
    """(Minibatches of 64 rows: one wavefront sums the solo update's gradient, in a fixed order.  Larger ones are summed
    across workgroups with floating-point atomics, and two undisturbed trainers already differ in their last bits there.)"""
    venv = g.ACAS2DVecEnv(EM, 1, device=DEV, dtype=F32, seed=13)
    return g.PPOTrainer(venv, g.PPOConfig(n_steps=T, batch_size=64, n_epochs=2, seed=3), collector="fused", updater="fused", **kw)


def population(g, cls=None, K=2, config=None, **kw):
    venv = g.ACAS2DVecEnv(K * EM, 1, device=DEV, dtype=F32, seed=13, config=config)
    cfgs = [g.PPOConfig(n_steps=T, batch_size=64, n_epochs=2, seed=3 + k) for k in range(K)]      # (64: as solo_trainer)
    return (cls or g.PopulationTrainer)(venv, cfgs, **kw)


def test_zero_disturbance_trains_the_undisturbed_bits(g):
    a, b = two_iterations(solo_trainer(g)), two_iterations(solo_trainer(g, disturbance=g.Disturbance(seed=4)))
    assert a.keys() == b.keys() and all(ES.bits_equal(a[k], b[k]) for k in a)
    a, b = two_iterations(population(g)), two_iterations(population(g, disturbances=g.Disturbance(seed=4)))
    assert a.keys() == b.keys() and all(ES.bits_equal(a[k], b[k]) for k in a)


def test_disturbed_training_repeats_itself(g):
    d = noisy(g)
    plain = two_iterations(solo_trainer(g, gae="kernel"))
    a, b = (two_iterations(solo_trainer(g, gae="kernel", disturbance=d)) for _ in range(2))
    assert all(ES.bits_equal(a[k], b[k]) for k in a) and not all(ES.bits_equal(a[k], plain[k]) for k in a)
    ds = [d, g.Disturbance.normalised(sep=0.1, action=0.1, seed=7)]
    a, b = (two_iterations(population(g, gae="kernel", disturbances=ds)) for _ in range(2))
    assert all(ES.bits_equal(a[k], b[k]) for k in a)


def test_pbt_exploit_leaves_the_sigmas_in_their_slots(g):
    K = 4
    ds = [g.Disturbance.normalised(sep=0.02 * k, action=0.1 * k, seed=7) for k in range(K)]      # member 0: none
    # (max_steps = 5: episodes end inside the first collection, so there is a score to exploit by)
    tr = population(g, g.PBTTrainer, K, config=g.ACAS2DConfig(n_traffic=1, max_steps=MAX_STEPS),
                    pbt=g.PBTConfig(ready_every=1, fraction=0.25, seed=3), disturbances=ds)
    rows = tr.disturbances.rows.copy()
    tr.collect()
    tr.update()                                               # ready_every = 1: followed by exploit()
    recs = [r for r in tr.history if "exploit" in r]
    assert len(recs) == K and sum(r["exploit"] is not None for r in recs) == 1
    assert np.array_equal(tr.disturbances.rows, rows) and [d.to_dict() for d in tr.disturbances.members] == [d.to_dict() for d in ds]
    # the next collection, under the donor's weights: every member still reads ITS noise -- member 0 the true rows, member k
    # the rows records.disturb_observation() makes of them with its own sigmas
    episode, steps = tr.venv.episode.cpu().numpy().view(np.uint32).copy(), tr.venv.steps.cpu().numpy().copy()
    tr.collect()
    read, true = tr._fused_out["obs_read"].cpu().numpy(), tr._fused_out["obs"].cpu().numpy()
    for k in range(K):
        cols = slice(k * EM, (k + 1) * EM)
        z = normals_for(g, 7, k * EM, episode[cols], steps[cols], 1)
        assert ES.bits_equal(read[0, cols], g.records.disturb_observation(true[0, cols], ds[k].sigma, z[:, 1:])), k
        assert ES.bits_equal(read[:, cols], true[:, cols]) == (k == 0), k
    assert tr.state_dict() == {"disturbance": tr.disturbances.state_dict()}
