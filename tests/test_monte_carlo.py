"""Monte Carlo campaigns on the GPU (acas2d_monte_carlo_*, policy.MonteCarlo): the accumulators of a campaign against the
existing entries folded on the host (tests/monte_carlo_support.py) -- integers exactly, the per-lane arrays bit for bit --
and the properties a campaign is used for: chaining, resuming, common random numbers, reproducibility, regenerating an
encounter.  70 lanes x 3 episodes, K = 3 (two policies and the all-zero one), 16 bins, at every shape family and under
two configs.  Further down: the campaign at wide keys (a 64-bit seed, the lane crossing 2^32 inside a wave, counters up to
2^32 - 1), the histogram rule on a rounding edge, with one bin, past the last edge and at 4 096 bins, and 1, 64 and 129
lanes."""
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


# ---- wide keys ---------------------------------------------------------------------------------------------------------------------------
WIDE_SHAPES = [S.Shape(S.F32, True, 1, False, 150), S.Shape(S.F32, True, 8, False, 150), S.Shape(S.F32, True, 16, True, 150),
               S.Shape(S.F64, False, 1, False, 150)]


@pytest.mark.parametrize("s", WIDE_SHAPES, ids=[S.shape_id(s) for s in WIDE_SHAPES])
def test_campaign_at_wide_keys(g, s):
    """monte_carlo_support.WIDE: the seed's halves non-zero and distinct, the lane crossing 2^32 at local lane 37, the
    launch's last counter 2^32 - 1 -- every accumulator against the reference at those keys, the counters in
    lane_worst_episode, chaining, the closest encounters and the two lanes at the crossing regenerated and replayed, and
    the refusal of counter 2^32 (monte_carlo_support.campaign_at_wide_keys)."""
    S.campaign_at_wide_keys(g, s)


# ---- the histogram rule and the lane count -----------------------------------------------------------------------------------------------
HIST_SHAPES = [S.Shape(S.F32, True, 1, False, 150), S.Shape(S.F32, True, 16, True, 150), S.Shape(S.F64, False, 1, False, 150)]
HIST = pytest.mark.parametrize("s", HIST_SHAPES, ids=[S.shape_id(s) for s in HIST_SHAPES])


def histogram(g, s, n_bins, hist_max=None):
    """(the campaign's accumulators, the reference's) under the histogram (n_bins, hist_max): the cached per-counter results
    folded with the id's own bin rule."""
    kw = {} if hist_max is None else {"hist_max": hist_max}
    got = S.campaign(g, s, n_bins=n_bins, **kw).run(S.EPISODES).accumulators()
    assert got["sep_hist"].shape == (3, n_bins)
    return got, S.reference(g, s, n_bins=n_bins, hist_max=hist_max)


def separations(g, s):
    """[EPISODES, K, LANES]: the reference's minimum separations."""
    return np.stack([r["min_separation"] for r in S.per_counter(g, s)[:S.EPISODES]])


@HIST
def test_histogram_on_a_rounding_edge(g, s):
    """16 bins of a width at which the median separation's product with the inverse width is, rounded to the kernel's
    format, exactly a bin edge while the exact product lies below it (monte_carlo_support.edge_hist_max): a kernel that
    formed the product in another precision, or divided by the width, bins that episode one lower."""
    dt = S.npdt(s)
    m, hist_max = S.edge_separation(g, s, 16)
    inv = S.inv_bin_width(g, s, 16, hist_max)
    sep = separations(g, s)
    assert np.isfinite(sep).all() and (sep[:, 0] == m).any()
    moved = int((g.records.separation_bin(sep, 16, inv, dt) != S.exact_bins(sep, 16, inv, dt)).sum())
    print("\n%s: separation %r, hist_max %r, %d of %d episodes change their bin with the precision of the product"
          % (S.shape_id(s), float(m), hist_max, moved, sep.size))
    assert moved >= 1
    got, ref = histogram(g, s, 16, hist_max)
    same(g, got, ref)


@HIST
def test_histogram_of_one_bin(g, s):
    got, ref = histogram(g, s, 1)
    assert got["sep_hist"][:, 0].tolist() == [S.LANES * S.EPISODES] * 3
    same(g, got, ref)


@HIST
def test_histogram_past_the_last_edge(g, s):
    """hist_max = safe_distance / 64: most episodes lie beyond it and take the last bin through `q >= n_bins`;
    hist_max = 1e-30: every product is >= 2^31 (float32: some 1e33; none overflows to inf), so every episode takes it
    through the branch that never casts.  A non-finite minimum separation cannot be produced by a drawn campaign -- every
    episode has a step row with a finite d_sep -- so the NaN / inf side of that branch stays held on the CPU alone
    (tests/test_monte_carlo_host.py)."""
    dt = S.npdt(s)
    sep = separations(g, s)
    assert np.isfinite(sep).all() and (sep > 0).all()
    near = S.config(g, s).safe_distance / 64.0
    got, ref = histogram(g, s, S.N_BINS, near)
    assert (2 * ref["sep_hist"][:, -1] > S.LANES * S.EPISODES).all()
    same(g, got, ref)
    got, ref = histogram(g, s, S.N_BINS, 1e-30)
    with np.errstate(over="ignore"):
        scaled = sep.astype(dt) * dt(S.inv_bin_width(g, s, S.N_BINS, 1e-30))
    assert (scaled >= dt(2147483648.0)).all()
    assert ref["sep_hist"][:, -1].tolist() == [S.LANES * S.EPISODES] * 3
    same(g, got, ref)


@HIST
def test_fine_histogram(g, s):
    """4096 bins: at least 32 occupied bins per policy row, rows that differ, and all K x 4096 counters -- the row
    addressing k * n_bins + b.  At the default hist_max (4 x the safe distance) that holds with 16 aircraft.  A single
    aircraft never comes that close in these 210 encounters -- asserted: every separation lies past the default hist_max
    and the whole fine histogram is its last bin, which is compared too -- so those shapes are held to the spread under
    hist_max = d_sep_max, the bound of the observation's separation entry, which no separation exceeds."""
    got, ref = histogram(g, s, 4096)
    same(g, got, ref)
    hist_max = None
    if s.N == 1:
        sep, hist_max = separations(g, s), float(S.config(g, s).to_c().d_sep_max)
        assert ref["sep_hist"][:, -1].tolist() == [S.LANES * S.EPISODES] * 3 and (sep < hist_max).all()
        got, ref = histogram(g, s, 4096, hist_max)
    occupied = (ref["sep_hist"] > 0).sum(1)
    print("\n%s: hist_max %r, %s of 4096 bins occupied" % (S.shape_id(s), hist_max, occupied.tolist()))
    assert (occupied >= 32).all(), occupied
    assert all(not np.array_equal(ref["sep_hist"][a], ref["sep_hist"][b]) for a, b in ((0, 1), (0, 2), (1, 2)))
    same(g, got, ref)


LANE_COUNTS = [(s, n) for s in HIST_SHAPES[:2] for n in (1, 64, 129)]


@pytest.mark.parametrize("s,lanes", LANE_COUNTS, ids=["%s-L%d" % (S.shape_id(s), n) for s, n in LANE_COUNTS])
def test_lane_counts(g, s, lanes):
    """1 lane (63 padding lanes thread per env, 15 padding envs in the group shape's wave), exactly 64 (none) and 129 (more
    than two waves) against a reference computed for that lane count: padding lanes play nothing and count nothing, and the
    lane, not the launch, names the encounter."""
    ref = S.reference(g, s, lanes=lanes)
    got = S.campaign(g, s, lanes=lanes).run(S.EPISODES).accumulators()
    assert got["outcome_count"].sum(1).tolist() == got["sep_hist"].sum(1).tolist() == [lanes * S.EPISODES] * 3
    assert all(got[k].shape == (3, lanes) for k in g.records.MONTE_CARLO_LANE_KEYS)
    same(g, got, ref)
    n = min(lanes, S.LANES)
    for k in g.records.MONTE_CARLO_LANE_KEYS:
        assert S.bits_equal(got[k][:, :n], ran(g, s)[k][:, :n]), k


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
