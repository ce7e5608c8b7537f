"""The edge-state generator (tests/edge_states.py) against the CPU oracle: every case does what its label says, so the
GPU tests that run the batch on every work shape (tests/test_gpu_edge_states.py) cannot pass vacuously."""
import functools

import numpy as np
import pytest

import edge_states as ES
import helpers as H

NS = sorted({s.n_traffic for s in H.SHAPES})
_CASES = [(N, "default") for N in NS] + [(N, "small") for N in NS] + [(N, "wide") for N in (1, 8, 64)]


@functools.lru_cache(maxsize=None)
def _config(name):
    from oracle import oracle as O
    if name == "default":
        return O.default_config()
    import gym_acas2d_amd as g
    return H.oracle_config(O, g.ACAS2DConfig(n_traffic=1, **H.NONDEFAULT_CONFIGS[name]))


@pytest.mark.parametrize("N,config", _CASES, ids=["N%d-%s" % c for c in _CASES])
def test_edge_batch_does_what_its_labels_say(oracle_mod, N, config):
    O = oracle_mod
    cfg = _config(config)
    b = ES.edge_batch(N, cfg, seed=N)
    E, M, cd = len(b.case), int(cfg.max_steps), float(cfg.collision_dist)
    assert b.whole % ES.arena_unit(N) == 0 and E == b.whole + ES.TAIL
    d, d_goal, ref = ES.post_step_geometry(O, b, config=cfg)
    fam = ES.labels(b, "family")
    coll_slot = ES.labels(b, "coll_slot").astype(int)
    coll_off, goal_off = ES.labels(b, "coll_off").astype(float), ES.labels(b, "goal_off").astype(float)

    # every case sits at the first and at the last env of a wave of every work shape of N, and in the partial last wave
    W = ES.wave_unit(N)
    for k in range(len(b.cases)):
        at = np.nonzero(b.case == k)[0]
        assert (at % W == 0).any() and (at % W == W - 1).any(), k
    assert {b.cases[k].family for k in b.case[b.whole:]} == {c.family for c in b.cases}

    # collisions come from the placed slot only, at the placed offset; everything else stays MIN_SEP away
    placed = coll_slot >= 0
    rows = np.nonzero(placed)[0]
    np.testing.assert_allclose(d[rows, coll_slot[rows]] - cd, coll_off[rows], rtol=0, atol=1e-11)
    others = np.ones_like(d, bool)
    others[rows, coll_slot[rows]] = False
    near = np.isin(fam, ("parallel", "parallel+timeout", "mirror", "speeds"))       # placed 2 cd .. MIN_SEP away
    slot = ES.labels(b, "slot").astype(int)
    assert (d[near, slot[near]] > 2 * cd - 10).all()
    others[near, slot[near]] = False
    assert d[others].min() > ES.MIN_SEP - 10
    gp = ~np.isnan(goal_off)
    np.testing.assert_allclose(d_goal[gp] - cfg.goal_radius, goal_off[gp], rtol=0, atol=1e-11)
    assert (d_goal[~gp] > cfg.goal_radius + 20).all()
    for j in range(N):                          # a collision case at every slot, at every offset
        assert {o for s, o in zip(coll_slot[fam == "collision"], coll_off[fam == "collision"]) if s == j} == set(ES.OFFSETS)

    # in-band rows (1e-9 in float64; 1e-3 from the float32-rounded state) are exactly the ones placed there
    band64 = ES.in_band(cfg, d, d_goal, ES.F64_BAND)
    assert np.array_equal(band64, ES.placed_in_band(b, ES.F64_BAND)) and band64.sum() >= 3 * (N + 1)
    f32 = lambda a: np.asarray(a).astype(np.float32).astype(np.float64)  # noqa: E731
    d32, dg32, _ = ES.post_step_geometry(O, b, config=cfg, rounding=f32)
    band32 = ES.in_band(cfg, d32, dg32, ES.F32_BAND)
    assert np.array_equal(band32, ES.placed_in_band(b, ES.F32_BAND)) and band32.sum() > band64.sum()

    # NaN exactly in slot j's d_cpa column of the parallel-flight cases; the reward stays finite even at slot 0
    # (v_closing is 0 and min(1, nan ** 4) == 1, rewards.py:16), as in the reference's own fixtures
    assert np.array_equal(np.isnan(ref.obs), ES.expected_nan_columns(b))
    assert np.isfinite(ref.reward).all()
    for j in range(N):
        assert ((fam == "parallel") & (ES.labels(b, "nan_slot") == j)).any()

    # mirror headings: |v12x| < 1e-9 at the mirror slot and nowhere else (the FAST d_cpa sign rule's set)
    r = lambda deg: deg / 360.0 * 2 * np.pi  # noqa: E731
    v12x = ref.own_v[:, None] * np.cos(r(ref.own_psi))[:, None] - ref.trf_v * np.cos(r(ref.trf_psi))
    v12y = ref.own_v[:, None] * np.sin(r(ref.own_psi))[:, None] - ref.trf_v * np.sin(r(ref.trf_psi))
    mirror = np.zeros_like(d, bool)
    ms = ES.labels(b, "mirror_slot").astype(int)
    mirror[np.nonzero(ms >= 0)[0], ms[ms >= 0]] = True
    parallel = ES.expected_nan_columns(b)[:, 6::3]
    assert np.array_equal(np.abs(v12x) < 1e-9, mirror | parallel)
    assert (np.hypot(v12x, v12y)[~(mirror | parallel)] > 2.0).all()

    # injected traffic headings: the step wraps them as aircraft.py:22 does
    inj = np.nonzero(fam == "injected")[0]
    slot = ES.labels(b, "slot").astype(int)[inj]
    h = ES.labels(b, "offset").astype(float)[inj]
    got = ref.trf_psi[inj, slot]
    assert np.array_equal(got, np.mod(h + 0.0, 360.0)) and ((got >= 0) & (got < 360)).all()
    hair = h == -2.0 ** -40
    assert hair.any() and (got[hair] == 360.0 - 2.0 ** -40).all() and (f32(got[hair]) == 360.0).all()
    assert set(h) == set(ES.INJECTED_HEADINGS) and len(set(slot)) == N

    # outcomes: is_done() -- timeout > collision > goal (acas2d_oracle.c, game.py:294-314) -- outside the band
    steps_in = b.steps
    want = np.where(steps_in + 1 > M, 3, np.where(coll_off < 0, 2, np.where(goal_off < 0, 1, 0)))
    ok = ~band64
    assert np.array_equal(ref.outcome[ok], want[ok]) and np.array_equal(ref.status[ok], want[ok])
    to = fam == "timeout"
    assert {(int(s), int(o)) for s, o in zip(steps_in[to], ref.outcome[to])} >= {(M - 2, 0), (M - 2, 1), (M - 2, 2),
                                                                                   (M, 3), (M + 1, 3), (M - 1, 2)}
    assert (ref.outcome[fam == "goal+collision"] == 2).all()
    # the fillers are calm: nothing ends there
    assert (ref.outcome[b.case < 0] == 0).all()
