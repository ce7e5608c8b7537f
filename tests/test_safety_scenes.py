"""The safety-statistics scenes and their reference (tests/safety_ref.py) in the CPU oracle alone: every scene does what
its label says, the exact scenes give exactly the expected integers, the criteria of tests/test_eval_stats_oracle.py decide
nearly every episode by equality, and the comparison sees the classic mistake (traffic taken after its move).  So the GPU
test cannot pass vacuously."""
import functools

import numpy as np
import pytest

import helpers as H
import safety_ref as S

_CASES = [(N, "default") for N in (1, 2, 3, 4, 8, 16, 32, 64)] + [(3, "small"), (16, "small")]
GOAL_FAMILIES = ("nearest", "goal", "receding", "first_goal")
EXACT_FAMILIES = ("tie", "threshold", "twin")            # goal episodes when flown straight (b = 0), 24 .. 70 steps long


@functools.lru_cache(maxsize=None)
def _case(N, name):
    import gym_acas2d_amd as g
    from oracle import oracle as O
    O.build()
    cfg = S.config(g, N, name)
    sc = S.scenes(cfg, O)
    actions = S.cpu_actions(sc, cfg.max_steps + 1)
    ref = S.reference(O, H, g, cfg, sc, actions)
    D = S.drift(O, H, cfg, sc, actions, ref)
    return g, O, cfg, sc, actions, ref, D


def _as_got(ref, stats, npdt=np.float64):
    got = {k: (v if v.dtype.kind == "i" else v.astype(npdt)) for k, v in stats.items()}
    got.update(outcome=ref.outcome, steps=ref.steps)
    return got


@pytest.mark.parametrize("N,config", _CASES, ids=["N%d-%s" % c for c in _CASES])
def test_scenes_do_what_their_labels_say(oracle_mod, N, config):
    g, O, cfg, sc, actions, ref, D = _case(N, config)
    fam, E = sc.family, len(sc.family)
    s, sd, cd = S.step_len(cfg), float(cfg.safe_distance), 2.0 * cfg.collision_radius
    assert E <= 160 and cfg.max_steps <= 120 and ref.outcome.shape == (S.K, E)
    assert np.array_equal(S.f32(sc.own), sc.own) and np.array_equal(S.f32(sc.trf), sc.trf)
    exact = S.exact_scenes_hold(cfg)
    assert exact                                                     # (both configs of this file have exact step lengths)
    assert set(fam) == {"nearest", "goal", "collision", "timeout", "receding", "first_goal", "first_collision", "tie",
                        "threshold", "twin", "nan"}

    # outcomes per family, under every policy, and thresholds a good margin away
    for k in range(S.K):
        oc, st = ref.outcome[k], ref.steps[k]
        assert (oc[np.isin(fam, GOAL_FAMILIES)] == H.GOAL).all(), k
        assert (oc[np.isin(fam, EXACT_FAMILIES)] == H.GOAL).all() or k > 0
        assert (oc[np.isin(fam, ("collision", "first_collision"))] == H.COLLISION).all(), k
        assert (oc[np.isin(fam, ("timeout", "nan"))] == H.TIMEOUT).all(), k
        assert (st[np.isin(fam, ("timeout", "nan"))] == cfg.max_steps + 1).all()
        assert (st[np.isin(fam, ("first_goal", "first_collision"))] == 2).all()        # one step row
        assert (st[fam == "nearest"] <= 19).all() and (st[fam == "nearest"] >= 6).all()
        coll = fam == "collision"                                    # a collision's minimum is on its last row
        assert np.array_equal(ref.stats["min_separation_step"][k][coll], st[coll] - 1)
        assert (ref.stats["min_separation_step"][k][fam == "receding"] == 1).all()
        assert (ref.stats["los_steps"][k][fam == "nearest"] == st[fam == "nearest"] - 1).all()   # every row inside
        assert (ref.stats["los_steps"][k][fam == "timeout"] == 0).all()
    const = slice(0, 3)
    assert np.nanmin(ref.margin[const]) >= S.MARGIN * s
    short = np.isin(fam, GOAL_FAMILIES)                              # under ANY actions (full deflection, the random walk)
    assert np.nanmin(ref.margin[:, short]) >= 0.2 * s, np.nanmin(ref.margin[:, short])
    print("N=%d %s: E=%d, least threshold margin %.3f px (constant policies) / %.3f px (random walk)"
          % (N, config, E, np.nanmin(ref.margin[const]), np.nanmin(ref.margin[3])))
    assert np.isnan(ref.margin[:, fam == "nan"]).all() and np.isfinite(ref.margin[:, fam != "nan"]).all()
    # a NaN nowhere but in the nan scenes: every row of every other episode is finite
    rows = S.step_rows(ref)
    other = rows & (fam != "nan")[None, None, :]
    assert np.isfinite(ref.d_sep[other]).all() and np.isfinite(ref.d_dev[other]).all() and np.isfinite(ref.a_lat[other]).all()

    # nearest-at-slot j: aircraft j attains the minimum, no other within 10 px of it; every slot is held at least once
    near = np.nonzero(fam == "nearest")[0]
    assert set(sc.slot[near]) == set(range(N))
    env = O.OracleEnvs(E, N, auto_reset=False, config=H.oracle_config(O, cfg))
    for k in (0, 2, 3):
        env.set_state(sc.own, sc.trf, sc.goal)
        env.observe()
        best = np.full((E, N), np.inf)
        for t in range(int(ref.steps[k][near].max()) - 1):
            tx, ty = env.trf_x.copy(), env.trf_y.copy()
            env.step(actions[k][t])
            d = np.hypot(env.own_x[:, None] - tx, env.own_y[:, None] - ty)
            best = np.where((t + 2 <= ref.steps[k])[:, None], np.minimum(best, d), best)
        b = best[near]
        at = b[np.arange(len(near)), sc.slot[near]]
        assert np.array_equal(at, ref.stats["min_separation"][k][near])
        b[np.arange(len(near)), sc.slot[near]] = np.inf
        assert (b.min(1) > at + 10).all()                              # (+inf at N = 1)
        assert (at > cd + 5).all() and (at < sd - 5).all()

    # the exact scenes, under the b = 0 policy: exactly the expected numbers
    z = ref.stats["min_separation_step"][0]
    for f in ("tie", "threshold", "twin"):
        assert (fam == f).sum() == 2 and (z[fam == f] == S.TIE_ROW).all()
        assert (ref.stats["max_abs_a_lat"][0][fam == f] == 0).all() and (ref.stats["max_abs_deviation"][0][fam == f] == 0).all()
        assert (ref.steps[0][fam == f] > S.TIE_ROW + 4).all()
    tie = fam == "tie"
    ties = (ref.d_sep[0][:, tie] == ref.stats["min_separation"][0][tie]).sum(0)
    assert (ties == 2).all() and (ref.d_sep[0][S.TIE_ROW, tie] == ref.d_sep[0][S.TIE_ROW + 1, tie]).all()
    assert (ref.d_sep[0][S.TIE_ROW, fam == "threshold"] == sd).all()
    assert (ref.stats["min_separation"][0][fam == "threshold"] == sd).all()
    assert (ref.stats["los_steps"][0][tie | (fam == "threshold")] == 0).all()
    assert (ref.stats["los_steps"][0][fam == "twin"] == 1).all()
    nan = fam == "nan"
    assert set(sc.slot[nan]) == {0, N - 1}
    env.set_state(sc.own, sc.trf, sc.goal)
    first = env.observe()
    want = np.zeros_like(first, bool)
    want[np.nonzero(nan)[0], 5 + 3 * sc.slot[nan] + 1] = True       # NaN exactly in the d_cpa entry of the parallel aircraft
    assert np.array_equal(np.isnan(first), want)
    for k in range(S.K):
        assert np.isposinf(ref.stats["min_separation"][k][nan]).all() and np.isnan(ref.stats["mean_abs_deviation"][k][nan]).all()
        for key in ("min_separation_step", "los_steps", "max_abs_a_lat", "max_abs_deviation"):
            assert (ref.stats[key][k][nan] == 0).all(), key
    S.assert_exact_scenes(_as_got(ref, ref.stats), sc, cfg, np.float64)


@pytest.mark.parametrize("config", ["default", "small"])
def test_exact_scenes_are_exact_in_float32(config):
    """A NumPy float32 restatement of the position updates of the tie / threshold scenes: every position, difference and
    squared distance of the rows up to the tie is exact, so float32 and float64 see the same numbers."""
    g, O, cfg, sc, actions, ref, D = _case(3, config)
    f = np.float32
    v, dt, one, zero = f(cfg.airspeed), f(cfg.dt), f(1), f(0)
    s = S.step_len(cfg)
    if config == "default":
        assert f(100) * f(0.01) == 1
    # the step in any association of v, cos(0) = 1 and dt, at full and at half airspeed
    for vv, want in ((v, s), (f(0.5) * v, s / 2)):
        for step in ((vv * one) * dt, vv * (one * dt), (vv * dt) * one):
            assert step.dtype == np.float32 and float(step) == want
        assert float(vv * zero * dt) == 0.0                          # sin(0): y does not move
    sd = float(cfg.safe_distance)
    for fam in ("tie", "threshold", "twin"):
        for i in np.nonzero(sc.family == fam)[0]:
            j = sc.slot[i]
            x, y, tx, ty = f(sc.own[i, 0]), f(sc.own[i, 1]), f(sc.trf[i, j, 0]), f(sc.trf[i, j, 1])
            x64, tx64 = float(x), float(tx)
            assert float(x).is_integer() and float(y).is_integer() and sc.own[i, 2] == 0 and sc.trf[i, j, 2] == 0
            assert float(f(sc.trf[i, j, 3])) == cfg.airspeed / 2
            d2 = []
            for row in range(1, S.TIE_ROW + 3):
                x = x + v * dt                                       # the player moves, the traffic not yet
                x64 += s
                dx, dy = x - tx, y - ty
                assert float(x) == x64 and float(tx) == tx64 and float(dx) == x64 - tx64
                sq = f(float(dy) * float(dy) + float(dx) * float(dx))                  # fma(dy, dy, dx * dx): one rounding
                d2.append(float(sq))
                if fam != "twin":                                    # (the twin's dy = safe_distance - 2^-10 squares inexactly)
                    assert float(sq) == float(dy) ** 2 + float(dx) ** 2                # ... which rounds nothing
                    assert float(dx * dx) == float(dx) ** 2 and float(dy * dy + dx * dx) == float(sq)
                    assert np.sqrt(f(sq)).astype(np.float64) == f(ref.d_sep[0][row, i])
                tx = tx + f(0.5) * v * dt
                tx64 += s / 2
            if fam == "tie":
                assert d2[S.TIE_ROW - 1] == d2[S.TIE_ROW] == min(d2) and d2.count(min(d2)) == 2
            elif fam == "threshold":
                assert d2[S.TIE_ROW - 1] == sd * sd == min(d2) and d2.count(min(d2)) == 1
                assert np.sqrt(f(d2[S.TIE_ROW - 1])) == f(sd)
            else:
                assert np.sqrt(f(d2[S.TIE_ROW - 1])) < f(sd) and sorted(d2)[1] > sd * sd


@pytest.mark.parametrize("N,config", _CASES, ids=["N%d-%s" % c for c in _CASES])
def test_criteria_decide_by_equality_and_see_the_classic_mistake(oracle_mod, N, config):
    g, O, cfg, sc, actions, ref, D = _case(N, config)
    fam, sd, rows = sc.family, float(cfg.safe_distance), cfg.max_steps
    B32 = S.bound(H, "float32", rows, ref.extent, D)
    assert B32 >= 4 * D and B32 >= rows * 1.3e-4 and B32 < 0.1
    print("N=%d %s: D = %.3e px, extent %.0f px, B(float32) = %.4e px, B(float64 FAST) = %.2e px"
          % (N, config, D, ref.extent, B32, S.bound(H, "float64fast", rows)))
    for build, B in (("float32", B32), ("float64fast", S.bound(H, "float64fast", rows)), ("float64", S.bound(H, "float64", rows))):
        unique, same = S.decided(ref, B, sd)
        fin = fam != "nan"                                            # (a nan episode has no finite row: its index must be 0)
        assert unique[:, fin].mean() >= 0.90 and same.mean() >= 0.95, (build, unique[:, fin].mean(), same.mean())
        for f in set(fam) - {"nan"}:
            assert unique[:, fam == f].any() and same[:, fam == f].any(), (build, f)
        assert not S.candidates(ref, B)[:, :, ~fin].any()
        # the reference passes its own comparison
        err = S.compare(_as_got(ref, ref.stats), ref, cfg, B, np.float64)
        assert err["min_separation"] == 0 and err["episodes"] == S.K * len(fam)
    # the exact scenes under b = 0 are the ones the criteria cannot decide: both rows of a tie are candidates, and a row
    # exactly at the threshold lies between the two counts -- those are asserted exactly instead
    unique, same = S.decided(ref, 1e-9, sd)
    assert not unique[0, fam == "tie"].any() and not same[0, fam == "threshold"].any()
    assert unique[0, fam == "threshold"].all() and same[0, fam == "tie"].all() and same[0, fam == "twin"].all()

    # the deliberately wrong reference: d_sep from the traffic AFTER its move
    wrong = [S.run(O, H, cfg, sc, a, traffic="after") for a in actions]
    stats = [S.reduce_rows(g, cfg, r) for r in wrong]
    wstats = {k: np.stack([s[k] for s in stats]) for k in stats[0]}
    near = fam == "nearest"
    diff = np.abs(wstats["min_separation"][:, near] - ref.stats["min_separation"][:, near])
    assert (diff > 4 * B32).mean() >= 0.5, (diff > 4 * B32).mean()
    with pytest.raises(AssertionError):
        S.compare(_as_got(ref, wstats), ref, cfg, B32, np.float64)
    # ... and a step index off by one row, a loss of separation counted with <=, a maximum that starts from the first row
    for key, delta in (("min_separation_step", 1), ("los_steps", 1)):
        bad = dict(ref.stats)
        bad[key] = ref.stats[key] + delta
        with pytest.raises(AssertionError):
            S.compare(_as_got(ref, bad), ref, cfg, B32, np.float64)
