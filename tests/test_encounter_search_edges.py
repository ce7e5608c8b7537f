"""The three kernels of csrc/acas2d_search.hip, each called on its own with hand-placed inputs (tests/encounter_search_edges.py)
and held to the NumPy specification (records.search_*): candidate counts on the edges of the wave, the 128- and 256-thread
blocks and the 64-env padding, K = 3 with a different pattern per row.  Every comparison is bitwise except two: exp() and
log() within 4 ulp of NumPy's (both libraries document 1 ulp), and the weighted sums within n 2^-53 relative of math.fsum of
the device's own weights (n positive addends in any order); the worst seen of either is printed.  The last test grows the
Python log of policy.EncounterSearch past its first 8 rows."""
import math

import numpy as np
import pytest

import encounter_search_edges as E
import encounter_search_support as S

pytestmark = pytest.mark.gpu
SIZES = pytest.mark.parametrize("L", E.LS)
DTYPE = pytest.mark.parametrize("dtype", sorted(E.DTYPES))
SAMPLER_CASES = E.sampler_cases()
ARCHIVE_CASES = E.archive_cases()


@pytest.fixture(scope="module")
def g():
    import gym_acas2d_amd as g
    return g


@pytest.fixture(scope="module")
def O(oracle_mod):
    return oracle_mod


def log_row(row, generation):
    return np.concatenate([row[:12], [float(generation), 0.0, 0.0, 0.0]])


# ---- select -----------------------------------------------------------------------------------------------------------------
@SIZES
@DTYPE
def test_select_placed_scores(g, L, dtype):
    """weighted = 0: elite_w, the whole log row (twelve columns, the generation, three zeros) and with it gamma_q, the
    counts and the argmin (the lowest index of a tie) equal the specification bit for bit, for every score pattern,
    n_quantile and level."""
    R = g.records
    d = E.Direct(g, L, 1, 8, dtype)
    for n, case in enumerate(E.select_cases(L, dtype)):
        generation = n if n % 2 == 0 else 2 ** 32 - 1 - n
        d.put(min_sep=case.sep, outcome=case.outcome).fill("elite_w", -5.0).fill("history", -9.0)
        d.select(case.n_quantile, case.level, 0, generation=generation)
        elite_w, history = d.get("elite_w", "history")
        for k in range(E.K):
            sel = R.search_select(case.sep[k], case.outcome[k], np.zeros(L), case.n_quantile, case.level, False)
            assert E.bits_equal(elite_w[k], sel["elite_w"]), (case.label, k)
            assert E.bits_equal(history[k], log_row(sel["row"], generation)), (case.label, k, history[k], sel["row"])


@SIZES
@DTYPE
def test_select_weighted(g, L, dtype):
    """weighted = 1 with log_w in [-30, 30].  The batch whose candidates are all elite gives the device's weight of every
    candidate: within 4 ulp of np.exp(log_w).  In every batch elite_w is that weight on the specification's elite and 0
    elsewhere, the counts, thresholds and argmin are exact, and columns 6 .. 9 lie within n 2^-53 relative of math.fsum of
    the device's weights.  With log_w = 0 the sums are exact and the whole row is compared bitwise."""
    R, dt = g.records, E.DTYPES[dtype]
    cases = E.weighted_cases(L, dtype)
    d = E.Direct(g, L, 1, 8, dtype)
    W = None
    worst_ulp = worst_sum = 0.0
    for n, case in enumerate(cases):
        d.put(min_sep=case.sep, outcome=case.outcome, log_w=case.log_w).fill("elite_w", -5.0).fill("history", -9.0)
        d.select(case.n_quantile, case.level, 1, generation=n)
        elite_w, history = d.get("elite_w", "history")
        if n == 0:
            W = elite_w.copy()
            assert (W > 0).all()                                 # every candidate is elite: elite_w holds every weight
            worst_ulp = float(S.ulps(W, np.exp(case.log_w)).max())
            print("exp(log_w) against NumPy, L = %d: worst %.2f ulp" % (L, worst_ulp))
            assert worst_ulp <= 4.0
        for k in range(E.K):
            sel = R.search_select(case.sep[k], case.outcome[k], case.log_w[k], case.n_quantile, case.level, True)
            row, h = sel["row"], history[k]
            if case.exact:
                assert E.bits_equal(elite_w[k], sel["elite_w"]) and E.bits_equal(h, log_row(row, n)), (case.label, k, h, row)
                continue
            assert E.bits_equal(elite_w[k], np.where(sel["elite"], W[k], 0.0)), (case.label, k)
            assert E.bits_equal(h[:6], row[:6]) and E.bits_equal(h[10:], log_row(row, n)[10:]), (case.label, k, h, row)
            ev = sel["score"] <= dt(case.level)
            w, w2 = W[k], W[k] * W[k]
            for col, ref, terms in ((6, math.fsum(w[ev]), ev.sum()), (7, math.fsum(w2[ev]), ev.sum()), (8, math.fsum(w), L),
                                    (9, math.fsum(w2), L)):
                err = abs(h[col] - ref) / ref if ref else abs(h[col])
                worst_sum = max(worst_sum, err / E.EPS)
                assert err <= terms * E.EPS, (case.label, k, col, err / E.EPS, terms)
    print("weighted sums against math.fsum of the device's weights, L = %d: worst %.2f x 2^-53 relative" % (L, worst_sum))


@pytest.mark.parametrize("case", ARCHIVE_CASES, ids=[c.label for c in ARCHIVE_CASES])
def test_archive(g, O, case):
    """Five select calls on the same buffers.  A call in which nothing finished leaves the archive as it is (empty at first:
    best_candidate -1); an equal minimum a generation later keeps the first; a strictly smaller one replaces it.  After
    each replacement best_own_psi and best_traffic are the specification's draw of that candidate from the tables passed in
    THAT call, bit for bit -- at N = 64 thread 64, in the second wave, draws traffic 63."""
    R, dt = g.records, E.DTYPES[case.dtype]
    cfg = E.search_config(g, case.N)
    active = R.search_active_coordinates(cfg)
    d = E.Direct(g, case.L, case.N, case.B, case.dtype, config=cfg)
    flat = np.full((E.K, d.NC, case.B), 1.0 / case.B)
    first = E.random_tables(R, d.NC, case.B, E.case_rng(case.N, 1)) if case.nonflat else (flat,) + R.search_tables(flat)
    second = E.random_tables(R, d.NC, case.B, E.case_rng(case.N, 2))
    names = ("best_score", "best_generation", "best_candidate", "best_own_psi", "best_traffic")
    steps, _ = E.archive_steps(case)
    for n, st in enumerate(steps):
        tables = second if st.second_tables else first
        before = d.get(*names)
        d.tables(tables).put(min_sep=st.sep, outcome=st.outcome)
        d.select(E.middle(case.L), 0.0, 0, generation=st.generation, seed=case.seed, env_offset=case.offset)
        after = dict(zip(names, d.get(*names)))
        if not st.replaces:
            assert all(E.bits_equal(a, b) for a, b in zip(before, after.values())), (st.name, before, after)
            if n == 0:
                assert after["best_candidate"].tolist() == [-1] * E.K and np.isposinf(after["best_score"]).all()
            continue
        for k in range(E.K):
            cand = int(np.argmin(st.sep[k]))
            assert after["best_score"][k] == st.sep[k, cand] and after["best_candidate"][k] == cand, (st.name, k)
            assert after["best_generation"][k] == st.generation, (st.name, k)
            u = E.uniforms(O, case.N, st.generation, 1, case.offset + cand, case.seed)
            c, _, _ = R.search_sample(tuple(t[k] for t in tables), active, u)
            own, trf, _ = R.encounter_from_uniforms(cfg, c, dt)
            assert E.bits_equal(after["best_own_psi"][k], own[0, 2]), (st.name, k)
            assert E.bits_equal(after["best_traffic"][k], trf[0]), (st.name, k)
    assert d.get("best_generation").tolist() == [steps[3].generation] * E.K


# ---- refit ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", E.REFIT_SIZES, ids=["B%d-L%d-N%d" % s for s in E.REFIT_SIZES])
def test_refit_placed_bins(g, size):
    """Dyadic weights: p and cdf equal records.search_refit() / search_tables() bit for bit and log_ratio within 4 ulp, for
    every alpha and p_floor; a row whose policy has no elite weight or whose coordinate is inactive keeps its sentinel in
    all three tables."""
    R = g.records
    B, L, N = size
    d = E.Direct(g, L, N, B, "f64")
    worst = 0.0
    cases = [c for c in E.refit_cases(g) if (c.B, c.L, c.N) == size]
    assert cases
    for case in cases:
        want_p, want_cdf, want_lr, touched = E.refit_expected(R, case)
        cdf0, lr0 = E.sentinel_tables(want_cdf.shape, want_lr.shape)
        d.put(p=case.p0, cdf=cdf0, log_ratio=lr0, bins=case.bins, elite_w=case.w)
        d.refit(case.alpha, case.p_floor)
        p, cdf, lr = d.get("p", "cdf", "log_ratio")
        assert E.bits_equal(p, want_p), (case.label, np.argwhere(p != want_p)[:4])
        assert E.bits_equal(cdf, want_cdf), case.label
        assert E.bits_equal(lr[~touched], lr0[~touched]), case.label
        worst = max(worst, float(S.ulps(lr[touched], want_lr[touched]).max()) if touched.any() else 0.0)
        assert worst <= 4.0, case.label
        assert E.bits_equal(np.isposinf(lr), np.isposinf(want_lr))
    print("log_ratio against NumPy, B = %d, L = %d, N = %d: worst %.2f ulp" % (B, L, N, worst))


# ---- sampler ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SAMPLER_CASES, ids=[c.label for c in SAMPLER_CASES])
@DTYPE
def test_sampler_placed_tables(g, O, case, dtype):
    """From placed tables (flat, refit rows with empty bins, a bin of mass 2^-40, cdf edges equal to a candidate's uniform,
    the 0 / 0 of a tie on an empty last bin), 64-bit seeds and offsets and the last generation: the bins, log_w and every
    state array of every real lane equal the specification bit for bit; the padding lanes repeat candidate 0; steps and
    total_reward are 0; nothing is written behind the real candidates' bins and log_w."""
    R, dt, L = g.records, E.DTYPES[dtype], case.L
    ref = E.sampler_reference(g, O, case)
    cfg = E.search_config(g, case.N)
    d = E.Direct(g, L, case.N, case.B, dtype, config=cfg).tables(ref["tables"]).fill("bins", 0xEE).fill("log_w", -123.0)
    own, trf, goal, steps, reward = d.sample(case.generation, case.seed, case.offset)
    bins, log_w = d.get("bins", "log_w")
    pad = own.shape[1] - L
    assert pad == (-L) % 64
    for k in range(E.K):
        wo, wt, wg = R.encounter_from_uniforms(cfg, ref["c"][k], dt)
        assert np.array_equal(bins[k], ref["bins"][k].T), (k, np.argwhere(bins[k] != ref["bins"][k].T)[:4])
        assert E.bits_equal(log_w[k], ref["log_w"][k]), k
        assert E.bits_equal(own[k, :L], wo) and E.bits_equal(trf[k, :L], wt) and E.bits_equal(goal[k, :L], wg), k
        assert E.bits_equal(own[k, L:], np.repeat(wo[:1], pad, 0)) and E.bits_equal(trf[k, L:], np.repeat(wt[:1], pad, 0)), k
        assert E.bits_equal(goal[k, L:], np.repeat(wg[:1], pad, 0)), k
    assert not steps.any() and not reward.any() and not np.signbit(reward).any()
    assert (d.guard("bins") == 0xEE).all() and (d.guard("log_w") == -123.0).all()


# ---- the Python log ---------------------------------------------------------------------------------------------------------
def test_the_log_grows(g):
    """EncounterSearch's log starts with 8 rows and doubles: run(9) equals run(5), state_dict(), a new object, run(4) in
    every buffer, bit for bit; the log has nine rows and its generation column counts 0 .. 8."""
    s = S.SHAPES[5]
    assert s.dtype == S.F32 and s.N == 1 and s.max_steps == 150 and S.CANDIDATES == 70
    whole = S.search(g, s).run(9)
    first = S.search(g, s).run(5)
    resumed = S.search(g, s).load_state_dict(first.state_dict()).run(4)
    want, got = whole.buffers(), resumed.buffers()
    bad = S.mismatches(got, want)
    assert not bad, bad
    for es in (whole, resumed):
        h = es.history()
        assert h.shape == (9, 3, 16) and es.generation == 9
        assert E.bits_equal(h[:, :, 12], np.repeat(np.arange(9.0)[:, None], 3, 1)) and not h[:, :, 13:].any()
        assert (h[:, :, 0] + h[:, :, 1] == S.CANDIDATES).all()
