"""The hand-placed cases of tests/encounter_search_edges.py, host side (no GPU): every case is what its label says, so the GPU
test cannot pass vacuously; and records.search_select() against a plain Python rewrite (sorted, comprehensions, math.fsum) on
every select case, so the specification's own handling of ties, NaN, unfinished episodes and the empty elite is held too."""
import math

import numpy as np
import pytest

import encounter_search_edges as E

SIZES = pytest.mark.parametrize("L", E.LS)
DTYPE = pytest.mark.parametrize("dtype", sorted(E.DTYPES))


@pytest.fixture(scope="module")
def g():
    import gym_acas2d_amd as g
    return g


@pytest.fixture(scope="module")
def O(oracle_mod):
    return oracle_mod


def high_word(a):
    return E._bits(a) >> np.uint64(32)


def key_byte(a, byte):
    """Byte `byte` (0 = the lowest) of the ordered key of positive floats: the bits themselves."""
    return (E._bits(a).astype(np.uint64) >> np.uint64(8 * byte)) & np.uint64(255)


# ---- select -----------------------------------------------------------------------------------------------------------------
def plain_select(sep, outcome, weights, n_quantile, level):
    """records.search_select() again in plain Python on lists of floats; weights: W of every candidate."""
    inf = math.inf
    s = [x if (o != 0 and x == x) else inf for x, o in zip(sep, outcome)]
    gamma_q = sorted(s)[n_quantile - 1]
    gamma = max(gamma_q, level)
    elite = [x <= gamma and math.isfinite(x) for x in s]
    event = [x <= level for x in s]
    low = min(s)
    return {"score": s, "elite": elite, "elite_w": [w if e else 0.0 for w, e in zip(weights, elite)],
            "row": [sum(o != 0 for o in outcome), sum(o == 0 for o in outcome), sum(elite), gamma_q, gamma, sum(event),
                    math.fsum(w for w, e in zip(weights, event) if e), math.fsum(w * w for w, e in zip(weights, event) if e),
                    math.fsum(weights), math.fsum(w * w for w in weights), low, s.index(low), 0.0, 0.0, 0.0, 0.0]}


def check_against_plain(R, sep, oc, log_w, nq, level, weighted):
    dt = sep.dtype.type
    sel = R.search_select(sep, oc, log_w, nq, level, weighted)
    w = np.exp(log_w).tolist() if weighted else [1.0] * len(sep)
    want = plain_select([float(x) for x in sep], oc.tolist(), w, nq, float(dt(level)))
    assert sel["score"].dtype == sep.dtype and sel["score"].tolist() == want["score"]
    assert sel["elite"].tolist() == want["elite"] and sel["elite_w"].tolist() == want["elite_w"]
    assert E.bits_equal(sel["row"], np.array(want["row"], np.float64)), (sel["row"], want["row"])
    return sel


@SIZES
@DTYPE
def test_select_cases_are_what_they_say(g, L, dtype):
    R, dt = g.records, E.DTYPES[dtype]
    cases = E.select_cases(L, dtype)
    seen, levels, nqs, tie_checked = set(), set(), set(), 0
    for case in cases:
        assert case.sep.shape == case.outcome.shape == (E.K, L) and case.sep.dtype == dt and case.outcome.dtype == np.uint8
        assert len(set(case.kinds)) == E.K and 1 <= case.n_quantile <= L
        assert not (np.signbit(case.sep) & (case.sep == 0)).any()                    # no -0.0
        assert not np.isneginf(case.sep).any()
        assert float(dt(case.level)) == case.level                                  # the level is a number of the dtype
        for k, kind in enumerate(case.kinds):
            sep, oc = case.sep[k], case.outcome[k]
            sel = check_against_plain(R, sep, oc, np.zeros(L), case.n_quantile, case.level, False)
            s, fin = sel["score"], np.isfinite(sel["score"])
            seen.add((k, kind))
            if kind == "distinct":
                assert len(np.unique(sep)) == L and oc.all() and (L < 3 or (np.diff(sep) < 0).any() and (np.diff(sep) > 0).any())
            elif kind == "all_equal":
                assert len(np.unique(sep)) == 1 and sel["row"][11] == 0 and sel["row"][2] == L
            elif kind == "tie":
                nq, srt = case.n_quantile, np.sort(s)
                at = np.nonzero(s == srt[nq - 1])[0]
                assert len(at) == len(E.tie_ranks(L, nq)) and sel["row"][3] == srt[nq - 1]
                if 1 < nq < L:                                   # copies on both sides of the rank: the elite outgrows n_quantile
                    assert srt[nq - 2] == srt[nq - 1] == srt[nq] and sel["row"][2] > nq
                    assert len(set(at % 64)) >= min(len(at), 3) and len(set(at % 256)) >= min(len(at), 3)
                    assert L <= 64 or len(set((at % 256) // 64)) >= 2          # ... in different waves
                    assert L <= 262 or {6, 262} <= set(at.tolist())            # ... and twice in one thread
                    tie_checked += 1
            elif kind == "min_tie":
                at = np.nonzero(s == s.min())[0]
                assert len(at) == min(4, L) and sel["row"][11] == at.min()
                assert L <= 262 or ({6, 262} <= set(at.tolist()) and len(set((at % 256) // 64)) >= 3)
            elif kind == "low_byte":
                assert len(np.unique(E._bits(sep) >> 8)) == 1 and (L < 63 or len(np.unique(key_byte(sep, 0))) > 32)
            elif kind == "top_byte":
                top = sep.dtype.itemsize - 1
                assert len(np.unique(E._bits(sep) & ((1 << 8 * top) - 1))) == 1 and fin.all() and (sep > 0).all()
                assert L < 2 or {0, 127} <= set(key_byte(sep, top).tolist())
            elif kind == "high_word_equal":
                assert dtype == "f64" and len(np.unique(high_word(sep))) == 1 and len(np.unique(sep)) == L
            elif kind == "zeros_denormals":
                tiny = np.finfo(dt).tiny
                assert (sep >= 0).all() and (L < 63 or ((sep == 0).any() and ((sep > 0) & (sep < tiny)).any() and (sep >= tiny).any()))
            elif kind == "inf_finished":
                assert oc.all() and (L < 2 or np.isposinf(sep).any()) and (L < 3 or np.isposinf(sep[0]))
            elif kind == "nan":
                assert oc.all() and (L < 3 or (np.isnan(sep).any() and np.isnan(sep[0]) and np.isposinf(s[0])))
            elif kind == "some_unfinished":
                assert (L < 8 or ((oc == 0).any() and (oc != 0).any())) and np.isfinite(sep).all()
                assert L < 8 or sep[oc == 0].min() < sep[oc != 0].min()              # the closest never finished: it must not count
            elif kind == "all_unfinished":
                assert not oc.any() and np.isfinite(sep).all() and not sel["elite"].any() and sel["row"][3] == np.inf
                assert sel["row"][10] == np.inf and sel["row"][11] == 0
            elif kind == "negative":
                assert L < 3 or ((sep < 0).any() and (sep > 0).any())
            else:
                raise AssertionError(kind)
        s = E.effective(case.sep[case.level_row], case.outcome[case.level_row])
        gq = np.sort(s)[case.n_quantile - 1]
        lv = dt(case.level)
        if case.level_kind == "below":
            assert (s > lv).all()
        elif case.level_kind == "equal":
            assert (s == lv).any() or not np.isfinite(s).any()
        elif case.level_kind == "between":
            # (with one finite value only: between it and +inf)
            assert not (s == lv).any() and np.isfinite(lv) and ((s < lv).any() or not np.isfinite(s).any())
        elif case.level_kind == "above":
            assert lv > gq or np.isposinf(gq)
        else:
            assert np.isposinf(lv)
        levels.add(case.level_kind)
        nqs.add(case.n_quantile)
    assert {kind for _, kind in seen} == set(E.SELECT_KINDS[dtype]) and levels == set(E.LEVEL_KINDS)
    assert nqs == {1, E.middle(L), L} and (L < 63 or tie_checked > 0)
    assert len({c.label for c in cases}) == len(cases)


def test_every_pattern_meets_every_row():
    """Over the candidate counts the rotation puts every score pattern into every policy row."""
    for dtype, kinds in E.SELECT_KINDS.items():
        seen = {(k, kind) for L in E.LS for case in E.select_cases(L, dtype) for k, kind in enumerate(case.kinds)}
        assert seen == {(k, kind) for k in range(E.K) for kind in kinds}


@SIZES
@DTYPE
def test_weighted_cases(g, L, dtype):
    R = g.records
    cases = E.weighted_cases(L, dtype)
    lw = cases[0].log_w
    assert lw.min() == (-30.0 if L > 1 else 30.0) and lw.max() == 30.0 and (np.abs(lw) <= 30.0).all()
    assert L < 3 or ((lw == 0.0).any() and not E.bits_equal(lw[0], lw[1]))
    first = cases[0]
    assert first.n_quantile == L and first.outcome.all() and np.isfinite(first.sep).all()
    for k in range(E.K):
        sel = check_against_plain(R, first.sep[k], first.outcome[k], lw[k], L, first.level, True)
        assert sel["elite"].all() and E.bits_equal(sel["elite_w"], np.exp(lw[k]))    # elite_w holds every weight
    for case in cases[1:]:
        assert E.bits_equal(case.log_w, np.zeros_like(lw) if case.exact else lw)
        for k in range(E.K):
            check_against_plain(R, case.sep[k], case.outcome[k], case.log_w[k], case.n_quantile, case.level, True)
    assert cases[-1].exact and [c.exact for c in cases[:-1]] == [False] * 3


# ---- refit ------------------------------------------------------------------------------------------------------------------
def test_refit_cases_are_what_they_say(g):
    R = g.records
    cases = E.refit_cases(g)
    seen = set()
    zeros = flat_steps = infs = rounded = 0
    for case in cases:
        B, L, NC = case.B, case.L, case.active.size
        assert case.bins.shape == (E.K, NC, L) and case.bins.dtype == np.uint8 and case.w.shape == (E.K, L) and NC == 4 * (case.N + 1)
        m = case.w * 1024.0
        assert (m == np.floor(m)).all() and (m < 2 ** 20).all() and (case.w >= 0).all()         # dyadic: every sum is exact
        assert not E.bits_equal(case.p0, np.full_like(case.p0, 1.0 / B)) and (case.p0 > 0).all()
        assert (~case.active).any() and case.active.any()
        seen.add((B, L, case.N, case.alpha, case.p_floor > 0))
        p, cdf, lr, touched = E.refit_expected(R, case)
        s_cdf, s_lr = E.sentinel_tables(cdf.shape, lr.shape)
        c0, l0 = R.search_tables(case.p0)
        assert not (s_cdf == c0).any() and not (s_lr == l0).any()                   # the sentinel is no table of p0
        for k, kind in enumerate(case.kinds):
            elite = case.w[k] != 0
            assert (case.bins[k][:, ~elite] == 255).all() or kind == "none"
            assert (case.bins[k][:, elite] < B).all()
            if kind == "one_bin":
                assert elite.all() and all(len(np.unique(row)) == 1 for row in case.bins[k])
            elif kind == "every_bin":
                assert elite.all()
                if L >= 2 * B:
                    assert all(len(np.unique(row)) == B for row in case.bins[k])
                if L >= 128:                                     # every refit thread and both waves carry mass
                    assert set(np.nonzero(elite)[0] % 128) == set(range(128))
                if L > 128:                                      # ... and a thread's second candidate falls into another bin
                    assert (case.bins[k][:, 0] != case.bins[k][:, 128]).all()
            elif kind == "last_only":
                assert np.nonzero(elite)[0].tolist() == [L - 1]
            elif kind == "sparse":
                assert elite[L - 1] and (L < 3 or not elite.all())
            elif kind == "none":
                assert not elite.any() and (case.bins[k] < B).all() and not touched[k].any()
                assert E.bits_equal(p[k], case.p0[k]) and E.bits_equal(cdf[k], s_cdf[k]) and E.bits_equal(lr[k], s_lr[k])
            if kind != "none":
                assert touched[k].tolist() == case.active.tolist()
                if case.alpha == 0.0:                            # the row is still divided by its rounded sum
                    rounded += int(case.p_floor == 0.0 and not E.bits_equal(p[k][case.active], case.p0[k][case.active]))
                if case.alpha == 1.0 and case.p_floor == 0.0 and kind in ("one_bin", "last_only"):
                    rows = p[k][case.active]
                    assert ((rows == 0).sum(1) == B - 1).all() and ((rows == 1).sum(1) == 1).all()
                    zeros += 1
                    flat_steps += int((np.diff(cdf[k][case.active]) == 0).sum())
                    infs += int(np.isposinf(lr[k][case.active]).sum())
        assert E.bits_equal(p[:, ~case.active], case.p0[:, ~case.active])
    assert zeros > 0 and flat_steps > 0 and infs > 0 and rounded > 0
    for B in (2, 8, 64):
        for L in E.LS:
            for alpha in (0.0, 0.7, 1.0):
                for floor in (False, True):
                    assert (B, L, 1, alpha, floor) in seen
    assert {n for _, _, n, _, _ in seen} == {1, 8, 64}
    kinds = {(k, kind) for case in cases for k, kind in enumerate(case.kinds)}
    assert kinds == {(k, kind) for k in range(E.K) for kind in E.ELITE_KINDS}


# ---- sampler ----------------------------------------------------------------------------------------------------------------
def test_lane_words_carry_into_the_high_word():
    L, off = 65, 2 ** 32 - 3
    words = [E.counter_words(off, i) for i in range(L)]
    assert words[:4] == [(2 ** 32 - 3, 0), (2 ** 32 - 2, 0), (2 ** 32 - 1, 0), (0, 1)] and words[-1] == (61, 1)
    assert E.counter_words(2 ** 40, 5) == (5, 256) and E.counter_words(0, 7) == (7, 0)
    assert E.BIG_SEED >> 32 == 2 ** 31 and E.BIG_SEED & E.M32 == 5


def test_uniforms_are_the_oracles_reset_words(g, O):
    """uniforms() at a 64-bit offset and seed names the same episodes as the oracle's reset: the state map of its uniforms
    equals OracleEnvs.reset_philox() bit for bit on both sides of the carry."""
    N, lanes, off, seed, counter = 3, 6, 2 ** 32 - 3, E.BIG_SEED, 2 ** 32 - 1
    ref = O.OracleEnvs(lanes, N, seed=seed, env_offset=off)
    ref.episode[:] = counter
    ref.reset_philox()
    u = E.uniforms(O, N, counter, lanes, off, seed)
    own, trf, _ = g.records.encounter_from_uniforms(g.ACAS2DConfig(n_traffic=N), u)
    assert E.bits_equal(own[:, 2], np.asarray(ref.own_psi, np.float64))
    assert E.bits_equal(trf, np.stack([ref.trf_x, ref.trf_y, ref.trf_psi, ref.trf_v], axis=2).astype(np.float64))
    assert not np.array_equal(u, E.uniforms(O, N, counter, lanes, off, seed & E.M32))          # the seed's high word counts
    assert not np.array_equal(u[3], E.uniforms(O, N, counter, 1, 0, seed)[0])        # lane 2^32 is not lane 0


def test_sampler_cases_are_what_they_say(g, O):
    cases = E.sampler_cases()
    assert {(c.N, c.L) for c in cases} == set(E.SAMPLER_SIZES) and len({c.label for c in cases}) == len(cases)
    assert {(c.seed, c.generation, c.offset) for c in cases if (c.N, c.L) == E.FULL_CROSS} == set(E.SETTINGS)
    assert {c.seed for c in cases} == {13, 2 ** 63 + 5} and {c.generation for c in cases} == {0, 2 ** 32 - 1}
    assert {c.offset for c in cases} == {0, 2 ** 32 - 3, 2 ** 40}
    carried = [c for c in cases if c.offset == 2 ** 32 - 3 and c.L > 3]
    assert carried and all({E.counter_words(c.offset, i)[1] for i in range(c.L)} == {0, 1} for c in carried)
    kinds = set()
    in_tiny = inf_w = zero_p = 0
    for case in cases:
        ref = E.sampler_reference(g, O, case)
        (p, cdf, lr), u, B = ref["tables"], ref["u"], case.B
        assert p.shape == (E.K, 4 * (case.N + 1), B) and ref["bins"].max() < B
        assert not np.isnan(ref["log_w"]).any() and not np.isneginf(ref["log_w"]).any()
        for pl in ref["placed"]:
            kinds.add(pl.kind)
            row_p, row_c = p[pl.k, pl.c], cdf[pl.k, pl.c]
            if pl.kind == "empty_front":
                assert (row_p[:2] == 0).all() and (row_c[:3] == 0).all() and (row_p[2:] > 0).all()
            elif pl.kind == "empty_middle":
                h = B // 2
                assert (row_p[h - 1:h + 1] == 0).all() and row_c[h - 1] == row_c[h] == row_c[h + 1] and np.isposinf(lr[pl.k, pl.c, h])
                assert not (ref["bins"][pl.k][:, pl.c] == h).any() and not (ref["bins"][pl.k][:, pl.c] == h - 1).any()
            elif pl.kind == "empty_end":
                assert row_p[B - 1] == 0 and row_c[B - 1] == row_c[B] and not (ref["bins"][pl.k][:, pl.c] == B - 1).any()
            elif pl.kind == "floored":
                assert (row_p > 0).all() and len(np.unique(row_p)) >= 3
            elif pl.kind == "tie":                               # the placed edge equals the uniform bitwise: bin j at t = 0
                assert E.bits_equal(row_c[pl.bin], u[pl.cand, pl.c]) and pl.bin >= 1
                assert ref["bins"][pl.k][pl.cand, pl.c] == pl.bin and ref["c"][pl.k][pl.cand, pl.c] == pl.bin / B
            elif pl.kind == "mass_2^-40":
                assert row_p[pl.bin] == 2.0 ** -40 and ref["bins"][pl.k][pl.cand, pl.c] == pl.bin
                assert ref["c"][pl.k][pl.cand, pl.c] == (pl.bin + 0.5) / B
                in_tiny += 1
            elif pl.kind == "tie_last_empty":
                assert pl.bin == B - 1 and E.bits_equal(row_c[B - 1], u[pl.cand, pl.c]) and row_p[B - 1] == 0
                assert ref["bins"][pl.k][pl.cand, pl.c] == B - 1 and ref["c"][pl.k][pl.cand, pl.c] == (B - 1) / B      # 0 / 0, then t = 0
                assert np.isposinf(ref["log_w"][pl.k][pl.cand])
                inf_w += 1
                zero_p += int(row_p[B - 1] == 0)
        flat = np.full(B, 1.0 / B)
        for k in range(E.K):                                     # different per policy; inactive rows are flat
            assert all(E.bits_equal(p[k, c], flat) for c in np.nonzero(~ref["active"])[0])
            assert not all(E.bits_equal(t[k], t[(k + 1) % E.K]) for t in (p, cdf, lr))
    assert kinds == set(E.TABLE_KINDS) - {"flat"} and in_tiny > 0 and inf_w > 0 and zero_p > 0


# ---- archive ----------------------------------------------------------------------------------------------------------------
def test_archive_steps_are_what_they_say(g):
    cases = E.archive_cases()
    assert {c.N for c in cases} == {1, 8, 64} and {c.offset for c in cases} == {0, 2 ** 40} and any(c.nonflat for c in cases)
    for case in cases:
        steps, (first, again, closer) = E.archive_steps(case)
        assert [s.replaces for s in steps] == [False, True, False, True, False]
        assert not steps[0].outcome.any() and not steps[4].outcome.any() and steps[-1].generation < 2 ** 32
        best = [np.inf] * E.K
        for st in steps:
            for k in range(E.K):
                row = g.records.search_select(st.sep[k], st.outcome[k], np.zeros(case.L), 1, 0.0, False)["row"]
                assert (row[10] < best[k]) == st.replaces, (case.label, st.name)
                best[k] = min(best[k], row[10])
        for k in range(E.K):
            mins = [int(np.argmin(E.effective(steps[i].sep[k], steps[i].outcome[k]))) for i in (1, 2, 3)]
            assert mins == [first[k], again[k], closer[k]]
            assert steps[1].sep[k].min() == steps[2].sep[k].min() > steps[3].sep[k].min()
        assert len({c % 256 for c in first + again + closer}) == 9 and max(first) >= 256
