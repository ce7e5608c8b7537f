"""Hand-placed inputs for the three kernels of csrc/acas2d_search.hip, and a thin harness that calls their entries one at a
time on caller-owned buffers (acas2d_encounter_sample_f32/_f64, acas2d_encounter_select_f32/_f64, acas2d_encounter_refit),
exactly as policy.EncounterSearch._struct / _sample / _generation do.  Shared by tests/test_encounter_search_edges_host.py
(every case is what its label says; no GPU) and tests/test_encounter_search_edges.py (the kernels against records.search_*).

Why: tests/test_encounter_search.py meets 70 candidates only, so no thread of select (256) or refit (128) takes a second
candidate, waves hold no candidate, the scores are distinct finite floats and every table comes out of a floored refit.
The counts here sit on the edges of the 64-lane wave, the 128- and 256-thread blocks and the sampler's 64-env padding:
L in {1, 63, 65, 129, 257, 1025} (at 1 025 a select thread takes five candidates, a refit thread nine), always K = 3 with a
different pattern per policy row, so a row stride taken from the wrong size shows.

Scores.  -0.0 is left out on purpose: min_separation is a norm, and NumPy's sort does not order -0.0 before +0.0 while the
kernel's integer key does, so the specification is silent there.  -inf is left out likewise (a norm is never -inf).  Every
other class of float is placed: distinct, all equal, a run of equal values across the quantile's rank, values that differ
in the lowest or only in the top byte of the key, float64 values that agree in their high word, zeros and denormals, +inf
and NaN on finished episodes, unfinished episodes, negative values.

Refit weights are dyadic (m 2^-10, m < 2^20, or 1.0), so every partial sum is exact in any order and the new tables are
compared bit for bit: a wrong stride, column or cross-wave combine changes a sum.

Uniforms come from the oracle's Philox with the lane id split into counter words 0 and 1 (uniforms() below), cached per
(N, generation, lanes, offset, seed)."""
import ctypes as C
from collections import namedtuple

import numpy as np

from eval_stats_support import DEV, bits_equal                     # noqa: F401  (for the tests)

K = 3
LS = (1, 63, 65, 129, 257, 1025)
DTYPES = {"f32": np.float32, "f64": np.float64}
SEED = 13
BIG_SEED = 2 ** 63 + 5
M32 = 0xFFFFFFFF
EPS = 2.0 ** -53


def case_rng(*words):
    return np.random.default_rng([int(w) for w in words])


def middle(L):
    return max(1, (L + 1) // 3)


# ---- uniforms ---------------------------------------------------------------------------------------------------------------
_UNIFORMS = {}


def counter_words(offset, i):
    """(lane lo, lane hi) of lane offset + i: Philox counter words 0 and 1."""
    gid = int(offset) + int(i)
    return gid & M32, gid >> 32


def uniforms(O, N, generation, lanes, offset=0, seed=SEED):
    """u [lanes, 4 (N + 1)] of the oracle's Philox: counter (lane lo, lane hi, generation, entity), key (seed lo, seed hi),
    u = (w + 0.5) 2^-32."""
    key = (N, generation, lanes, offset, seed)
    if key not in _UNIFORMS:
        u = np.zeros((lanes, 4 * (N + 1)), np.float64)
        k = [seed & M32, seed >> 32]
        for i in range(lanes):
            lo, hi = counter_words(offset, i)
            for e in range(N + 1):
                w = O.philox4x32([lo, hi, generation, e], k)
                u[i, 4 * e:4 * e + 4] = (w.astype(np.float64) + 0.5) / 4294967296.0
        u.setflags(write=False)
        _UNIFORMS[key] = u
    return _UNIFORMS[key]


# ---- select: placed scores --------------------------------------------------------------------------------------------------
SELECT_KINDS = {"f32": ("distinct", "all_equal", "tie", "low_byte", "top_byte", "zeros_denormals", "inf_finished", "nan",
                        "some_unfinished", "all_unfinished", "negative", "min_tie"),
                "f64": ("distinct", "all_equal", "tie", "low_byte", "top_byte", "high_word_equal", "zeros_denormals", "inf_finished",
                        "nan", "some_unfinished", "all_unfinished", "negative", "min_tie")}
NQ_KINDS = ("one", "middle", "all")
LEVEL_KINDS = ("below", "equal", "between", "above", "inf")
STEP = 0.375                                                     # dyadic: lo + STEP i is exact and distinct in float32


def spots(L):
    """Candidate indices in different threads (mod 256), lanes (mod 64) and waves, the last and the first among them; 6 and
    262 share a select thread, as 0 and 1 024 do."""
    out = []
    for i in (L - 1, 0, 75, 262, 6, 200, 150, L // 2, L // 3, 1):
        if 0 <= i < L and i not in out:
            out.append(i)
    return out


def _arrange(sorted_vals, ranks, idx, rng):
    """The values in shuffled order, with the value of rank ranks[j] at candidate idx[j]."""
    L = len(sorted_vals)
    perm = rng.permutation(L)                                    # perm[r]: the candidate that gets the value of rank r
    for r, i in zip(ranks, idx):
        j = int(np.nonzero(perm == i)[0][0])
        perm[j], perm[r] = perm[r], perm[j]
    out = np.empty(L, sorted_vals.dtype)
    out[perm] = sorted_vals
    return out


def _from_bits(bits, dt):
    return np.asarray(bits, {4: np.uint32, 8: np.uint64}[np.dtype(dt).itemsize]).view(dt)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def tie_ranks(L, nq):
    """The 0-based ranks of the run of equal values around rank nq - 1: two copies on each side where there is room."""
    return list(range(nq - 1 - min(2, nq - 1), nq + min(2, L - nq)))


def scores(kind, L, dt, nq, rng):
    """(min_sep [L] of dt, outcome [L] uint8) of one policy row."""
    dt = np.dtype(dt).type
    wide = np.dtype(dt).itemsize == 8
    oc = (np.arange(L) % 3 + 1).astype(np.uint8)
    line = (50.0 + STEP * np.arange(L)).astype(dt)
    distinct = line[rng.permutation(L)]
    if kind == "distinct":
        return distinct, oc
    if kind == "all_equal":
        return np.full(L, 123.4375, dt), oc
    if kind == "tie":
        ranks = tie_ranks(L, nq)
        v = line.copy()
        v[ranks] = v[nq - 1]
        return _arrange(v, ranks, spots(L)[:len(ranks)], rng), oc
    if kind == "min_tie":
        m = min(4, L)
        v = line.copy()
        v[:m] = v[0]
        idx = [i for i in (262, 6, 200, 75) if i < L]
        idx += [i for i in spots(L) if i not in idx]
        return _arrange(v, list(range(m)), idx[:m], rng), oc
    if kind == "low_byte":
        base = int(_bits(np.array([150.0], dt))[0]) & ~0xFF
        return _from_bits(base | rng.integers(0, 256, L), dt).copy(), oc
    if kind == "top_byte":
        t = rng.integers(0, 128, L)
        t[:2] = (0, 127)[:L]
        t = rng.permutation(t)
        low, shift = (0x23456789ABCDEF, 56) if wide else (0x123456, 24)
        return _from_bits((t.astype(np.uint64) << np.uint64(shift)) | np.uint64(low), dt).copy(), oc
    if kind == "high_word_equal":
        hi = int(_bits(np.array([150.0], dt))[0]) >> 32 << 32
        return _from_bits(np.uint64(hi) | rng.integers(0, 2 ** 32, L, dtype=np.uint64), dt).copy(), oc
    if kind == "zeros_denormals":
        f = np.finfo(dt)
        pool = np.array([0.0, f.smallest_subnormal, 2 * f.smallest_subnormal, 5 * f.smallest_subnormal,
                         1000 * f.smallest_subnormal, f.tiny, 2 * f.tiny], dt)
        return pool[rng.integers(0, len(pool), L)], oc
    if kind == "inf_finished":
        distinct[1::4] = np.inf
        if L > 2:
            distinct[0] = np.inf
        return distinct, oc
    if kind == "nan":
        distinct[2::5] = np.nan
        if L > 1:
            distinct[0] = np.nan
        return distinct, oc
    if kind == "some_unfinished":                                # the closest quarter never finished, nor did every seventh
        oc[distinct < line[L // 4]] = 0
        oc[3::7] = 0
        return distinct, oc
    if kind == "all_unfinished":
        return distinct, np.zeros(L, np.uint8)
    if kind == "negative":
        v = ((STEP * np.arange(L)) - (STEP * (L // 2))).astype(dt)[rng.permutation(L)]
        v[L // 5] = -1.0e30
        return v, oc
    raise KeyError(kind)


def effective(sep, oc):
    """score_of(): the separation where the episode finished and the value is a number, else +inf."""
    sep = np.asarray(sep)
    return np.where((np.asarray(oc) != 0) & ~np.isnan(sep), sep, sep.dtype.type(np.inf)).astype(sep.dtype)


def level_of(kind, sep, oc, nq):
    """A level of the requested kind for one row, in the row's dtype (returned as a Python float, exactly representable)."""
    dt = sep.dtype.type
    s = effective(sep, oc)
    fin = np.unique(s[np.isfinite(s)])
    if fin.size == 0:
        fin = np.array([100.0], dt)
    inf = dt(np.inf)
    if kind == "below":
        return float(np.nextafter(fin[0], -inf))
    if kind == "equal":
        return float(fin[fin.size // 2])
    if kind == "between":
        for a, b in zip(fin[:-1], fin[1:]):
            m = np.nextafter(a, inf)
            if m < b:
                return float(m)
        return float(np.nextafter(fin[-1], inf))
    if kind == "above":
        gq = np.sort(s)[nq - 1]
        above = fin[fin > gq]
        return float(above[min(1, above.size - 1)]) if above.size else float(np.nextafter(gq, inf))
    if kind == "inf":
        return float("inf")
    raise KeyError(kind)


SelectCase = namedtuple("SelectCase", "label L dtype kinds sep outcome n_quantile nq_kind level level_kind level_row")


def nq_values(L):
    out = []
    for kind, v in zip(NQ_KINDS, (1, middle(L), L)):
        if v not in [x for _, x in out]:
            out.append((kind, v))
    return out


def select_rows(kinds, L, dtype, nq):
    dt = DTYPES[dtype]
    rows = [scores(kind, L, dt, nq, case_rng(L, np.dtype(dt).itemsize, SELECT_KINDS[dtype].index(kind), r, nq))
            for r, kind in enumerate(kinds)]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


def select_cases(L, dtype):
    """Every score pattern of the dtype in a row of some launch (three per launch, rotated with L), crossed with n_quantile
    in {1, a middle value, L} and the five levels; the level is placed against the scores of row level_row."""
    kinds = SELECT_KINDS[dtype]
    n, rot = len(kinds), LS.index(L)
    out = []
    for t in range(0, n, 3):
        triple = tuple(kinds[(t + r + rot) % n] for r in range(K))
        for nq_kind, nq in nq_values(L):
            sep, oc = select_rows(triple, L, dtype, nq)
            for level_kind in LEVEL_KINDS:
                row = len(out) % K
                level = level_of(level_kind, sep[row], oc[row], nq)
                out.append(SelectCase("%s-L%d-%s-nq_%s-level_%s" % (dtype, L, "+".join(triple), nq_kind, level_kind), L, dtype,
                                      triple, sep, oc, nq, nq_kind, level, level_kind, row))
    return out


WeightedCase = namedtuple("WeightedCase", "label L dtype kinds sep outcome log_w n_quantile level exact")


def weighted_log_w(L):
    """log_w [K, L] in [-30, 30], both ends and 0 placed."""
    lw = case_rng(L, 30).uniform(-30.0, 30.0, (K, L))
    lw[:, L // 2] = 0.0
    lw[:, -1] = 30.0
    lw[:, 0] = -30.0 if L > 1 else 30.0
    return lw


def weighted_cases(L, dtype):
    """The weighted path.  The first case has every candidate finished, finite and elite (n_quantile = L): its elite_w are
    the device's weights of all candidates, which the others' sums are held to.  The last has log_w = 0: its sums are exact."""
    lw, mid = weighted_log_w(L), middle(L)
    out = []
    for name, kinds, nq, level_kind, exact in (("all_elite", ("distinct", "low_byte", "negative"), L, "below", False),
                                               ("mixed", ("some_unfinished", "tie", "nan"), mid, "above", False),
                                               ("level_inf", ("distinct", "inf_finished", "all_unfinished"), 1, "inf", False),
                                               ("log_w_zero", ("tie", "some_unfinished", "distinct"), mid, "equal", True)):
        sep, oc = select_rows(kinds, L, dtype, nq)
        level = level_of(level_kind, sep[1], oc[1], nq)
        out.append(WeightedCase("%s-L%d-%s" % (dtype, L, name), L, dtype, kinds, sep, oc, np.zeros_like(lw) if exact else lw, nq,
                                level, exact))
    return out


# ---- tables -----------------------------------------------------------------------------------------------------------------
def search_config(g, N):
    """The config of the sampler and archive cases: the airspeed factor varies, so every aircraft's word w is active too."""
    return g.ACAS2DConfig(n_traffic=N, airspeed_factor_min=0.8, airspeed_factor_max=1.2)


def refit_row(R, B, masses, alpha=1.0, p_floor=0.0):
    """The row records.search_refit() makes of a flat row and `masses[b]` elite candidates of weight 1 in bin b."""
    masses = np.asarray(masses, np.int64)
    bins = np.repeat(np.arange(B, dtype=np.uint8), masses)[:, None]
    return R.search_refit(np.full((1, B), 1.0 / B), [True], bins, np.ones(bins.shape[0]), alpha, p_floor)[0]


def random_tables(R, NC, B, rng):
    """Non-flat proposals [K, NC, B] with their tables: floored refits of random counts."""
    p = np.stack([np.stack([refit_row(R, B, rng.integers(0, 9, B) + (np.arange(B) == c % B), 0.7, 1.0 / (16 * B))
                            for c in range(NC)]) for _ in range(K)])
    return (p,) + R.search_tables(p)


TABLE_KINDS = ("flat", "empty_front", "empty_middle", "empty_end", "floored", "mass_2^-40", "tie", "tie_last_empty")
Placed = namedtuple("Placed", "kind k c cand bin")               # a table row placed against u[cand, c]


def sampler_tables(R, active, u, B, salt=0):
    """Tables [K, NC, B] / [K, NC, B + 1] / [K, NC, B], a different kind per policy and active coordinate, and the list of
    rows placed against a candidate's uniform.  The tables need not be consistent: the specification and the kernel read the
    same three arrays."""
    L, NC = u.shape
    p = np.full((K, NC, B), 1.0 / B)
    cdf, lr = R.search_tables(p)
    placed = []
    h = B // 2
    rows = {"empty_front": refit_row(R, B, [0, 0] + [3] * (B - 2)),
            "empty_middle": refit_row(R, B, [5] * (h - 1) + [0, 0] + [2] * (B - h - 1)),
            "empty_end": refit_row(R, B, [1] * (B - 1) + [0]),
            "floored": refit_row(R, B, [7, 1] + [0] * (B - 2), 0.7, 1.0 / (16 * B))}
    for k in range(K):
        for n, c in enumerate(np.nonzero(active)[0]):
            kind = TABLE_KINDS[(salt + n + 3 * k) % len(TABLE_KINDS)]
            if kind in rows:
                p[k, c] = rows[kind]
                cdf[k, c], lr[k, c] = R.search_tables(rows[kind])
                placed.append(Placed(kind, k, int(c), -1, -1))
            if kind not in ("mass_2^-40", "tie", "tie_last_empty"):
                continue
            order = (np.arange(L) + (37 * k + 11 * c)) % L       # the first candidate from a row-dependent start whose bin is not 0
            ok = [int(i) for i in order if int(u[i, c] * B) >= 1]
            if not ok:
                continue                                         # (a single candidate in bin 0: the row stays flat)
            i = ok[0]
            ui, j = float(u[i, c]), int(u[i, c] * B)
            if kind == "tie":                                    # cdf[j] == u: bin j at t = 0, not bin j - 1
                cdf[k, c, j] = ui
            elif kind == "mass_2^-40":                           # the candidate sits in the middle of a bin of mass 2^-40
                cdf[k, c, j] = ui - 2.0 ** -41
                cdf[k, c, j + 1] = cdf[k, c, j] + 2.0 ** -40
                p[k, c, j] = 2.0 ** -40
                p[k, c, j - 1] = cdf[k, c, j] - cdf[k, c, j - 1]
                if j + 1 < B:
                    p[k, c, j + 1] = cdf[k, c, j + 2] - cdf[k, c, j + 1]
                with np.errstate(divide="ignore"):
                    lr[k, c] = -np.log(B * p[k, c])
            else:                                                # the tie on the last edge, and the last bin is empty: 0 / 0
                j = B - 1
                cdf[k, c, :B] = ui * (np.arange(B) / float(B - 1))
                cdf[k, c, B] = ui
                p[k, c, :B - 1] = np.diff(cdf[k, c, :B])
                p[k, c, j] = 0.0
                with np.errstate(divide="ignore"):
                    lr[k, c] = -np.log(B * p[k, c])
            placed.append(Placed(kind, k, int(c), i, j))
    return (p, cdf, lr), placed


SamplerCase = namedtuple("SamplerCase", "label N L B seed generation offset")
SETTINGS = [(s, gen, off) for s in (SEED, BIG_SEED) for gen in (0, 2 ** 32 - 1) for off in (0, 2 ** 32 - 3, 2 ** 40)]
SAMPLER_SIZES = [(N, L) for N in (1, 3, 8) for L in LS] + [(64, 65)]
FULL_CROSS = (3, 129)                                            # every setting at this size (64 bins); two per other size


def sampler_cases():
    out = []
    for n, (N, L) in enumerate(SAMPLER_SIZES):
        settings = SETTINGS if (N, L) == FULL_CROSS else [SETTINGS[(5 * n) % 12], SETTINGS[(5 * n + 7) % 12]]
        B = 64 if (N, L) == FULL_CROSS else 8
        for seed, gen, off in settings:
            out.append(SamplerCase("N%d-L%d-B%d-seed%s-gen%s-off%s" % (N, L, B, "13" if seed == SEED else "2^63+5", "0" if gen == 0 else "2^32-1",
                                                                      {0: "0", 2 ** 32 - 3: "2^32-3", 2 ** 40: "2^40"}[off]),
                                   N, L, B, seed, gen, off))
    return out


_SAMPLES = {}


def sampler_reference(g, O, case):
    """{"tables", "placed", "u", "bins" [K, L, NC], "log_w" [K, L], "c" [K, L, NC]} of the specification, computed once."""
    if case not in _SAMPLES:
        R, cfg = g.records, search_config(g, case.N)
        active = R.search_active_coordinates(cfg)
        u = uniforms(O, case.N, case.generation, case.L, case.offset, case.seed)
        tables, placed = sampler_tables(R, active, u, case.B, salt=SAMPLER_SIZES.index((case.N, case.L)))
        per = [R.search_sample(tuple(t[k] for t in tables), active, u) for k in range(K)]
        ref = {"tables": tables, "placed": placed, "u": u, "active": active, "c": np.stack([x[0] for x in per]),
               "bins": np.stack([x[1] for x in per]), "log_w": np.stack([x[2] for x in per])}
        for a in ref.values():
            for t in (a if isinstance(a, tuple) else (a,)):
                if isinstance(t, np.ndarray):
                    t.setflags(write=False)
        _SAMPLES[case] = ref
    return _SAMPLES[case]


# ---- refit: placed bins and weights -----------------------------------------------------------------------------------------
ELITE_KINDS = ("one_bin", "every_bin", "last_only", "sparse", "none")
RefitCase = namedtuple("RefitCase", "label B L N alpha p_floor kinds active p0 bins w")


def refit_active(g, N):
    return g.records.search_active_coordinates(g.ACAS2DConfig(n_traffic=N))


def elite_rows(kind, B, L, NC, rng, counted):
    """(bins [NC, L] uint8, elite_w [L]) of one policy row.  Non-elite candidates (weight 0) carry bin 255."""
    i, c = np.arange(L)[None, :], np.arange(NC)[:, None]
    w = np.ones(L) if counted else rng.integers(1, 2 ** 20, L).astype(np.float64) * 2.0 ** -10
    if kind == "one_bin":
        bins = np.broadcast_to((5 * c + 3) % B, (NC, L))
    elif kind == "every_bin":                                    # a thread's successive candidates fall into different bins
        bins = (i + i // 128 + c) % B
    elif kind == "last_only":
        bins = np.where(i == L - 1, (c + 1) % B, 255)
        w = np.where(np.arange(L) == L - 1, w, 0.0)
    elif kind == "sparse":
        elite = np.arange(L) % 3 == (L - 1) % 3
        bins = np.where(elite[None, :], rng.integers(0, B, (NC, L)), 255)
        w = np.where(elite, w, 0.0)
    elif kind == "none":
        bins = rng.integers(0, B, (NC, L))
        w = np.zeros(L)
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(bins, dtype=np.uint8), w


def start_proposal(B, NC, rng):
    """A non-flat p [K, NC, B] whose rows sum to 1 only within rounding, so alpha = 0 still changes its bits."""
    raw = rng.integers(1, 64, (K, NC, B)).astype(np.float64)
    return raw / raw.sum(-1, keepdims=True)


REFIT_SETTINGS = [(a, f) for a in (0.0, 0.7, 1.0) for f in (0, 1)]          # f: p_floor = 0 or 1 / (16 B)
REFIT_SIZES = [(B, L, 1) for B in (2, 8, 64) for L in LS] + [(B, L, 8) for B in (2, 8, 64) for L in (65, 1025)] + \
    [(8, 129, 64), (64, 257, 64)]


_REFIT_CASES = []


def refit_cases(g):
    """Every size of REFIT_SIZES with every (alpha, p_floor) (two of them at N = 64), three elite kinds per launch, rotated;
    counted and dyadic weights alternate.  Computed once."""
    out = _REFIT_CASES
    if out:
        return out
    for n, (B, L, N) in enumerate(REFIT_SIZES):
        active = refit_active(g, N)
        NC = active.size
        settings = REFIT_SETTINGS if N < 64 else [(0.7, 1), (1.0, 0)]
        for m, (alpha, f) in enumerate(settings):
            rng = case_rng(B, L, N, m)
            kinds = tuple(ELITE_KINDS[(n + m + r) % len(ELITE_KINDS)] for r in range(K))
            rows = [elite_rows(kind, B, L, NC, rng, counted=(n + m + r) % 2 == 0) for r, kind in enumerate(kinds)]
            p_floor = 1.0 / (16 * B) if f else 0.0
            out.append(RefitCase("B%d-L%d-N%d-alpha%g-floor%s-%s" % (B, L, N, alpha, "1/16B" if f else "0", "+".join(kinds)), B, L, N,
                                 alpha, p_floor, kinds, active, start_proposal(B, NC, rng), np.stack([r[0] for r in rows]),
                                 np.stack([r[1] for r in rows])))
    return out


def sentinel_tables(shape_cdf, shape_lr):
    """cdf and log_ratio that are no search_tables() of anything: what an untouched row must still hold."""
    cdf = -7.0 - 0.5 * np.arange(int(np.prod(shape_cdf)), dtype=np.float64).reshape(shape_cdf)
    lr = 1234.5 + np.arange(int(np.prod(shape_lr)), dtype=np.float64).reshape(shape_lr)
    return cdf, lr


def refit_expected(R, case):
    """(p, cdf, log_ratio, touched [K, NC]) of the specification from the sentinel tables: a row is touched iff its coordinate
    is active and its policy has elite weight."""
    cdf, lr = sentinel_tables((K, case.active.size, case.B + 1), (K, case.active.size, case.B))
    p = np.stack([R.search_refit(case.p0[k], case.active, case.bins[k].T, case.w[k], case.alpha, case.p_floor) for k in range(K)])
    touched = case.active[None, :] & (case.w.sum(1) > 0)[:, None]
    c2, l2 = R.search_tables(p)
    return p, np.where(touched[:, :, None], c2, cdf), np.where(touched[:, :, None], l2, lr), touched


# ---- archive ----------------------------------------------------------------------------------------------------------------
ArchiveCase = namedtuple("ArchiveCase", "label N L B dtype seed offset generation nonflat")
ARCHIVE_L, ARCHIVE_B = 257, 8
ARCHIVE_VARIANTS = (("flat", SEED, 0, 5, False), ("nonflat", BIG_SEED, 0, 2 ** 32 - 4, True), ("offset_2^40", SEED, 2 ** 40, 7, True))


def archive_cases():
    return [ArchiveCase("%s-N%d-%s" % (dtype, N, name), N, ARCHIVE_L, ARCHIVE_B, dtype, seed, off, gen, nonflat)
            for dtype in DTYPES for N in (1, 8, 64) for name, seed, off, gen, nonflat in ARCHIVE_VARIANTS]


ArchiveStep = namedtuple("ArchiveStep", "name sep outcome generation second_tables replaces")


def archive_steps(case):
    """Five select calls on the same buffers: nothing finished (the archive stays empty); a first minimum; a generation later
    the same minimum at other candidates (the first is kept); a strictly smaller one, drawn from other tables (it replaces);
    nothing finished again (untouched).  Row k's minima sit at different candidates, beyond a thread's first one too."""
    dt, L = DTYPES[case.dtype], case.L
    oc = (np.arange(L) % 3 + 1).astype(np.uint8)
    first, again, closer = (200, 6, 256), (3, 199, 70), (64, 255, 130)
    steps = []

    def batch(salt, spot, value):
        sep = np.stack([(50.0 + STEP * case_rng(case.N, salt, k).permutation(L)).astype(dt) for k in range(K)])
        for k in range(K):
            sep[k, spot[k]] = value
        return sep

    g0 = case.generation
    steps.append(ArchiveStep("nothing finished", batch(0, first, 1.0), np.zeros((K, L), np.uint8), g0, False, False))
    steps.append(ArchiveStep("first minimum", batch(1, first, 40.5), np.tile(oc, (K, 1)), g0 + 1, False, True))
    steps.append(ArchiveStep("equal minimum", batch(2, again, 40.5), np.tile(oc, (K, 1)), g0 + 2, False, False))
    steps.append(ArchiveStep("smaller minimum", batch(3, closer, 40.25), np.tile(oc, (K, 1)), g0 + 3, True, True))
    steps.append(ArchiveStep("nothing finished again", batch(4, again, 1.0), np.zeros((K, L), np.uint8), g0 + 3, False, False))
    return steps, (first, again, closer)


# ---- the direct-call harness (GPU) ------------------------------------------------------------------------------------------
GUARD = 256                                                      # sentinel elements kept behind bins and log_w


class Direct:
    """The fifteen buffers of an Acas2dEncounterSearch as torch tensors, and the three entries called on them one at a time.
    put() / get() move numpy arrays; best_generation reads back as uint32."""

    def __init__(self, g, n_candidates, n_traffic, n_bins, dtype, config=None):
        import torch
        self.g, self.torch, self.native = g, torch, g.native
        self.L, self.N, self.B, self.dtype = int(n_candidates), int(n_traffic), int(n_bins), dtype
        self.tdtype = torch.float32 if DTYPES[dtype] == np.float32 else torch.float64
        self.config = config if config is not None else g.ACAS2DConfig(n_traffic=n_traffic)
        self.ccfg = self.config.to_c()
        self.NC = NC = 4 * (self.N + 1)
        L, B, N, T = self.L, self.B, self.N, self.tdtype
        z = lambda *shape, dt=torch.float64: torch.zeros(*shape, dtype=dt, device=DEV)  # noqa: E731
        flat = np.full((K, NC, B), 1.0 / B)
        self.t = {"p": z(K, NC, B), "cdf": z(K, NC, B + 1), "log_ratio": z(K, NC, B), "active": z(NC, dt=torch.uint8),
                  "bins": z(K * NC * L + GUARD, dt=torch.uint8), "log_w": z(K * L + GUARD), "elite_w": z(K, L),
                  "outcome": z(K, L, dt=torch.uint8), "min_sep": z(K, L, dt=T), "history": z(K, g.native.SEARCH_HISTORY_WIDTH),
                  "best_score": torch.full((K,), float("inf"), dtype=T, device=DEV), "best_generation": z(K, dt=torch.int32),
                  "best_candidate": torch.full((K,), -1, dtype=torch.int32, device=DEV), "best_own_psi": z(K, dt=T),
                  "best_traffic": z(K, N, 4, dt=T)}
        self.put(p=flat, active=g.records.search_active_coordinates(self.config).astype(np.uint8))
        self.put(**dict(zip(("cdf", "log_ratio"), g.records.search_tables(flat))))
        self._env = None

    def put(self, **arrays):
        for name, a in arrays.items():
            t = self.t[name]
            a = np.array(a, order="C")                           # (a writable copy: the cases' arrays are read-only)
            src = self.torch.as_tensor(a.view(np.int32) if a.dtype == np.uint32 else a)
            assert src.dtype == t.dtype, (name, src.dtype, t.dtype)
            if name in ("bins", "log_w"):                        # (their guard tail is left alone)
                t[:src.numel()].copy_(src.reshape(-1))
            else:
                assert tuple(src.shape) == tuple(t.shape), (name, src.shape, t.shape)
                t.copy_(src)
        return self

    def tables(self, tables):
        return self.put(p=tables[0], cdf=tables[1], log_ratio=tables[2])

    def fill(self, name, value):
        self.t[name].fill_(value)
        return self

    def get(self, *names):
        out = []
        for name in names:
            a = self.t[name].cpu().numpy()
            if name == "bins":
                a = a[:K * self.NC * self.L].reshape(K, self.NC, self.L)
            elif name == "log_w":
                a = a[:K * self.L].reshape(K, self.L)
            elif name == "best_generation":
                a = a.view(np.uint32)
            out.append(a)
        return out[0] if len(out) == 1 else out

    def guard(self, name):
        return self.t[name][-GUARD:].cpu().numpy()

    def struct(self, generation=0, n_quantile=1, weighted=0, alpha=0.7, p_floor=0.0, level=0.0):
        t = self.t
        return self.native.CEncounterSearch(
            *[t[n].data_ptr() for n in ("p", "cdf", "log_ratio", "active", "bins", "log_w", "elite_w", "outcome", "min_sep", "history",
                                        "best_score", "best_generation", "best_candidate", "best_own_psi", "best_traffic")],
            self.B, self.NC, int(n_quantile), int(weighted), float(alpha), float(p_floor), float(level), int(generation))

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.torch.device(DEV)).cuda_stream)

    def _entry(self, stem):
        return getattr(self.native.lib(), "acas2d_encounter_%s_%s" % (stem, self.dtype))

    def select(self, n_quantile, level, weighted, generation=0, seed=SEED, env_offset=0):
        cs = self.struct(generation, n_quantile, weighted, level=level)
        with self.torch.cuda.device(DEV):
            self.native.check(self._entry("select")(C.byref(self.ccfg), K, self.L, seed, env_offset, self.N, C.byref(cs), self._stream()))
        return self

    def refit(self, alpha, p_floor):
        cs = self.struct(alpha=alpha, p_floor=p_floor)
        with self.torch.cuda.device(DEV):
            self.native.check(self.native.lib().acas2d_encounter_refit(C.byref(cs), K, self.L, self._stream()))
        return self

    def env(self):
        if self._env is None:
            self.EP = self.g.policy.PolicyBlocks.block_envs(self.L)
            self._env = self.g.ACAS2DVecEnv(K * self.EP, self.N, device=DEV, dtype=self.tdtype, config=self.config,
                                            keep_terminal_obs=False, double_buffer=False)
        return self._env

    STATE = ("own_x", "own_y", "own_psi", "own_v", "goal_x", "goal_y", "trf_x", "trf_y", "trf_psi", "trf_v")

    def sample(self, generation, seed=SEED, env_offset=0):
        """One sampler launch into a state whose arrays hold a sentinel.  Returns own [K, EP, 4], traffic [K, EP, N, 4],
        goal [K, EP, 2], steps [K, EP] and total_reward [K, EP] of all envs, the padding included."""
        v = self.env()
        for name in self.STATE + ("total_reward",):
            getattr(v, name).fill_(-777.0)
        v.steps.fill_(7)
        cs = self.struct(generation)
        with self.torch.cuda.device(DEV):
            self.native.check(self._entry("sample")(C.byref(v._ccfg), C.byref(v._cstate), v.num_envs, K, self.L, seed, env_offset,
                                                    self.N, C.byref(cs), self._stream()))
        f = lambda t: t.detach().cpu().numpy()  # noqa: E731
        EP = self.EP
        own = np.stack([f(v.own_x), f(v.own_y), f(v.own_psi), f(v.own_v)], axis=1).reshape(K, EP, 4)
        trf = np.stack([f(v.trf_x), f(v.trf_y), f(v.trf_psi), f(v.trf_v)], axis=2).reshape(K, EP, self.N, 4)
        goal = np.stack([f(v.goal_x), f(v.goal_y)], axis=1).reshape(K, EP, 2)
        return own, trf, goal, f(v.steps).reshape(K, EP), f(v.total_reward).reshape(K, EP)
