"""Shared by tests/test_encounter_search.py: the search's shapes, the uniforms of the oracle's Philox, the device's
generations read back one by one, and the reference -- the host loop of the NumPy specification (records.search_*) around
the EXISTING evaluate_policies_fused(safety=True).  One trace and one reference per (shape, settings), computed once and left
unchanged."""
from collections import namedtuple

import numpy as np

from eval_stats_support import DEV, bits_equal                     # noqa: F401  (bits_equal: for the tests)
from monte_carlo_support import F32, F64, policies as _policies, zero_policy  # noqa: F401

CANDIDATES = 70              # one full wave and a partial one
N_BINS = 8
N_QUANTILE = 7
GENERATIONS = 3
SEED = 13
ALPHA = 0.7
P_FLOOR = 1.0 / (16 * N_BINS)

Shape = namedtuple("Shape", "dtype fast N group max_steps")
SHAPES = [Shape(F32, True, 1, False, 1000), Shape(F32, True, 3, False, 1000), Shape(F64, False, 1, False, 1000),
          Shape(F64, True, 1, False, 1000), Shape(F32, True, 8, True, 1000), Shape(F32, True, 1, False, 150)]


def shape_id(s):
    return "%s%s-N%d%s%s" % ("f32" if s.dtype == F32 else "f64", "" if s.dtype == F32 else ("-fast" if s.fast else "-exact"), s.N,
                             "-group" if s.group else "", "" if s.max_steps == 1000 else "-T%d" % s.max_steps)


def config(g, s):
    return g.ACAS2DConfig(n_traffic=s.N, max_steps=s.max_steps, fast_math=s.fast)


def npdt(s):
    return np.float32 if s.dtype == F32 else np.float64


def level(g, s):
    return float(2 * config(g, s).collision_radius)


def policies(g, s):
    """[a, b, zero] of tests/monte_carlo_support.py."""
    return _policies(g, s)


def search(g, s, pols=None, **kw):
    kw.setdefault("alpha", ALPHA)
    return g.EncounterSearch(policies(g, s) if pols is None else pols, CANDIDATES, seed=SEED, dtype=s.dtype, group=s.group,
                             config=config(g, s), n_bins=N_BINS, n_quantile=N_QUANTILE, device=DEV, **kw)


_UNIFORMS = {}


def uniforms(O, N, generation, lanes=CANDIDATES, offset=0):
    """u [lanes, 4 (N + 1)] of the oracle's Philox: counter (lane, 0, generation, entity), key (SEED, 0), u = (w + 0.5) 2^-32."""
    key = (N, generation, lanes, offset)
    if key not in _UNIFORMS:
        u = np.zeros((lanes, 4 * (N + 1)), np.float64)
        for i in range(lanes):
            for e in range(N + 1):
                w = O.philox4x32([offset + i, 0, generation, e], [SEED, 0])
                u[i, 4 * e:4 * e + 4] = (w.astype(np.float64) + 0.5) / 4294967296.0
        u.setflags(write=False)
        _UNIFORMS[key] = u
    return _UNIFORMS[key]


def _freeze(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


_TRACES = {}


def trace(g, s, **kw):
    """The device's generations one by one: GENERATIONS x run(1), after each the buffers(), the candidates() and best().
    A list of {"buf", "cand", "best"}; trace[-1]["buf"] holds the buffers of the finished search."""
    key = (s, tuple(sorted(kw.items())))
    if key not in _TRACES:
        es = search(g, s, **kw)
        out = []
        for _ in range(GENERATIONS):
            es.run(1)
            buf = _freeze(es.buffers())                  # before candidates(): it draws the generation again
            out.append({"buf": buf, "cand": _freeze(es.candidates()), "best": es.best()})
        _TRACES[key] = out
    return _TRACES[key]


_CHAINS = {}


def host_chain(g, O, s, weighted, alpha=ALPHA):
    """The parent's only way to the same result: per generation and policy the NumPy sampler on the oracle's uniforms, the
    state map, evaluate_policies_fused(safety=True), the NumPy select and refit.  A list per generation of dicts of [K, ...]
    arrays: the tables drawn from (p, cdf, log_ratio), bins, log_w, own, traffic, goal, score, outcome, elite_w, row, p_next."""
    key = (s, weighted, alpha)
    if key not in _CHAINS:
        R, cfg, pols = g.records, config(g, s), policies(g, s)
        active = R.search_active_coordinates(cfg)
        K, NC = len(pols), 4 * (s.N + 1)
        p = np.full((K, NC, N_BINS), 1.0 / N_BINS)
        out = []
        for gen in range(GENERATIONS):
            u = uniforms(O, s.N, gen)
            cdf, lr = R.search_tables(p)
            rec = {"p": p.copy(), "cdf": cdf, "log_ratio": lr}
            per = {k: [] for k in ("bins", "log_w", "own", "traffic", "goal", "score", "outcome", "elite_w", "row", "p_next")}
            for k in range(K):
                c, bins, log_w = R.search_sample((p[k], cdf[k], lr[k]), active, u)
                own, trf, goal = R.encounter_from_uniforms(cfg, c, npdt(s))
                res = g.evaluate_policies_fused([pols[k]], own, trf, goal, dtype=s.dtype, device=DEV, config=cfg, group=s.group,
                                                safety=True)
                sel = R.search_select(res["min_separation"][0], res["outcome"][0], log_w, N_QUANTILE, level(g, s), weighted)
                nxt = R.search_refit(p[k], active, bins, sel["elite_w"], alpha, P_FLOOR)
                for name, val in zip(per, (bins, log_w, own, trf, goal, res["min_separation"][0], res["outcome"][0],
                                           sel["elite_w"], sel["row"], nxt)):
                    per[name].append(val)
            rec.update({k: np.stack(v) for k, v in per.items()})
            p = rec["p_next"].copy()
            out.append(_freeze(rec))
        _CHAINS[key] = out
    return _CHAINS[key]


# the policy axis of every buffer of EncounterSearch.buffers() (None: the buffer has none)
POLICY_AXIS = {"p": 0, "cdf": 0, "log_ratio": 0, "active": None, "bins": 0, "log_w": 0, "elite_w": 0, "outcome": 0, "steps": 0,
               "total_reward": 0, "stats_f": 1, "stats_i": 1, "best_score": 0, "best_generation": 0, "best_candidate": 0,
               "best_own_psi": 0, "best_traffic": 0, "history": 1}


def rows(buf, idx):
    """The buffers with their policy axis indexed by the list idx."""
    return {k: (v if POLICY_AXIS[k] is None else np.take(v, idx, axis=POLICY_AXIS[k])) for k, v in buf.items()}


def mismatches(got, want):
    assert set(got) == set(want) == set(POLICY_AXIS)
    return [k for k in want if not bits_equal(got[k], want[k])]


def ulps(a, b):
    """The distance of two float64 arrays in units of the last place of b (inf where one is not finite and they differ)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b) / np.spacing(np.abs(b))
    return np.where(a == b, 0.0, np.where(np.isfinite(a) & np.isfinite(b), d, np.inf))
