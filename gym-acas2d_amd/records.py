"""Episode records in the reference's CSV layout.

`baseline_main.simulate()` (baseline_main.py:32-74) and `testing_main.simulate()`
(testing_main.py:62-138) roll TEST_EPISODES episodes on one env and dump a pandas DataFrame with
the columns  Episode, Outcome, Total Reward, Time Steps, Path, Traffic Paths  (the test script adds
per-step records that live only in the pygame-side game object).  This module produces the same
table from the single-env adapter, so the reference's notebooks keep working on engine output.
"""
import numpy as np

from .config import OUTCOME_NAMES

BASELINE_COLUMNS = ("Episode", "Outcome", "Total Reward", "Time Steps", "Path", "Traffic Paths")
# testing_main.py:114-138: the baseline columns, Path Length and the thirteen per-step record lists
TESTING_RECORDS = (("psi", "heading_record"), ("d_sep", "d_sep_record"), ("a_lat", "a_lat_record"),
                   ("d_goal", "d_goal_record"), ("delta_heading", "delta_h_goal_record"),
                   ("v_closing", "v_closing_record"), ("d_cpa", "d_cpa_record"), ("d_dev", "d_dev_record"),
                   ("r_d_goal", "step_reward_d_goal_record"), ("r_h_goal", "step_reward_h_goal_record"),
                   ("r_d_cpa", "step_reward_d_cpa_record"), ("r_d_dev", "step_reward_d_dev_record"),
                   ("r_step", "step_reward_record"))
TESTING_COLUMNS = ("Episode", "Outcome", "Total Reward", "Time Steps", "Path Length", "Path", "Traffic Paths") + \
    tuple(c for c, _ in TESTING_RECORDS)


def simulate(env, episodes=100, policy=None, max_steps=None, columns="baseline", initial_states=None):
    """baseline_main.simulate() / testing_main.simulate(): `episodes` x (reset; step until done or
    MAX_STEPS).  `policy(obs)` returns the action array (default: the constant action [0] of
    baseline_main.py:44; testing_main.py:74 passes `model.predict(obs, deterministic=True)[0]`).
    columns="baseline": baseline_main.py:67-74's table; "testing": testing_main.py:114-138's, with Path
    Length and the per-step records.  initial_states: optional list of (own, trf, goal) to replay instead of
    drawing episodes.  Returns a dict of columns (lists), ready for pandas.DataFrame(...)."""
    max_steps = max_steps or env.config.max_steps
    names = TESTING_COLUMNS if columns == "testing" else BASELINE_COLUMNS
    cols = {c: [] for c in names}
    for episode in range(1, episodes + 1):
        obs = env.reset() if initial_states is None else env.reset_to(*initial_states[episode - 1])
        env.game.episode = episode
        for _ in range(max_steps):
            action = np.array([0]) if policy is None else policy(obs)
            obs, _, done, _ = env.step(action)
            if done:
                break
        g = env.game
        cols["Episode"].append(episode)
        cols["Outcome"].append(OUTCOME_NAMES.get(g.outcome))
        cols["Total Reward"].append(g.total_reward)
        cols["Time Steps"].append(g.steps)
        cols["Path"].append(list(g.path))
        cols["Traffic Paths"].append([list(p) for p in g.traffic_paths])
        if columns == "testing":
            cols["Path Length"].append(g.d_path)
            for c, attr in TESTING_RECORDS:
                cols[c].append(list(getattr(g, attr)))
    return cols


def to_csv(cols, path):
    """DataFrame.to_csv(path, index=False) as the reference writes it (baseline_main.py:67-74,
    testing_main.py:114-138)."""
    import pandas as pd
    names = TESTING_COLUMNS if "Path Length" in cols else BASELINE_COLUMNS
    pd.DataFrame({c: cols[c] for c in names}).to_csv(path, index=False)


# ---- per-episode safety statistics (acas2d_evaluate_policies_stats_*, policy.evaluate_policies_fused(safety=True)) -------
SAFETY_KEYS = ("min_separation", "min_separation_step", "los_steps", "max_abs_a_lat", "max_abs_deviation",
               "mean_abs_deviation")


def episode_safety(d_sep, a_lat, d_dev, safe_distance, dtype=np.float64):
    """The six safety statistics of ONE episode from its record lists (d_sep_record, a_lat_record, d_dev_record; the
    d_sep / a_lat / d_dev columns of simulate(columns="testing")), as the fused evaluator keeps them per lane
    (include/acas2d.h, Acas2dEvalStats).  They cover the rows of the episode's step() calls: ROW 0, which
    ACAS2DGame.__init__ appends before the first step, IS DROPPED, so step row i is list entry i.
      min_sep       min of d_sep over the step rows, min_sep_step the 1-based index of the first row that attains it
      los_steps     number of step rows with d_sep < safe_distance
      max_a_lat     max of |a_lat|;  max_dev: max of |d_dev|;  sum_dev: sum of |d_dev|, added row by row in `dtype`
    Minimum and maxima start from +inf / 0 and take a row only if it compares below / above the held value, so a NaN
    never replaces one (min_sep_step stays 0 if no row compared below +inf).  Returns a dict of numpy scalars in `dtype`
    (the two counts: int)."""
    dt = np.dtype(dtype).type
    d_sep, a_lat, d_dev = (np.asarray(v, dtype=dt)[1:] for v in (d_sep, a_lat, d_dev))
    if not (len(d_sep) == len(a_lat) == len(d_dev)):
        raise ValueError("record lists of different lengths: %d, %d, %d" % (len(d_sep) + 1, len(a_lat) + 1, len(d_dev) + 1))
    safe = dt(safe_distance)
    m, m_step, los, ma, md, sd = dt(np.inf), 0, 0, dt(0), dt(0), dt(0)
    for i, (d, a, v) in enumerate(zip(d_sep, np.abs(a_lat), np.abs(d_dev)), start=1):
        if d < m:
            m, m_step = d, i
        los += int(d < safe)
        ma = a if a > ma else ma
        md = v if v > md else md
        sd = dt(sd + v)
    return {"min_sep": m, "min_sep_step": m_step, "los_steps": los, "max_a_lat": ma, "max_dev": md, "sum_dev": sd}


def safety_summary(stats, steps):
    """episode_safety()'s dict under the keys of evaluate_policies_fused(safety=True) (SAFETY_KEYS): the mean deviation
    is sum_dev over the steps - 1 step rows (`steps`: game.steps at done, "Time Steps"), 0 where steps <= 1."""
    dt = type(stats["sum_dev"])
    return {"min_separation": stats["min_sep"], "min_separation_step": stats["min_sep_step"], "los_steps": stats["los_steps"],
            "max_abs_a_lat": stats["max_a_lat"], "max_abs_deviation": stats["max_dev"],
            "mean_abs_deviation": stats["sum_dev"] / dt(steps - 1) if steps > 1 else dt(0)}


def safety_columns(cols, safe_distance, dtype=np.float64):
    """episode_safety() for every episode of simulate(columns="testing")'s table: a dict of six lists under SAFETY_KEYS,
    one entry per episode -- what evaluate_policies_fused(safety=True) returns per policy, from the slow path."""
    out = {k: [] for k in SAFETY_KEYS}
    for d_sep, a_lat, d_dev, steps in zip(cols["d_sep"], cols["a_lat"], cols["d_dev"], cols["Time Steps"]):
        row = safety_summary(episode_safety(d_sep, a_lat, d_dev, safe_distance, dtype), int(steps))
        for k in SAFETY_KEYS:
            out[k].append(row[k])
    return out


# ---- Monte Carlo campaigns (acas2d_monte_carlo_*, policy.MonteCarlo): the accumulators' definitions, on the host -----------
MONTE_CARLO_INT_KEYS = ("outcome_count", "sum_steps", "los_episodes", "sum_los_steps", "sep_hist")
MONTE_CARLO_LANE_KEYS = ("lane_return_sum", "lane_return_sq", "lane_worst_sep", "lane_worst_episode")
MONTE_CARLO_KEYS = MONTE_CARLO_INT_KEYS + MONTE_CARLO_LANE_KEYS


def separation_bin(min_sep, n_bins, inv_bin_width, dtype=np.float64):
    """The histogram bin of an episode's minimum separation, as the Monte Carlo kernel finds it (include/acas2d.h,
    Acas2dMonteCarlo): b = (int)(min_sep * inv_bin_width), the product evaluated in `dtype` with inv_bin_width rounded to
    it; a bin >= n_bins and a non-finite value (+-inf, NaN) go to bin n_bins - 1, and a negative product (no separation is)
    to bin 0.  Scalars or arrays; returns int64."""
    dt = np.dtype(dtype).type
    with np.errstate(invalid="ignore", over="ignore"):
        scaled = np.asarray(min_sep, dtype=dt) * dt(inv_bin_width)
        ok = np.abs(scaled) < dt(2147483648.0)                       # finite and an int32 (NaN compares false)
        q = np.where(ok, scaled, dt(0)).astype(np.int64)             # truncation toward zero, as the C cast
    return np.where(ok & (q < n_bins), np.maximum(q, 0), n_bins - 1).astype(np.int64)


def monte_carlo_empty(n_policies, n_lanes, n_bins, dtype=np.float64):
    """The accumulators of a campaign before its first episode: lane_worst_sep +inf, everything else 0."""
    K, L = int(n_policies), int(n_lanes)
    return {"outcome_count": np.zeros((K, 4), np.int64), "sum_steps": np.zeros(K, np.int64),
            "los_episodes": np.zeros(K, np.int64), "sum_los_steps": np.zeros(K, np.int64),
            "sep_hist": np.zeros((K, int(n_bins)), np.int64), "lane_return_sum": np.zeros((K, L), np.float64),
            "lane_return_sq": np.zeros((K, L), np.float64), "lane_worst_sep": np.full((K, L), np.inf, np.dtype(dtype)),
            "lane_worst_episode": np.zeros((K, L), np.uint32)}


def monte_carlo_reduce(per_episode_results, n_bins, inv_bin_width, dtype=np.float64, acc=None, first_episode=0):
    """Fold a list of evaluate_policies_fused(safety=True) result dicts -- one per episode counter, in counter order, each
    [K, n_lanes] -- into the accumulators of acas2d_monte_carlo_* (include/acas2d.h, Acas2dMonteCarlo): the
    specification of the kernel's folding and the tests' reference.  `acc`: accumulators to go on from (a copy is
    returned; default: monte_carlo_empty()), `first_episode`: the counter of the first dict.  total_reward is taken as
    the float64 value of the launch's `dtype` result (evaluate_policies_fused returns it so), min_separation in `dtype`."""
    dt = np.dtype(dtype)
    acc = None if acc is None else {k: np.array(v, copy=True) for k, v in acc.items()}
    for n, res in enumerate(per_episode_results):
        oc = np.asarray(res["outcome"]).astype(np.int64)
        K, L = oc.shape
        if acc is None:
            acc = monte_carlo_empty(K, L, n_bins, dt)
        steps, los = np.asarray(res["steps"]).astype(np.int64), np.asarray(res["los_steps"]).astype(np.int64)
        sep = np.asarray(res["min_separation"]).astype(dt, copy=False)
        ret = np.asarray(res["total_reward"]).astype(dt).astype(np.float64)
        b = separation_bin(sep, n_bins, inv_bin_width, dt)
        for k in range(K):
            acc["outcome_count"][k] += np.bincount(oc[k], minlength=4)[:4]
            acc["sep_hist"][k] += np.bincount(b[k], minlength=n_bins)
        acc["sum_steps"] += steps.sum(1)
        acc["los_episodes"] += (los > 0).sum(1)
        acc["sum_los_steps"] += los.sum(1)
        acc["lane_return_sum"] = acc["lane_return_sum"] + ret               # plain float64 adds, counter after counter
        acc["lane_return_sq"] = acc["lane_return_sq"] + ret * ret
        with np.errstate(invalid="ignore"):
            better = sep < acc["lane_worst_sep"]                          # strictly: the first occurrence keeps its place
        acc["lane_worst_sep"] = np.where(better, sep, acc["lane_worst_sep"]).astype(dt)
        acc["lane_worst_episode"] = np.where(better, np.uint32(first_episode + n), acc["lane_worst_episode"]).astype(np.uint32)
    if acc is None:
        raise ValueError("monte_carlo_reduce needs at least one result, or acc")
    return acc


def wilson_interval(k, n, z=1.959963984540054):
    """Wilson score interval of a binomial rate k / n (default z: 95 %); (nan, nan) at n = 0."""
    k, n = np.asarray(k, np.float64), np.asarray(n, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        p = k / n
        den = 1.0 + z * z / n
        mid = (p + z * z / (2.0 * n)) / den
        half = z * np.sqrt(p * (1.0 - p) / n + z * z / (4.0 * n * n)) / den
    return mid - half, mid + half


def monte_carlo_summary(acc, baseline=None, hist_max=None):
    """What a campaign's accumulators say, per policy (arrays [K]): episodes, the goal / collision / timeout counts and
    rates, the collision rate's Wilson 95 % interval (collision_rate_lo / _hi), the rate of episodes that lost separation
    (los_rate), mean los steps per episode, mean_steps, mean_return and its standard error (return_sem) -- from the per-lane
    sums, reduced in float64 in lane order; the standard error takes the episodes as independent -- and the histogram
    with its n_bins + 1 edges (hist_edges; given hist_max = n_bins bin widths, else in units of a bin).
    baseline = k0 adds risk_ratio: each policy's collision rate over policy k0's.  A baseline without collisions gives inf
    (nan for a policy that has none either), never an exception."""
    oc = np.asarray(acc["outcome_count"], np.int64)
    n = oc.sum(1)
    nf = n.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        rate = lambda c: np.asarray(c, np.float64) / nf  # noqa: E731
        s1 = np.zeros(len(n), np.float64)
        s2 = np.zeros(len(n), np.float64)
        for k in range(len(n)):                                           # sequential, lane after lane (cumsum adds in order)
            s1[k] = np.cumsum(np.asarray(acc["lane_return_sum"][k], np.float64))[-1]
            s2[k] = np.cumsum(np.asarray(acc["lane_return_sq"][k], np.float64))[-1]
        mean = s1 / nf
        var = np.maximum(s2 / nf - mean * mean, 0.0) * (nf / (nf - 1.0))
        lo, hi = wilson_interval(oc[:, 2], n)
        out = {"episodes": n, "goals": oc[:, 1], "collisions": oc[:, 2], "timeouts": oc[:, 3], "unfinished": oc[:, 0],
               "goal_rate": rate(oc[:, 1]), "collision_rate": rate(oc[:, 2]), "timeout_rate": rate(oc[:, 3]),
               "collision_rate_lo": lo, "collision_rate_hi": hi, "los_rate": rate(acc["los_episodes"]),
               "mean_los_steps": rate(acc["sum_los_steps"]), "mean_steps": rate(acc["sum_steps"]), "mean_return": mean,
               "return_sem": np.sqrt(var / nf), "sep_hist": np.asarray(acc["sep_hist"], np.int64)}
        n_bins = out["sep_hist"].shape[1]
        out["hist_edges"] = np.arange(n_bins + 1, dtype=np.float64) * (1.0 if hist_max is None else float(hist_max) / n_bins)
        if baseline is not None:
            out["risk_ratio"] = out["collision_rate"] / out["collision_rate"][int(baseline)]
    return out


# ---- encounter search (acas2d_encounter_*, policy.EncounterSearch): the definitions of the three kernels, on the host -------
# An encounter is a point of the unit cube with 4 (N + 1) coordinates (coordinate 4 e + j: word j of entity e's Philox block;
# entity 0 is the player, n + 1 traffic n); the proposal is one piecewise-constant density per coordinate, p[c][b] on B equal
# bins.  No random numbers are drawn here: the caller brings the uniforms.
SEARCH_HISTORY_COLUMNS = ("finished", "unfinished", "n_elite", "gamma_q", "gamma", "n_event", "sum_w_event", "sum_w2_event",
                          "sum_w", "sum_w2", "min_score", "min_candidate", "generation")
SEARCH_HISTORY_WIDTH = 16                     # the three last columns are spare (0)
_T_MAX = 1.0 - 2.0 ** -53


def search_active_coordinates(config):
    """bool [4 (N + 1)]: the coordinates that reach the state under the reset distribution -- the player's heading (word z);
    traffic 0's x (through the starts_down bit only), z, and w iff the airspeed factor varies; traffic n >= 1's x, y, z, and w
    under the same condition.  The others are drawn nominally, never refit, and add nothing to the likelihood ratio."""
    N = int(config.n_traffic)
    speed = config.airspeed_factor_min != config.airspeed_factor_max
    act = np.zeros((N + 1, 4), bool)
    act[0, 2] = True
    act[1] = [True, False, True, speed]
    act[2:] = [True, True, True, speed]
    return act.reshape(-1)


def search_tables(p):
    """The tables the sampler reads beside p [..., B]: cdf [..., B + 1] (cdf[0] = 0, cdf[b + 1] = cdf[b] + p[b], added one
    after the other in ascending b) and log_ratio [..., B] = -log(B p[b])."""
    p = np.asarray(p, np.float64)
    B = p.shape[-1]
    cdf = np.zeros(p.shape[:-1] + (B + 1,), np.float64)
    for b in range(B):
        cdf[..., b + 1] = cdf[..., b] + p[..., b]
    with np.errstate(divide="ignore"):
        log_ratio = -np.log(B * p)
    return cdf, log_ratio


def search_sample(tables, active, u):
    """The inverse CDF of one policy's proposal on uniforms u [L, n_coord]: tables = (p, cdf, log_ratio), each [n_coord, ...].
    Per active coordinate: b = the largest bin with cdf[b] <= u (at most B - 1), t = (u - cdf[b]) / p[b] clamped to
    [0, 1 - 2^-53] (a NaN to 0), c = (b + t) / B; an inactive one keeps c = u (bin min(int(u B), B - 1)).  Returns c [L, n_coord]
    float64, bins [L, n_coord] uint8 and log_w [L]: the active coordinates' log_ratio[b], added in ascending coordinate order
    from 0."""
    p, cdf, log_ratio = (np.asarray(t, np.float64) for t in tables)
    u = np.asarray(u, np.float64)
    L, NC = u.shape
    B = p.shape[-1]
    c, bins, log_w = u.copy(), np.zeros((L, NC), np.uint8), np.zeros(L, np.float64)
    for j in range(NC):
        uj = u[:, j]
        if not active[j]:
            bins[:, j] = np.minimum((uj * B).astype(np.int64), B - 1)
            continue
        b = np.where(cdf[j, None, :B] <= uj[:, None], np.arange(B)[None, :], 0).max(1)
        with np.errstate(invalid="ignore", divide="ignore"):
            t = (uj - cdf[j, b]) / p[j, b]
            t = np.where(t > 0.0, t, 0.0)
        t = np.where(t < _T_MAX, t, _T_MAX)
        c[:, j] = (b.astype(np.float64) + t) / float(B)
        bins[:, j] = b
        log_w = log_w + log_ratio[j, b]
    return c, bins, log_w


def _py_mod360(a):
    r = np.where(a >= 360.0, a - 360.0, a)
    r = np.where(a < 0.0, a + 360.0, r)
    out = ~((a > -360.0) & (a < 720.0))
    if np.any(out):
        r = np.where(out, np.mod(a, 360.0), r)
    return r


def encounter_from_uniforms(config, c, dtype=np.float64):
    """The encounters of coordinates c [L, 4 (N + 1)]: the reset distribution's float64 formulas (game.py:80-116, as the
    engine's reset evaluates them) with c in place of the uniforms and starts_down = c_x >= 0.5 for traffic 0, rounded to
    `dtype`.  Returns own [L, 4] = (x, y, psi, v), traffic [L, N, 4], goal [L, 2]."""
    cc = config.to_c()
    N = int(config.n_traffic)
    c = np.asarray(c, np.float64).reshape(-1, N + 1, 4)
    L = c.shape[0]
    uni = lambda a, b, u: a + (b - a) * u  # noqa: E731
    own = np.empty((L, 4), np.float64)
    own[:, 0], own[:, 1], own[:, 3] = cc.own_x0, cc.own_y0, cc.own_v
    own[:, 2] = _py_mod360(cc.own_heading0 + uni(-cc.own_heading_jitter, cc.own_heading_jitter, c[:, 0, 2]))
    trf = np.empty((L, N, 4), np.float64)
    down = (c[:, 1, 0] >= 0.5).astype(np.float64)
    trf[:, :, 0] = uni(0.0, cc.tn_x_max, c[:, 1:, 0])
    trf[:, :, 1] = uni(0.0, cc.tn_y_max, c[:, 1:, 1])
    trf[:, :, 2] = uni(0.0, 360.0, c[:, 1:, 2])
    trf[:, :, 3] = uni(cc.speed_factor_min, cc.speed_factor_max, c[:, 1:, 3]) * cc.airspeed
    trf[:, 0, 0] = cc.t0_x
    trf[:, 0, 1] = cc.t0_y_base + (down * cc.t0_y_span)
    trf[:, 0, 2] = _py_mod360((cc.t0_heading_base + (down * cc.t0_heading_step)) +
                              uni(-cc.t0_heading_jitter, cc.t0_heading_jitter, c[:, 1, 2]))
    goal = np.tile(np.array([cc.goal_x, cc.goal_y], np.float64), (L, 1))
    dt = np.dtype(dtype)
    return own.astype(dt), trf.astype(dt), goal.astype(dt)


def search_select(score, outcome, log_w, n_quantile, level, weighted=True):
    """One policy's selection from min_separation `score` [L] (its dtype is the engine's), `outcome` [L] and log_w [L]: a
    candidate's score is its min_separation where the episode finished and the value is a number, else +inf; gamma_q = the
    n_quantile-th smallest score, gamma = max(gamma_q, level rounded to the dtype); the elite: score <= gamma and finite (ties
    at gamma are all elite); W = exp(log_w) if weighted else 1.  Returns {"score", "elite" (bool), "elite_w" (W on the elite,
    else 0), "row"}: row is the history row of SEARCH_HISTORY_COLUMNS without its generation (math.fsum sums; the first
    candidate of the smallest score)."""
    import math
    score = np.asarray(score)
    dt = score.dtype.type
    oc = np.asarray(outcome)
    L = score.shape[0]
    s = np.where((oc != 0) & ~np.isnan(score), score, dt(np.inf)).astype(score.dtype)
    gamma_q = np.sort(s, kind="stable")[int(n_quantile) - 1]
    gamma = max(gamma_q, dt(level))
    elite = (s <= gamma) & np.isfinite(s)
    event = s <= dt(level)
    w = np.exp(np.asarray(log_w, np.float64)) if weighted else np.ones(L, np.float64)
    row = np.zeros(SEARCH_HISTORY_WIDTH, np.float64)
    row[:12] = [int((oc != 0).sum()), int((oc == 0).sum()), int(elite.sum()), gamma_q, gamma, int(event.sum()),
                math.fsum(w[event]), math.fsum(w[event] * w[event]), math.fsum(w), math.fsum(w * w), s.min(), int(np.argmin(s))]
    return {"score": s, "elite": elite, "elite_w": np.where(elite, w, 0.0), "row": row}


def search_refit(p, active, bins, elite_w, alpha, p_floor):
    """One policy's new proposal from p [n_coord, B], the candidates' bins [L, n_coord] and elite_w [L]: per active coordinate
    S[b] = the elite weight in bin b (math.fsum), S_tot = their sum in ascending b; unless S_tot > 0 the row stays; else
    p_new[b] = max((1 - alpha) p[b] + alpha (S[b] / S_tot), p_floor), divided by the sum of p_new in ascending b.  Inactive rows
    are returned as they are."""
    import math
    p = np.array(p, np.float64, copy=True)
    bins, w = np.asarray(bins), np.asarray(elite_w, np.float64)
    B = p.shape[-1]
    keep = 1.0 - float(alpha)
    elite = w != 0.0                                             # (a non-elite adds nothing)
    bins, w = bins[elite], w[elite]
    for j in np.nonzero(np.asarray(active))[0]:
        S = np.array([math.fsum(w[bins[:, j] == b]) for b in range(B)], np.float64)
        s_tot = 0.0
        for b in range(B):
            s_tot = s_tot + S[b]
        if not s_tot > 0.0:
            continue
        pn = np.maximum((keep * p[j]) + (float(alpha) * (S / s_tot)), float(p_floor))
        norm = 0.0
        for b in range(B):
            norm = norm + pn[b]
        p[j] = pn / norm
    return p


def search_estimate(history_rows, n_candidates, first_generation=0):
    """The importance-sampling estimate of the event's probability from history rows [G, ..., SEARCH_HISTORY_WIDTH] (further
    axes, e.g. policies, are kept): per generation p_g = sum_w_event / L, its standard error sqrt((sum_w2_event / L - p_g^2) /
    (L - 1)) and the effective sample size sum_w^2 / sum_w2; and over the generations from first_generation on the mean of
    p_g and its standard error sqrt(sum se_g^2) / G'.  A generation's proposal is fixed before the generation is drawn, so every
    p_g is unbiased and so is their mean."""
    h = np.asarray(history_rows, np.float64)
    L = float(n_candidates)
    p_g = h[..., 6] / L
    with np.errstate(invalid="ignore", divide="ignore"):
        se_g = np.sqrt(np.maximum(h[..., 7] / L - p_g * p_g, 0.0) / (L - 1.0))
        ess = h[..., 8] * h[..., 8] / h[..., 9]
    sel = slice(int(first_generation), None)
    n = p_g[sel].shape[0]
    return {"p_generation": p_g, "se_generation": se_g, "ess": ess, "n_event": h[..., 5], "generations": n,
            "p": p_g[sel].mean(0) if n else np.full(p_g.shape[1:], np.nan),
            "se": np.sqrt((se_g[sel] ** 2).sum(0)) / n if n else np.full(p_g.shape[1:], np.nan)}


# ---- sensor noise and actuator disturbance (acas2d_evaluate_policies_disturbed_*, acas2d_monte_carlo_disturbed_*) ----------
DISTURBANCE_TAG = 0x64697374                   # "dist": xor-ed into the key's high word
DISTURBANCE_SLOT_SHIFT = 20                    # counter word 3 = step | slot << 20
DISTURBANCE_PHILOX_ROUNDS = 7                  # the reset's generator (csrc/acas2d_kernels.hpp, philox4x32)
OBSERVATION_BOX = ((0.0, 1.0), (-1.0, 1.0), (-1.0, 1.0))      # separation, d_cpa, v_closing (environment.py:19-20)


def philox4x32(counter, key, rounds=DISTURBANCE_PHILOX_ROUNDS):
    """Philox4x32 on arrays: counter [..., 4] and key [..., 2] (or a pair of ints) of 32-bit words -> words [..., 4] uint32."""
    m32 = np.uint64(0xFFFFFFFF)
    c = [np.asarray(counter)[..., i].astype(np.uint64) & m32 for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) & m32 for i in range(2)]
    for _ in range(int(rounds)):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & m32]
        k = [(k[0] + np.uint64(0x9E3779B9)) & m32, (k[1] + np.uint64(0xBB67AE85)) & m32]
    return np.stack(np.broadcast_arrays(*c), axis=-1).astype(np.uint32)


def disturbance_words(seed, lane, episode, step, slot):
    """The Philox block of the disturbance at (lane, episode, step, slot), broadcast over array arguments -> [..., 4] uint32.
    Counter (lane lo, lane hi, episode, step | slot << 20), key (seed lo, seed hi ^ DISTURBANCE_TAG).  lane: the RNG index
    env_offset + index within the policy's block; step: game.steps before the step's increment; slot 0 the actuator,
    slot n + 1 traffic n."""
    lane, episode, step, slot = np.broadcast_arrays(*[np.asarray(a, np.uint64) for a in (lane, episode, step, slot)])
    if (step >= (1 << DISTURBANCE_SLOT_SHIFT)).any() or (slot > 64).any() or (episode >= (1 << 32)).any():
        raise ValueError("disturbance_words: step < 2^20, slot <= 64 and episode < 2^32 are required")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    ctr = np.stack([lane & np.uint64(0xFFFFFFFF), lane >> np.uint64(32), episode,
                    step | (slot << np.uint64(DISTURBANCE_SLOT_SHIFT))], axis=-1)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) ^ DISTURBANCE_TAG], np.uint64)
    return philox4x32(ctr, key)


def disturbance_normals(words):
    """The three standard normals (z_sep, z_cpa, z_closing) of blocks [..., 4] in float64: u_i = fl32((w_i >> 8) + 0.5) / 2^24 (the
    float32 uniforms of the kernels, exact in float64), r(u) = sqrt(-2 ln u), z_sep = r(u1) cos(2 pi u2), z_cpa = r(u1) sin(2 pi
    u2), z_closing = r(u3) cos(2 pi u4).  The actuator slot reads z_sep.  The kernels evaluate the same formulas with the
    hardware's approximate float32 log, sqrt, sin and cos: acas2d_disturbance_draw_f32 gives their values.
    fl32: the kernels form k + 0.5 in float32 (u01f()), which holds it only for k < 2^23; from there on it is a tie and goes
    to the even neighbour -- k for an even k, k + 1 for an odd one.  Nothing of that shows but next to u = 1, where ln u is all
    rounding: k = 2^24 - 1 gives u = 1 and the normal 0 (not 2.4e-4 times the cosine), k = 2^24 - 2 and 2^24 - 3 give
    r = 4.9e-4 (not 4.2e-4 and 5.5e-4)."""
    w = np.asarray(words, np.uint32)
    u = ((w >> np.uint32(8)).astype(np.float32) + np.float32(0.5)).astype(np.float64) / 16777216.0
    r1, r3 = np.sqrt(-2.0 * np.log(u[..., 0])), np.sqrt(-2.0 * np.log(u[..., 2]))
    a2, a4 = 2.0 * np.pi * u[..., 1], 2.0 * np.pi * u[..., 3]
    return np.stack([r1 * np.cos(a2), r1 * np.sin(a2), r3 * np.cos(a4)], axis=-1)


def _disturbed(x, s, z, lo, hi):
    """x + s z in float32 with both roundings, then the box by comparisons (a NaN stays, -0 stays); s == 0: x untouched."""
    x = np.asarray(x, np.float32)
    s = np.float32(s)
    if s == 0:
        return x.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        y = (x + (s * np.asarray(z, np.float32)).astype(np.float32)).astype(np.float32)
        return np.where(y < np.float32(lo), np.float32(lo), np.where(y > np.float32(hi), np.float32(hi), y)).astype(np.float32)


def disturb_observation(obs, sigma, normals):
    """The observation the actor reads: obs [..., 5 + 3 N] float32, sigma = (s_sep, s_cpa, s_closing) in normalised units,
    normals [..., N, 3] (slot n + 1's z_sep, z_cpa, z_closing, e.g. from acas2d_disturbance_draw_f32).  Entry 5 + 3 n + c
    becomes x + s_c z in float32 -- the product and the sum each rounded -- and is held to OBSERVATION_BOX[c]; a NaN stays
    a NaN; a channel with s_c == 0 is neither added to nor clamped; the five own-ship entries are never touched."""
    out = np.array(obs, np.float32, copy=True)
    z = np.asarray(normals, np.float32)
    n = (out.shape[-1] - 5) // 3
    if z.shape[-2:] != (n, 3):
        raise ValueError("disturb_observation: normals %s for %d traffic aircraft" % (z.shape, n))
    for c, (lo, hi) in enumerate(OBSERVATION_BOX):
        out[..., 5 + c::3] = _disturbed(out[..., 5 + c::3], sigma[c], z[..., c], lo, hi)
    return out


def disturb_action(action, s_action, normal):
    """The action the aircraft flies: the actor's clipped action + s_action z in float32 (two roundings), held to [-1, 1]
    again; a NaN stays a NaN; s_action == 0 leaves it untouched."""
    return _disturbed(action, s_action, normal, -1.0, 1.0)


# ---- time-correlated and biased errors (acas2d_evaluate_policies_correlated_*, acas2d_monte_carlo_correlated_*) -------------
def correlation_gain(rho):
    """The gain q = (float32) sqrt(1 - rho^2) of a channel's Gauss-Markov error, rho a float32 in [0, 1] (arrays: elementwise):
    the square and the difference in float64 (both exact enough that the correctly rounded float64 root, then ONE rounding to
    float32, is what the C entry forms with sqrt())."""
    r = np.asarray(rho, np.float32)
    if not ((r >= 0) & (r <= 1)).all():                                          # (a NaN fails both comparisons)
        raise ValueError("correlation_gain: rho = %r (each in [0, 1])" % (rho,))
    r = r.astype(np.float64)
    return np.sqrt(1.0 - r * r).astype(np.float32)


def correlated_errors(normals, rho):
    """The errors e_t that take the normals' place: `normals` [steps, ...] float32 from an episode's FIRST step on (axis 0 is
    the step), rho a float32 in [0, 1] or an array of them that broadcasts against normals[0] (e.g. one per channel of a last
    axis).  e_0 = z_0;  e_t = (rho e_{t-1}) + (q z_t) in float32 -- two products and a sum, each rounded, no fma -- with
    q = correlation_gain(rho).  Where rho == 0 the result is z's own bits (no arithmetic); rho == 1 repeats e_0."""
    z = np.asarray(normals, np.float32)
    if z.ndim < 1:
        raise ValueError("correlated_errors: normals [steps, ...] are required")
    rho_b = np.broadcast_to(np.asarray(rho, np.float32), z.shape[1:])
    q = correlation_gain(rho_b)
    white = rho_b == 0
    e = z.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(1, z.shape[0]):
            a = (rho_b * e[t - 1]).astype(np.float32)
            b = (q * z[t]).astype(np.float32)
            e[t] = np.where(white, z[t], (a + b).astype(np.float32))
    return e


def correlated_step(held, normals, rho, first):
    """ONE step of that scan, for a state that outlives the call (acas2d_collect_set_correlated_*, whose episodes span launches):
    the new errors e_t from `held` = e_{t-1}, `normals` = z_t (float32 arrays of one shape), rho as in correlated_errors()
    (broadcast against them) and `first`, a bool or bool array: where the step is an episode's first.  e_t = z_t where rho == 0
    or first;  else (rho held) + (q z_t) in float32, two products and a sum, each rounded, no fma, q = correlation_gain(rho).
    Returns e_t: the caller keeps it as the next step's `held` where rho != 0 (a channel with rho == 0 holds nothing)."""
    z = np.asarray(normals, np.float32)
    h = np.broadcast_to(np.asarray(held, np.float32), z.shape)
    rho_b = np.broadcast_to(np.asarray(rho, np.float32), z.shape)
    q = correlation_gain(rho_b)
    with np.errstate(invalid="ignore", over="ignore"):
        a = (rho_b * h).astype(np.float32)
        b = (q * z).astype(np.float32)
        return np.where((rho_b == 0) | np.broadcast_to(np.asarray(first, bool), z.shape), z, (a + b).astype(np.float32))


# ---- response delay and actuation lag (acas2d_evaluate_policies_delayed_*, acas2d_monte_carlo_delayed_*) --------------------
def response_gain(lag):
    """The gain g = (float32)(1 - lag) of the first-order lag, `lag` a float32 in [0, 1]: the difference in float64 (exact),
    then ONE rounding to float32, as the C entry forms it."""
    lam = np.float32(lag)
    if not 0 <= lam <= 1:                                                        # (a NaN fails both comparisons)
        raise ValueError("response_gain: lag = %r (in [0, 1])" % (lag,))
    return np.float32(1.0 - np.float64(lam))


def response_delay(actions, delay):
    """The dead time: `actions` [steps, ...] from an episode's FIRST step on (axis 0 is the step), the actor's clipped actions;
    returns the commands c of the same shape, c_s = a_{s - delay} and 0 for the first `delay` steps (nothing has arrived: the
    aircraft flies straight).  delay == 0 gives the actions' own bits; delay >= steps gives all zeros."""
    a = np.asarray(actions)
    d = int(delay)
    if a.ndim < 1 or d != delay or d < 0:
        raise ValueError("response_delay: actions [steps, ...] and a whole delay of at least 0 are required")
    out = np.zeros_like(a)
    if d < a.shape[0]:
        out[d:] = a[:a.shape[0] - d]
    return out


def response_lag_step(held, commands, lag, first, dtype=np.float32):
    """ONE step of the lag: u_s = clamp((lag u_{s-1}) + (g c_s)) from `held` = u_{s-1} and `commands` = c_s (arrays of one
    shape), with 0 in u_{s-1}'s place where `first` (a bool or bool array: the step is an episode's first); two products and a
    sum in `dtype`, each rounded, no fma, g = response_gain(lag), then fmin(fmax(., -1), 1) -- which sends a NaN to -1, as
    fminf(fmaxf()) does.  lag == 0: the commands' own bits (no arithmetic)."""
    c = np.asarray(commands, dtype)
    lam = np.float32(lag)
    g = response_gain(lam)
    if lam == 0:
        return c.copy()
    prev = np.where(np.broadcast_to(np.asarray(first, bool), c.shape), dtype(0), np.broadcast_to(np.asarray(held, dtype), c.shape))
    with np.errstate(invalid="ignore", over="ignore"):
        a = (dtype(lam) * prev).astype(dtype)
        b = (dtype(g) * c).astype(dtype)
        return np.fmin(np.fmax((a + b).astype(dtype), dtype(-1)), dtype(1)).astype(dtype)


def response_lag(commands, lag, dtype=np.float32):
    """The first-order lag behind the dead time: `commands` [steps, ...] from an episode's FIRST step on; returns u of the same
    shape, u_s = clamp((lag u_{s-1}) + (g c_s)) with u = 0 in front of the first step (response_lag_step() is one step of it).
    lag == 0 gives the commands' own bits; lag == 1 (g = 0) gives zeros: the aircraft never responds."""
    c = np.asarray(commands, dtype)
    if c.ndim < 1:
        raise ValueError("response_lag: commands [steps, ...] are required")
    u = np.empty_like(c)
    for s in range(c.shape[0]):
        u[s] = response_lag_step(u[s - 1] if s else np.zeros_like(c[0]), c[s], lag, s == 0, dtype)
    return u
