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
