#!/usr/bin/env python3
"""What a pilot response delay and an actuation lag cost and what they show, one JSON line per record (policy.MonteCarlo with a
policy.DelayedDisturbance: acas2d_monte_carlo_delayed_*).

cost    per case LANESxEPISODESxN_TRAFFICxK[g] (g: the group-cooperative launch), float32, K randomly initialised policies,
        every variant under the same sigmas, seed and rho 0.5:
          (a) correlated  MonteCarlo.run(EPISODES) under a CorrelatedDisturbance -- monte_carlo_correlated_kernel, untouched by
                          this model
          (b) neutral     a DelayedDisturbance with delay 0 and lag 0: monte_carlo_delayed_kernel with both branches off, the
                          same steps as (a) -- what the new kernel costs before it does anything
          (c) delay       delay = 50 steps alone: one 4-byte load and one 4-byte store per env and step through the ring
          (d) lag         lag = 0.5 alone: one LDS slot per lane
          (e) both        delay = 50, lag = 0.5
        (c) to (e) fly other actions than (a), so they do not play the same steps: sum_steps of every variant is recorded and
        *_per_step is the ratio of the kernel times per env step.  Wall clock between device synchronisations, and the kernel
        alone between HIP events; one warm-up of every variant, then --reps repetitions, the variants alternating in one
        process; median and min - max, `spread` is (max - min) / median.
curve   the committed reference policy (tests/golden/ref_policy_best_model.npz, one aircraft) and the all-zero policy with no
        sensor and no actuator noise at delays of 0, 10, 25, 50 and 100 steps, each without a lag and with lag 0.9.  One
        campaign per level, the same encounters at every level.

usage: bench_response.py [--cases ...] [--reps 5] [--curve 65536x8] [--out profiles/response_timing.jsonl]"""
import torch

import campaign_bench as B
from campaign_bench import DEV, N_BINS, g

SIGMAS = dict(sep=0.04, cpa=0.04, closing=0.04, action=0.2, seed=7)
RHO = 0.5
DELAY, LAG = 50, 0.5


def cost(lanes, episodes, N, K, group, reps):
    pols = B.policies(N, K)
    delayed = lambda **kw: g.DelayedDisturbance.normalised(rho=RHO, **SIGMAS, **kw)  # noqa: E731
    variants = {"correlated": g.CorrelatedDisturbance.normalised(rho=RHO, **SIGMAS), "neutral": delayed(),
                "delay": delayed(delay=DELAY), "lag": delayed(lag=LAG), "both": delayed(delay=DELAY, lag=LAG)}

    def make(dist):
        return g.MonteCarlo(pols, lanes, n_traffic=N, n_bins=N_BINS, group=group, device=DEV, disturbance=dist)

    acc, runs, summary = B.time_variants(make, variants, episodes, reps)
    steps = {name: sum(int(x) for x in a["sum_steps"]) for name, a in acc.items()}      # the warm-up's: the steps each plays
    assert steps["neutral"] == steps["correlated"]                                      # (b) is (a), bit for bit
    rec = {"bench": "response_cost", "lanes": lanes, "episodes_per_lane": episodes, "n_traffic": N, "policies": K, "group": group,
           "dtype": "float32", "reps": reps, "disturbance": variants["both"].to_dict(), "sum_steps": steps,
           "device": torch.cuda.get_device_name(0),
           "method": "one warm-up, variants alternating, median of reps; name: wall clock between synchronisations, "
                     "name_kernel: HIP events around the C call; seconds"}
    rec.update(summary)

    def ratio(name, base):
        """name over base: the kernel times' ratio, whether the two sets of runs lie apart, and the ratio per env step."""
        a, b = runs[name + "_kernel"], runs[base + "_kernel"]
        r = rec[name + "_kernel_s"] / rec[base + "_kernel_s"]
        return {"kernel_ratio": r, "apart_beyond_spreads": bool(min(a) > max(b) or max(a) < min(b)),
                "per_step_ratio": r * steps[base] / steps[name]}

    rec["over_correlated"] = {name: ratio(name, "correlated") for name in ("neutral", "delay", "lag", "both")}
    rec["ring_traffic"] = ratio("delay", "neutral")                                     # the delay alone against neutral
    return rec


def curve(lanes, episodes):
    levels = [g.DelayedDisturbance.normalised(seed=7, delay=d, lag=lag) for lag in (0.0, 0.9) for d in (0, 10, 25, 50, 100)]
    return B.curve(levels, lanes, episodes, "response_curve")


if __name__ == "__main__":
    B.main("bench_response.py", cost, curve)
