#!/usr/bin/env python3
"""What time-correlated errors cost and what they show, one JSON line per record (policy.MonteCarlo with a
policy.CorrelatedDisturbance: acas2d_monte_carlo_correlated_*).

cost    per case LANESxEPISODESxN_TRAFFICxK[g] (g: the group-cooperative launch), float32, K randomly initialised policies:
          (a) white       MonteCarlo.run(EPISODES) under a Disturbance -- monte_carlo_disturbed_kernel, untouched by this model
          (b) correlated  the same sigmas and seed as a CorrelatedDisturbance with every rho 0.5: every process is advanced and
                          its state goes through the wave's LDS at every step
        The two fly different actions from the second step on, so they do not play the same steps: sum_steps of both is
        recorded and per_step_ratio is the ratio of the kernel times per env step.  Wall clock between device
        synchronisations, and the kernel alone between HIP events; one warm-up of every variant, then --reps repetitions,
        the variants alternating in one process; median and min - max, `spread` is (max - min) / median.
curve   the committed reference policy (tests/golden/ref_policy_best_model.npz, one aircraft) and the all-zero policy under
        sensor noise of 4 and 8 % of the normalised range on all three channels, then actuator noise of 0.2 and 0.4, each at
        rho 0, 0.9, 0.99 and 1 on the disturbed channels: the columns of tools/bench_disturbance.py's curve, whose rows the
        rho = 0 levels must reproduce.  One campaign per level, the same encounters and the same normals at every level.

usage: bench_correlated.py [--cases ...] [--reps 5] [--curve 65536x8] [--out profiles/correlated_timing.jsonl]"""
import torch

import campaign_bench as B
from campaign_bench import DEV, N_BINS, g

SIGMAS = dict(sep=0.04, cpa=0.04, closing=0.04, action=0.2, seed=7)
RHO = 0.5


def cost(lanes, episodes, N, K, group, reps):
    pols = B.policies(N, K)
    white, corr = g.Disturbance.normalised(**SIGMAS), g.CorrelatedDisturbance.normalised(rho=RHO, **SIGMAS)

    def make(dist):
        return g.MonteCarlo(pols, lanes, n_traffic=N, n_bins=N_BINS, group=group, device=DEV, disturbance=dist)

    acc, runs, summary = B.time_variants(make, {"white": white, "correlated": corr}, episodes, reps)
    a, b = acc["white"], acc["correlated"]                                      # the warm-up's: the steps each plays
    rec = {"bench": "correlated_cost", "lanes": lanes, "episodes_per_lane": episodes, "n_traffic": N, "policies": K, "group": group,
           "dtype": "float32", "reps": reps, "disturbance": corr.to_dict(), "sum_steps_white": [int(x) for x in a["sum_steps"]],
           "sum_steps_correlated": [int(x) for x in b["sum_steps"]], "device": torch.cuda.get_device_name(0),
           "method": "one warm-up, variants alternating, median of reps; white / correlated: wall clock between synchronisations, "
                     "*_kernel: HIP events around the C call; seconds"}
    rec.update(summary)
    rec["correlated_over_white"] = rec["correlated_s"] / rec["white_s"]
    rec["correlated_kernel_over_white_kernel"] = rec["correlated_kernel_s"] / rec["white_kernel_s"]
    rec["apart_beyond_spreads"] = bool(min(runs["correlated_kernel"]) > max(runs["white_kernel"]) or
                                       max(runs["correlated_kernel"]) < min(runs["white_kernel"]))
    rec["per_step_ratio"] = rec["correlated_kernel_over_white_kernel"] * sum(rec["sum_steps_white"]) / sum(rec["sum_steps_correlated"])
    return rec


def curve(lanes, episodes):
    levels = [g.CorrelatedDisturbance.normalised(sep=s, cpa=s, closing=s, seed=7, rho=rho) for s in (0.04, 0.08) for rho in (0.0, 0.9, 0.99, 1.0)] + \
             [g.CorrelatedDisturbance.normalised(action=a, seed=7, rho=rho) for a in (0.2, 0.4) for rho in (0.0, 0.9, 0.99, 1.0)]
    return B.curve(levels, lanes, episodes, "correlated_curve")


if __name__ == "__main__":
    B.main("bench_correlated.py", cost, curve)
