#!/usr/bin/env python3
"""What the disturbance model costs and what it shows, one JSON line per record (policy.MonteCarlo with a
policy.Disturbance: acas2d_monte_carlo_disturbed_*).

cost    per case LANESxEPISODESxN_TRAFFICxK[g] (g: the group-cooperative launch), float32, K randomly initialised policies:
          (a) plain      MonteCarlo.run(EPISODES) without a disturbance -- the undisturbed kernel, untouched by the model
          (b) disturbed  the same campaign with all four standard deviations 1e-30: every block is drawn and every add
                         executed, yet no float32 value moves -- so the two play the SAME steps, and the difference is
                         the draws alone
        Before anything is timed the accumulators of (b) are compared with (a)'s and the outcome recorded: equal where every
        perturbed entry lies inside the observation box, which (b) clamps to and (a) does not.  Wall clock
        between device synchronisations, and the kernel alone between HIP events; one warm-up of every variant, then --reps
        repetitions, the variants alternating in one process; median and min - max, `spread` is (max - min) / median.
curve   the committed reference policy (tests/golden/ref_policy_best_model.npz, one aircraft) and the all-zero policy under
        sensor noise of 0, 1, 2, 4, 8 % of the normalised range on all three channels, then actuator noise of 0.1, 0.2, 0.4:
        collision rate with its Wilson 95 % interval, loss-of-separation rate and risk ratio per level.  One campaign
        per level, the same encounters at every level.

usage: bench_disturbance.py [--cases ...] [--reps 5] [--curve 65536x8] [--out profiles/disturbance_timing.jsonl]"""
import numpy as np
import torch

import campaign_bench as B
from campaign_bench import DEV, N_BINS, g

TINY = 1e-30


def cost(lanes, episodes, N, K, group, reps):
    pols = B.policies(N, K)
    tiny = g.Disturbance.normalised(sep=TINY, cpa=TINY, closing=TINY, action=TINY, seed=7)
    assert min(tiny.sigma + (tiny.s_action,)) > 0.0

    def make(dist):
        return g.MonteCarlo(pols, lanes, n_traffic=N, n_bins=N_BINS, group=group, device=DEV, disturbance=dist)

    acc, runs, summary = B.time_variants(make, {"plain": None, "disturbed": tiny}, episodes, reps)
    a, b = acc["plain"], acc["disturbed"]                                       # the warm-up's, and the agreement
    agree = all(np.array_equal(a[k], b[k]) for k in g.records.MONTE_CARLO_INT_KEYS)
    lanes_agree = all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in g.records.MONTE_CARLO_LANE_KEYS)
    rec = {"bench": "disturbance_cost", "lanes": lanes, "episodes_per_lane": episodes, "n_traffic": N, "policies": K, "group": group,
           "dtype": "float32", "reps": reps, "sigma": TINY, "integer_accumulators_equal": bool(agree),
           "lane_accumulators_equal": bool(lanes_agree), "sum_steps": [int(x) for x in a["sum_steps"]],
           "sum_steps_disturbed": [int(x) for x in b["sum_steps"]],
           "device": torch.cuda.get_device_name(0),
           "method": "one warm-up, variants alternating, median of reps; plain / disturbed: wall clock between synchronisations, "
                     "*_kernel: HIP events around the C call; seconds"}
    rec.update(summary)
    rec["disturbed_over_plain"] = rec["disturbed_s"] / rec["plain_s"]
    rec["disturbed_kernel_over_plain_kernel"] = rec["disturbed_kernel_s"] / rec["plain_kernel_s"]
    rec["apart_beyond_spreads"] = bool(min(runs["disturbed_kernel"]) > max(runs["plain_kernel"]))
    # per env step: where the clamp to the observation box moves an entry that lay outside it, the two campaigns no longer
    # play the same steps (integer_accumulators_equal is false), and the ratio of the times is not the ratio of the costs
    rec["per_step_ratio"] = rec["disturbed_kernel_over_plain_kernel"] * sum(rec["sum_steps"]) / sum(rec["sum_steps_disturbed"])
    return rec


def curve(lanes, episodes):
    levels = [g.Disturbance.normalised(sep=s, cpa=s, closing=s, seed=7) for s in (0.0, 0.01, 0.02, 0.04, 0.08)] + \
             [g.Disturbance.normalised(action=a, seed=7) for a in (0.1, 0.2, 0.4)]
    return B.curve(levels, lanes, episodes, "disturbance_curve")


if __name__ == "__main__":
    B.main("bench_disturbance.py", cost, curve)
