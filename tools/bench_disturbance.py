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
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gym_acas2d_amd as g  # noqa: E402

DEV = "cuda:0"
N_BINS = 64
TINY = 1e-30


def policies(N, K):
    out = []
    for seed in range(K):
        torch.manual_seed(seed + 1)
        pol = g.ActorCritic(5 + 3 * N)
        with torch.no_grad():
            pol.action_net.weight.mul_(40.0)
        out.append(pol)
    return out


def spread(runs):
    return (max(runs) - min(runs)) / float(np.median(runs))


def cost(lanes, episodes, N, K, group, reps):
    pols = policies(N, K)
    tiny = g.Disturbance.normalised(sep=TINY, cpa=TINY, closing=TINY, action=TINY, seed=7)
    assert min(tiny.sigma + (tiny.s_action,)) > 0.0

    def make(dist):
        return g.MonteCarlo(pols, lanes, n_traffic=N, n_bins=N_BINS, group=group, device=DEV, disturbance=dist)

    def wall(dist):
        mc = make(dist)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mc.run(episodes, per_launch=episodes)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, mc

    def kernel(dist):
        mc = make(dist)
        ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        mc._launch(episodes, events=ev)
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e-3

    a, b = wall(None)[1].accumulators(), wall(tiny)[1].accumulators()           # warm-up, and the agreement
    agree = all(np.array_equal(a[k], b[k]) for k in g.records.MONTE_CARLO_INT_KEYS)
    lanes_agree = all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in g.records.MONTE_CARLO_LANE_KEYS)
    kernel(None), kernel(tiny)
    runs = {"plain": [], "disturbed": [], "plain_kernel": [], "disturbed_kernel": []}
    for _ in range(reps):
        runs["plain"].append(wall(None)[0])
        runs["disturbed"].append(wall(tiny)[0])
        runs["plain_kernel"].append(kernel(None))
        runs["disturbed_kernel"].append(kernel(tiny))
    rec = {"bench": "disturbance_cost", "lanes": lanes, "episodes_per_lane": episodes, "n_traffic": N, "policies": K, "group": group,
           "dtype": "float32", "reps": reps, "sigma": TINY, "integer_accumulators_equal": bool(agree),
           "lane_accumulators_equal": bool(lanes_agree), "sum_steps": [int(x) for x in a["sum_steps"]],
           "sum_steps_disturbed": [int(x) for x in b["sum_steps"]],
           "device": torch.cuda.get_device_name(0),
           "method": "one warm-up, variants alternating, median of reps; plain / disturbed: wall clock between synchronisations, "
                     "*_kernel: HIP events around the C call; seconds"}
    for name, r in runs.items():
        rec[name + "_s"] = float(np.median(r))
        rec[name + "_runs_s"] = r
        rec[name + "_spread"] = spread(r)
        print("  %-17s median %.4f s   min %.4f   max %.4f" % (name, np.median(r), min(r), max(r)), flush=True)
    rec["disturbed_over_plain"] = rec["disturbed_s"] / rec["plain_s"]
    rec["disturbed_kernel_over_plain_kernel"] = rec["disturbed_kernel_s"] / rec["plain_kernel_s"]
    rec["apart_beyond_spreads"] = bool(min(runs["disturbed_kernel"]) > max(runs["plain_kernel"]))
    # per env step: where the clamp to the observation box moves an entry that lay outside it, the two campaigns no longer
    # play the same steps (integer_accumulators_equal is false), and the ratio of the times is not the ratio of the costs
    rec["per_step_ratio"] = rec["disturbed_kernel_over_plain_kernel"] * sum(rec["sum_steps"]) / sum(rec["sum_steps_disturbed"])
    return rec


def curve(lanes, episodes):
    ref = g.load_sb3_policy(os.path.join(ROOT, "tests", "golden", "ref_policy_best_model.npz"))
    D = g.ACAS2DConfig().obs_dim
    zero = (torch.zeros(64, D), torch.zeros(64), torch.zeros(64, 64), torch.zeros(64), torch.zeros(1, 64), torch.zeros(1))
    levels = [g.Disturbance.normalised(sep=s, cpa=s, closing=s, seed=7) for s in (0.0, 0.01, 0.02, 0.04, 0.08)] + \
             [g.Disturbance.normalised(action=a, seed=7) for a in (0.1, 0.2, 0.4)]
    out = []
    for level in levels:
        mc = g.MonteCarlo([ref, zero], lanes, n_traffic=1, n_bins=N_BINS, device=DEV, disturbance=level)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s = mc.run(episodes, per_launch=episodes).summary(baseline=1)
        wall = time.perf_counter() - t0
        rec = {"bench": "disturbance_curve", "policy": "tests/golden/ref_policy_best_model.npz", "baseline": "zero", "lanes": lanes,
               "episodes_per_lane": episodes, "disturbance": level.to_dict(), "seconds": wall, "device": torch.cuda.get_device_name(0)}
        for key in ("episodes", "collisions", "collision_rate", "collision_rate_lo", "collision_rate_hi", "los_rate", "goal_rate",
                    "timeout_rate", "risk_ratio", "mean_steps"):
            rec[key] = [int(x) if s[key].dtype.kind == "i" else float(x) for x in s[key]]
        rec["closest"] = [float(w[0][2]) for w in mc.worst(1)]
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="65536x8x1x1,65536x8x1x8,65536x8x8x1,65536x8x8x8,65536x8x16x1g")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--curve", metavar="LANESxEPISODES", default="65536x8")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_disturbance.py measures on the GPU"
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        if sink:
            sink.write(json.dumps(rec) + "\n")
            sink.flush()

    for c in [c for c in args.cases.split(",") if c]:
        group = c.endswith("g")
        lanes, episodes, N, K = (int(x) for x in c.rstrip("g").split("x"))
        print("case %s" % c, flush=True)
        rec = cost(lanes, episodes, N, K, group, args.reps)
        print(json.dumps(rec), flush=True)
        emit(rec)
    if args.curve and args.curve != "none":
        lanes, episodes = (int(x) for x in args.curve.lower().split("x"))
        for rec in curve(lanes, episodes):
            emit(rec)
