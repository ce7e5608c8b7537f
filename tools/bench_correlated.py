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
SIGMAS = dict(sep=0.04, cpa=0.04, closing=0.04, action=0.2, seed=7)
RHO = 0.5


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
    white, corr = g.Disturbance.normalised(**SIGMAS), g.CorrelatedDisturbance.normalised(rho=RHO, **SIGMAS)

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

    a, b = wall(white)[1].accumulators(), wall(corr)[1].accumulators()          # warm-up, and the steps each plays
    kernel(white), kernel(corr)
    runs = {"white": [], "correlated": [], "white_kernel": [], "correlated_kernel": []}
    for _ in range(reps):
        runs["white"].append(wall(white)[0])
        runs["correlated"].append(wall(corr)[0])
        runs["white_kernel"].append(kernel(white))
        runs["correlated_kernel"].append(kernel(corr))
    rec = {"bench": "correlated_cost", "lanes": lanes, "episodes_per_lane": episodes, "n_traffic": N, "policies": K, "group": group,
           "dtype": "float32", "reps": reps, "disturbance": corr.to_dict(), "sum_steps_white": [int(x) for x in a["sum_steps"]],
           "sum_steps_correlated": [int(x) for x in b["sum_steps"]], "device": torch.cuda.get_device_name(0),
           "method": "one warm-up, variants alternating, median of reps; white / correlated: wall clock between synchronisations, "
                     "*_kernel: HIP events around the C call; seconds"}
    for name, r in runs.items():
        rec[name + "_s"] = float(np.median(r))
        rec[name + "_runs_s"] = r
        rec[name + "_spread"] = spread(r)
        print("  %-18s median %.4f s   min %.4f   max %.4f" % (name, np.median(r), min(r), max(r)), flush=True)
    rec["correlated_over_white"] = rec["correlated_s"] / rec["white_s"]
    rec["correlated_kernel_over_white_kernel"] = rec["correlated_kernel_s"] / rec["white_kernel_s"]
    rec["apart_beyond_spreads"] = bool(min(runs["correlated_kernel"]) > max(runs["white_kernel"]) or
                                       max(runs["correlated_kernel"]) < min(runs["white_kernel"]))
    rec["per_step_ratio"] = rec["correlated_kernel_over_white_kernel"] * sum(rec["sum_steps_white"]) / sum(rec["sum_steps_correlated"])
    return rec


def curve(lanes, episodes):
    ref = g.load_sb3_policy(os.path.join(ROOT, "tests", "golden", "ref_policy_best_model.npz"))
    D = g.ACAS2DConfig().obs_dim
    zero = (torch.zeros(64, D), torch.zeros(64), torch.zeros(64, 64), torch.zeros(64), torch.zeros(1, 64), torch.zeros(1))
    levels = [g.CorrelatedDisturbance.normalised(sep=s, cpa=s, closing=s, seed=7, rho=rho) for s in (0.04, 0.08) for rho in (0.0, 0.9, 0.99, 1.0)] + \
             [g.CorrelatedDisturbance.normalised(action=a, seed=7, rho=rho) for a in (0.2, 0.4) for rho in (0.0, 0.9, 0.99, 1.0)]
    out = []
    for level in levels:
        mc = g.MonteCarlo([ref, zero], lanes, n_traffic=1, n_bins=N_BINS, device=DEV, disturbance=level)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s = mc.run(episodes, per_launch=episodes).summary(baseline=1)
        wall = time.perf_counter() - t0
        rec = {"bench": "correlated_curve", "policy": "tests/golden/ref_policy_best_model.npz", "baseline": "zero", "lanes": lanes,
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
    assert torch.cuda.is_available(), "bench_correlated.py measures on the GPU"
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
