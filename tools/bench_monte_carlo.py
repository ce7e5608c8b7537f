#!/usr/bin/env python3
"""A Monte Carlo campaign's launches (policy.MonteCarlo: acas2d_monte_carlo_*) beside the only way to the same numbers
without them, one JSON line per case.  A case is LANESxEPISODESxN_TRAFFICxK (default 65536x8x1x1, 65536x8x1x8, 65536x8x8x1,
65536x8x8x8), float32, K randomly initialised policies, the campaign's first EPISODES counters:

  (a) campaign   MonteCarlo.run(EPISODES): the draw of the first episode, its replication and the launch(es), wall clock
                 between device synchronisations
  (b) rounds     per counter: reset() / reset_masked(all) on a LANES-env engine, the state read back,
                 evaluate_policies_fused(safety=True), records.monte_carlo_reduce() of its nine [K, LANES] arrays -- wall
                 clock likewise
  (c) kernels    the kernel time alone of (b)'s EPISODES stats-evaluator launches: HIP events around each
                 acas2d_evaluate_policies_stats_* call on a state staged beforehand, summed
  (d) kernel     the kernel time alone of (a)'s launch(es), HIP events likewise

One warm-up of every variant, then --reps repetitions, the variants alternating in one process; the median and min - max
are printed, `spread` is (max - min) / median.  The accumulators of (a) are compared with (b)'s before anything is timed.
usage: bench_monte_carlo.py [--cases ...] [--reps 5] [--out profiles/monte_carlo_timing.jsonl]"""
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


class StatsLaunch:
    """evaluate_policies_fused(safety=True)'s launch on a state staged beforehand, so that HIP events see the kernel alone."""

    def __init__(self, pols, lanes, N, group):
        K = len(pols)
        self.blocks = g.policy.PolicyBlocks(pols, lanes, 5 + 3 * N, DEV)
        self.idx = self.blocks.index()
        self.v = g.ACAS2DVecEnv(len(self.idx), N, device=DEV, dtype=torch.float32, auto_reset=True)
        self.entry = g.policy.evaluate_policies_entry(torch.float32, group, True)
        new = lambda dt: torch.empty(K, lanes, dtype=dt, device=DEV)  # noqa: E731
        self.out = [new(torch.uint8), new(torch.int32), new(torch.float32)]
        self.st_f, self.st_i = torch.empty(4, K, lanes, device=DEV), torch.empty(2, K, lanes, dtype=torch.int32, device=DEV)

    def stage(self, own, trf, goal):
        self.v.set_state(own[self.idx], trf[self.idx], goal[self.idx], np.zeros(len(self.idx), np.int32), observe=True)

    def launch(self):
        self.blocks.call(self.entry, self.v, self.v.outputs["obs"], self.v.config.max_steps + 1,
                         *[t.data_ptr() for t in self.out], self.blocks.c_eval_stats(self.st_f, self.st_i))


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3


def case(lanes, episodes, N, K, reps):
    group = False                                              # (1 and 8 aircraft: thread per env)
    pols = policies(N, K)
    cfg = g.ACAS2DConfig(n_traffic=N)
    inv = N_BINS / (4.0 * cfg.safe_distance)
    src = g.ACAS2DVecEnv(lanes, N, device=DEV, dtype=torch.float32, seed=13)
    every = torch.ones(lanes, dtype=torch.uint8, device=DEV)
    stats = StatsLaunch(pols, lanes, N, group)

    def campaign():
        mc = g.MonteCarlo(pols, lanes, n_traffic=N, n_bins=N_BINS, device=DEV)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mc.run(episodes, per_launch=episodes)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, mc

    def campaign_kernel():
        mc = g.MonteCarlo(pols, lanes, n_traffic=N, n_bins=N_BINS, device=DEV)
        ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        mc._launch(episodes, events=ev)
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e-3

    def rounds():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        acc = None
        for c in range(episodes):
            src.reset() if c == 0 else src.reset_masked(every)
            own, trf, goal = g.policy.read_state(src)
            res = g.evaluate_policies_fused(pols, own, trf, goal, dtype=torch.float32, device=DEV, group=group, safety=True)
            acc = g.records.monte_carlo_reduce([res], N_BINS, inv, np.float32, acc=acc, first_episode=c)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, acc

    def kernels():
        total = 0.0
        for c in range(episodes):
            src.reset_to_episode(c)
            stats.stage(*g.policy.read_state(src))
            torch.cuda.synchronize()
            total += events(stats.launch)
        return total

    _, mc = campaign()                                         # warm-up, and the agreement
    _, ref = rounds()
    got = mc.accumulators()
    agree = all(np.array_equal(got[k].view(np.uint8), np.ascontiguousarray(ref[k]).view(np.uint8)) for k in g.records.MONTE_CARLO_KEYS)
    kernels()
    campaign_kernel()
    runs = {"campaign": [], "rounds": [], "kernels": [], "campaign_kernel": []}
    for _ in range(reps):
        runs["campaign"].append(campaign()[0])
        runs["rounds"].append(rounds()[0])
        runs["kernels"].append(kernels())
        runs["campaign_kernel"].append(campaign_kernel())
    s = mc.summary()
    rec = {"bench": "monte_carlo", "lanes": lanes, "episodes_per_lane": episodes, "n_traffic": N, "policies": K, "dtype": "float32",
           "reps": reps, "bit_equal_to_rounds": bool(agree), "episodes": int(s["episodes"][0]),
           "collision_rate": [float(x) for x in s["collision_rate"]], "mean_steps": [float(x) for x in s["mean_steps"]],
           "device": torch.cuda.get_device_name(0),
           "method": "one warm-up, variants alternating, median of reps; campaign / rounds: wall clock between synchronisations, "
                     "kernels / campaign_kernel: HIP events around the C calls; seconds"}
    for name, r in runs.items():
        rec[name + "_s"] = float(np.median(r))
        rec[name + "_runs_s"] = r
        rec[name + "_spread"] = spread(r)
        print("  %-16s median %.4f s   min %.4f   max %.4f" % (name, np.median(r), min(r), max(r)), flush=True)
    rec["campaign_over_rounds"] = rec["campaign_s"] / rec["rounds_s"]
    rec["campaign_over_kernels"] = rec["campaign_s"] / rec["kernels_s"]
    rec["campaign_kernel_over_kernels"] = rec["campaign_kernel_s"] / rec["kernels_s"]
    rec["campaign_above_kernels_beyond_spreads"] = bool(min(runs["campaign"]) > max(runs["kernels"]))
    return rec


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="65536x8x1x1,65536x8x1x8,65536x8x8x1,65536x8x8x8")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_monte_carlo.py measures on the GPU"
    sink = open(args.out, "a") if args.out else None
    for c in args.cases.split(","):
        lanes, episodes, N, K = (int(x) for x in c.split("x"))
        print("case %s" % c, flush=True)
        line = json.dumps(case(lanes, episodes, N, K, args.reps))
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
