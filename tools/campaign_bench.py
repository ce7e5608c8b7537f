"""What tools/bench_disturbance.py and tools/bench_correlated.py share: the policies, the timing of alternating campaign
variants, the collision-rate curve over disturbance levels and the command line.  A module, not a script: each bench keeps
its variants, its levels and the record fields only it computes."""
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


def time_variants(make, variants, episodes, reps):
    """`variants`: {name: disturbance}, make(disturbance): a fresh campaign.  One warm-up of every variant, wall clock and
    kernel; then `reps` repetitions, the variants alternating: wall clock between device synchronisations under `name`, the
    kernel alone between HIP events under `name_kernel`.  Returns (the warm-up campaigns' accumulators by name, the runs by
    name, their *_s / *_runs_s / *_spread summary, printed as it is made)."""
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

    acc = {name: wall(dist)[1].accumulators() for name, dist in variants.items()}
    for dist in variants.values():
        kernel(dist)
    runs = {name + tail: [] for tail in ("", "_kernel") for name in variants}
    for _ in range(reps):
        for name, dist in variants.items():
            runs[name].append(wall(dist)[0])
        for name, dist in variants.items():
            runs[name + "_kernel"].append(kernel(dist))
    summary = {}
    width = max(len(name) for name in runs) + 1
    for name, r in runs.items():
        summary[name + "_s"] = float(np.median(r))
        summary[name + "_runs_s"] = r
        summary[name + "_spread"] = spread(r)
        print("  %-*s median %.4f s   min %.4f   max %.4f" % (width, name, np.median(r), min(r), max(r)), flush=True)
    return acc, runs, summary


def curve(levels, lanes, episodes, bench_name):
    """One campaign per disturbance of `levels`, the same encounters at every level: the committed reference policy and the
    all-zero policy at one aircraft, one record each."""
    ref = g.load_sb3_policy(os.path.join(ROOT, "tests", "golden", "ref_policy_best_model.npz"))
    D = g.ACAS2DConfig().obs_dim
    zero = (torch.zeros(64, D), torch.zeros(64), torch.zeros(64, 64), torch.zeros(64), torch.zeros(1, 64), torch.zeros(1))
    out = []
    for level in levels:
        mc = g.MonteCarlo([ref, zero], lanes, n_traffic=1, n_bins=N_BINS, device=DEV, disturbance=level)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s = mc.run(episodes, per_launch=episodes).summary(baseline=1)
        wall = time.perf_counter() - t0
        rec = {"bench": bench_name, "policy": "tests/golden/ref_policy_best_model.npz", "baseline": "zero", "lanes": lanes,
               "episodes_per_lane": episodes, "disturbance": level.to_dict(), "seconds": wall, "device": torch.cuda.get_device_name(0)}
        for key in ("episodes", "collisions", "collision_rate", "collision_rate_lo", "collision_rate_hi", "los_rate", "goal_rate",
                    "timeout_rate", "risk_ratio", "mean_steps"):
            rec[key] = [int(x) if s[key].dtype.kind == "i" else float(x) for x in s[key]]
        rec["closest"] = [float(w[0][2]) for w in mc.worst(1)]
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return out


def main(tool, cost, curve_of):
    """The command line of `tool`: cost(lanes, episodes, N, K, group, reps) per case, then curve_of(lanes, episodes)."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="65536x8x1x1,65536x8x1x8,65536x8x8x1,65536x8x8x8,65536x8x16x1g")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--curve", metavar="LANESxEPISODES", default="65536x8")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "%s measures on the GPU" % tool
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
        for rec in curve_of(lanes, episodes):
            emit(rec)
