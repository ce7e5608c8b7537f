#!/usr/bin/env python3
"""What collecting under time-correlated errors costs over the white disturbed collector, one JSON line per record
(ACAS2DVecEnv.collect / collect_set with a policy.CorrelatedDisturbanceSet: acas2d_collect_set_correlated_*).

collect  per case ENVSxSTEPSxN_TRAFFICxK[g] (ENVS per member; g: the group-cooperative launch), float32, K randomly
         initialised actor-critics, two variants of ONE collection launch from the same env state:
           (a) white   the disturbed collector under sensor sigma 0.04 (normalised units) and action sigma 0.2
           (b) corr    the correlated collector under the same sigmas and seed with every rho 0.5: the same draws, two
                       products and a sum per channel through the wave's LDS, and one load and one store of 3 N + 1 floats
                       per env and launch
         They play different steps (the errors differ), on the same number of envs and steps.  The env state is put back and the
         held state zeroed before every launch; HIP events around the launch (the copies of the first and the last observation
         included, as in the trainers); one warm-up of every variant, then --reps repetitions, the variants alternating in one
         process; median and min - max, `spread` is (max - min) / median.
learn    PPOTrainer(collector="fused", updater="fused", gae="kernel").learn() steps per second at ENVSxSTEPSxN_TRAFFIC under
         (a) and under (b), each trainer warmed up by one iteration, then --reps windows of --iters iterations, alternating.

usage: bench_collect_correlated.py [--cases ...] [--learn 1024x512x1] [--reps 5] [--out profiles/collect_correlated_timing.jsonl]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gym_acas2d_amd as g  # noqa: E402
from bench_collect_disturbed import DEV, summarise  # noqa: E402

SIGMAS = dict(sep=0.04, cpa=0.04, closing=0.04, action=0.2, seed=7)
RHO = 0.5


def levels(K):
    """The two variants' `disturbance=` arguments for K members."""
    return {"white": g.DisturbanceSet(g.Disturbance.normalised(**SIGMAS), K),
            "corr": g.CorrelatedDisturbanceSet(g.CorrelatedDisturbance.normalised(**SIGMAS, rho=RHO), K)}


def collect_case(envs, steps, N, K, group, reps):
    venv = g.ACAS2DVecEnv(K * envs, N, device=DEV, dtype=torch.float32, seed=13)
    venv.reset()
    members = []
    for k in range(K):
        torch.manual_seed(k + 1)
        members.append(g.ActorCritic(5 + 3 * N))
    pset = g.ActorCriticSet.from_members(members, device=DEV)
    seeds = list(range(21, 21 + K))
    lv = levels(K)
    state, obs0 = venv.state_dict(), venv.outputs["obs"].clone()
    outs = {name: None for name in lv}

    def launch(name):
        venv.load_state_dict(state)
        venv.outputs["obs"].copy_(obs0)
        d = lv[name]
        if name == "corr":
            d.reset_held()
        ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        ev[0].record()
        if K == 1:
            outs[name] = venv.collect(members[0], steps, noise_seed=seeds[0], out=outs[name], group=group, disturbance=d)
        else:
            outs[name] = venv.collect_set(pset, steps, seeds, out=outs[name], group=group, disturbances=d)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e-3

    for name in lv:                                           # warm-up
        launch(name)
    # the first step of an episode reads z itself under both; the launch as a whole does not
    first_rows_equal = bool(torch.equal(outs["corr"]["obs_read"][0], outs["white"]["obs_read"][0]))
    rows_differ = not torch.equal(outs["corr"]["obs_read"], outs["white"]["obs_read"])
    runs = {name: [] for name in lv}
    for _ in range(reps):
        for name in lv:
            runs[name].append(launch(name))
    rec = {"bench": "collect_correlated", "envs_per_member": envs, "steps": steps, "n_traffic": N, "members": K, "group": group,
           "dtype": "float32", "reps": reps, "sigmas": SIGMAS, "rho": RHO, "first_rows_equal": first_rows_equal,
           "rows_differ": rows_differ, "held_bytes": int(lv["corr"].held.numel() * 4), "device": torch.cuda.get_device_name(0),
           "method": "one warm-up, variants alternating, median of reps; HIP events around one collection call (the launch and "
                     "the two observation-row copies), the env state put back and the held state zeroed before each; seconds"}
    summarise(rec, runs)
    rec["corr_over_white"] = rec["corr_s"] / rec["white_s"]
    rec["apart_beyond_spreads"] = bool(min(runs["corr"]) > max(runs["white"]) or max(runs["corr"]) < min(runs["white"]))
    return rec


def learn_case(envs, steps, N, reps, iters):
    trainers = {}
    for name, d in levels(1).items():
        venv = g.ACAS2DVecEnv(envs, N, device=DEV, dtype=torch.float32, seed=13)
        tr = g.PPOTrainer(venv, g.PPOConfig(n_steps=steps, batch_size=4096, seed=13), collector="fused", updater="fused",
                          gae="kernel", disturbance=d)
        tr.learn(envs * steps, log=None)                      # warm-up: one iteration (captures, the update's buffers)
        trainers[name] = tr
    runs = {name: [] for name in trainers}
    for _ in range(reps):
        for name, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.learn(tr.num_timesteps + iters * envs * steps, log=None)
            torch.cuda.synchronize()
            runs[name].append(iters * envs * steps / (time.perf_counter() - t0))
    rec = {"bench": "learn_correlated", "envs": envs, "steps": steps, "n_traffic": N, "iterations_per_window": iters, "reps": reps,
           "sigmas": SIGMAS, "rho": RHO, "collector": "fused", "updater": "fused", "gae": "kernel",
           "device": torch.cuda.get_device_name(0),
           "method": "one warm-up iteration per trainer, windows alternating, median of reps; env steps per second of wall clock"}
    summarise(rec, runs, unit="steps_per_s")
    rec["corr_over_white"] = rec["corr_steps_per_s"] / rec["white_steps_per_s"]
    return rec


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1024x512x1x1,1024x512x8x1,1024x128x16x1g,1024x512x1x4")
    ap.add_argument("--learn", metavar="ENVSxSTEPSxN_TRAFFIC", default="1024x512x1")
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_collect_correlated.py measures on the GPU"
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        print(json.dumps(rec), flush=True)
        if sink:
            sink.write(json.dumps(rec) + "\n")
            sink.flush()

    for c in [c for c in args.cases.split(",") if c]:
        group = c.endswith("g")
        envs, steps, N, K = (int(x) for x in c.rstrip("g").split("x"))
        print("case %s" % c, flush=True)
        emit(collect_case(envs, steps, N, K, group, args.reps))
    if args.learn and args.learn != "none":
        envs, steps, N = (int(x) for x in args.learn.lower().split("x"))
        print("learn %s" % args.learn, flush=True)
        emit(learn_case(envs, steps, N, args.reps, args.iters))
