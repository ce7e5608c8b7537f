#!/usr/bin/env python3
"""What collecting under a disturbance costs, one JSON line per record (ACAS2DVecEnv.collect(disturbance=) /
collect_set(disturbances=): acas2d_collect_set_disturbed_*).

collect  per case ENVSxSTEPSxN_TRAFFICxK[g] (ENVS per member; g: the group-cooperative launch), float32, K randomly
         initialised actor-critics, three variants of ONE collection launch on the same env state:
           (a) plain      collect() / collect_set() without a disturbance: the undisturbed kernel
           (b) zero       the disturbed kernel with all sigmas 0: nothing is drawn, obs_read is still written -- (b) - (a) is
                          the extra row store (it roughly doubles the collector's observation writes)
           (c) tiny       the disturbed kernel with all sigmas 1e-30: every block is drawn and every add executed, yet no
                          float32 value moves, so all three play the same steps -- (c) - (b) is the draws
         Before anything is timed (b)'s and (c)'s outputs are compared with (a)'s and the outcome recorded.  The env state is
         put back before every launch; HIP events around the launch (the copies of the first and the last observation
         included, as in the trainers); one warm-up of every variant, then --reps repetitions, the variants alternating
         in one process; median and min - max, `spread` is (max - min) / median.
learn    PPOTrainer(collector="fused", updater="fused", gae="kernel").learn() steps per second at ENVSxSTEPSxN_TRAFFIC, without
         a disturbance and with the tiny one, each trainer warmed up by one iteration, then --reps windows of --iters
         iterations, alternating.

usage: bench_collect_disturbed.py [--cases ...] [--learn 1024x512x1] [--reps 5] [--out profiles/collect_disturbed_timing.jsonl]"""
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
TINY = 1e-30
OUTPUTS = ("obs", "actions", "values", "logp", "reward", "done_u8", "outcome", "episode_return", "episode_steps")


def spread(runs):
    return (max(runs) - min(runs)) / float(np.median(runs))


def summarise(rec, runs, unit="s"):
    for name, r in runs.items():
        rec["%s_%s" % (name, unit)] = float(np.median(r))
        rec["%s_runs_%s" % (name, unit)] = r
        rec[name + "_spread"] = spread(r)
        print("  %-6s median %.6g   min %.6g   max %.6g" % (name, np.median(r), min(r), max(r)), flush=True)


def collect_case(envs, steps, N, K, group, reps):
    venv = g.ACAS2DVecEnv(K * envs, N, device=DEV, dtype=torch.float32, seed=13)
    venv.reset()
    members = []
    for k in range(K):
        torch.manual_seed(k + 1)
        members.append(g.ActorCritic(5 + 3 * N))
    pset = g.ActorCriticSet.from_members(members, device=DEV)
    seeds = list(range(21, 21 + K))
    levels = {"plain": None, "zero": g.Disturbance(seed=7),
              "tiny": g.Disturbance.normalised(sep=TINY, cpa=TINY, closing=TINY, action=TINY, seed=7)}
    assert min(levels["tiny"].sigma + (levels["tiny"].s_action,)) > 0.0
    state, obs0 = venv.state_dict(), venv.outputs["obs"].clone()
    outs = {name: None for name in levels}

    def launch(name):
        venv.load_state_dict(state)
        venv.outputs["obs"].copy_(obs0)
        d = levels[name]
        ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        ev[0].record()
        if K == 1:
            outs[name] = venv.collect(members[0], steps, noise_seed=seeds[0], out=outs[name], group=group,
                                      **({} if d is None else {"disturbance": d}))
        else:
            outs[name] = venv.collect_set(pset, steps, seeds, out=outs[name], group=group,
                                          **({} if d is None else {"disturbances": d}))
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e-3

    for name in levels:                                       # warm-up, and the agreement
        launch(name)
    equal = {name: all(torch.equal(outs[name][k], outs["plain"][k]) for k in OUTPUTS) for name in ("zero", "tiny")}
    read_is_true = {name: bool(torch.equal(outs[name]["obs_read"], outs[name]["obs"])) for name in ("zero", "tiny")}
    runs = {name: [] for name in levels}
    for _ in range(reps):
        for name in levels:
            runs[name].append(launch(name))
    rec = {"bench": "collect_disturbed", "envs_per_member": envs, "steps": steps, "n_traffic": N, "members": K, "group": group,
           "dtype": "float32", "reps": reps, "sigma": TINY, "outputs_equal_plain": equal, "obs_read_equals_obs": read_is_true,
           "device": torch.cuda.get_device_name(0),
           "method": "one warm-up, variants alternating, median of reps; HIP events around one collection call (the launch and "
                     "the two observation-row copies), the env state put back before each; seconds"}
    summarise(rec, runs)
    rec["zero_over_plain"] = rec["zero_s"] / rec["plain_s"]
    rec["tiny_over_plain"] = rec["tiny_s"] / rec["plain_s"]
    rec["tiny_over_zero"] = rec["tiny_s"] / rec["zero_s"]
    rec["store_share_of_difference"] = ((rec["zero_s"] - rec["plain_s"]) / (rec["tiny_s"] - rec["plain_s"])
                                        if rec["tiny_s"] != rec["plain_s"] else None)
    rec["apart_beyond_spreads"] = bool(min(runs["tiny"]) > max(runs["plain"]))
    return rec


def learn_case(envs, steps, N, reps, iters):
    tiny = g.Disturbance.normalised(sep=TINY, cpa=TINY, closing=TINY, action=TINY, seed=7)
    trainers = {}
    for name, d in (("plain", None), ("tiny", tiny)):
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
    rec = {"bench": "learn_disturbed", "envs": envs, "steps": steps, "n_traffic": N, "iterations_per_window": iters, "reps": reps,
           "sigma": TINY, "collector": "fused", "updater": "fused", "gae": "kernel", "device": torch.cuda.get_device_name(0),
           "method": "one warm-up iteration per trainer, windows alternating, median of reps; env steps per second of wall clock"}
    summarise(rec, runs, unit="steps_per_s")
    rec["tiny_over_plain"] = rec["tiny_steps_per_s"] / rec["plain_steps_per_s"]
    return rec


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1024x512x1x1,1024x512x8x1,1024x128x16x1g,1024x512x1x4")
    ap.add_argument("--learn", metavar="ENVSxSTEPSxN_TRAFFIC", default="1024x512x1")
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_collect_disturbed.py measures on the GPU"
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
