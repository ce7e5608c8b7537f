#!/usr/bin/env python3
"""Wall time of scoring K policies on the reference's 100 test episodes: ONE evaluate_policies_fused launch against K
evaluate_policy_fused calls (one rollout-policy launch each, with per-step outputs).  Timed with HIP events around
the launches only (env setup and the host copies of the results excluded; rollout_policy() stages its weights per call), after a warm-up, median of
--reps runs.  One JSON line.

    python tools/bench_policy_sets.py [--policies 32] [--reps 7] [--dtype float64]
"""
import argparse
import ctypes as C
import json
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gym_acas2d_amd as g  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--policies", type=int, default=32)
ap.add_argument("--episodes", type=int, default=100)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--dtype", choices=("float64", "float32"), default="float64")
args = ap.parse_args()

dt = getattr(torch, args.dtype)
K, E = args.policies, args.episodes
own, trf, goal = g.reset_parity.draw_episodes(g.ACAS2DConfig(), E, random.Random(13))
pols = []
for i in range(K):
    torch.manual_seed(100 + i)
    p = g.ActorCritic(8)
    with torch.no_grad():
        p.action_net.weight.mul_(40.0)
    pols.append(p)
T = g.ACAS2DConfig().max_steps + 1


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


# K single-policy evaluations: evaluate_policy_fused's launch (rollout_policy, T steps, per-step outputs), K times
singles = []
for p in pols:
    v = g.ACAS2DVecEnv(E, 1, device="cuda:0", dtype=dt, auto_reset=True)
    singles.append(v)
for v in singles:
    v.set_state(own, trf, goal, np.zeros(E, np.int32), observe=True)
outs = [None] * K


def run_singles():
    # a rollout-policy launch runs all T steps for every env whatever its state, so repeats cost the same
    for i, (v, p) in enumerate(zip(singles, pols)):
        outs[i] = v.rollout_policy(p, T, out=outs[i])


# the set: one launch on K x EP envs
EP = (E + 63) // 64 * 64
idx = np.tile(np.concatenate([np.arange(E), np.zeros(EP - E, np.int64)]), K)
venv = g.ACAS2DVecEnv(K * EP, 1, device="cuda:0", dtype=dt, auto_reset=True)
venv.set_state(own[idx], trf[idx], goal[idx], np.zeros(K * EP, np.int32), observe=True)
w = [torch.stack([t for t in ws]).contiguous() for ws in zip(*[(p.actor_weights()[0].t(), p.actor_weights()[1],
                                                                p.actor_weights()[2].t(), p.actor_weights()[3],
                                                                p.actor_weights()[4].reshape(64),
                                                                p.actor_weights()[5].reshape(1)) for p in pols])]
w = [t.to("cuda:0") for t in w]
res = (torch.empty(K, E, dtype=torch.uint8, device="cuda:0"), torch.empty(K, E, dtype=torch.int32, device="cuda:0"),
       torch.empty(K, E, dtype=dt, device="cuda:0"))
L = g.native.lib()
fn = L.acas2d_evaluate_policies_f32 if dt == torch.float32 else L.acas2d_evaluate_policies_f64
pw = g.native.CPolicy(*[t.data_ptr() for t in w], 64, 0)


def run_set():
    g.native.check(fn(C.byref(venv._ccfg), C.byref(venv._cstate), K * EP, C.byref(pw), K, E, venv.outputs["obs"].data_ptr(),
                      T, venv.seed_value, venv.env_offset, 1, *[r.data_ptr() for r in res], venv._stream()))


def run_one_single():
    v, p = singles[0], pols[0]
    outs[0] = v.rollout_policy(p, T, out=outs[0])


for f in (run_singles, run_set, run_one_single):      # warm-up
    timed(f)
t_set = [timed(run_set) for _ in range(args.reps)]
t_singles = [timed(run_singles) for _ in range(args.reps)]
t_one = [timed(run_one_single) for _ in range(args.reps)]
api = g.evaluate_policies_fused(pols, own, trf, goal, dtype=dt)
check = [g.evaluate_policy_fused(p, own, trf, goal, dtype=dt) for p in pols[:4]]
same = all(np.array_equal(api["steps"][k], c["steps"]) and np.array_equal(api["total_reward"][k], c["total_reward"])
           for k, c in enumerate(check))
print(json.dumps({"policies": K, "episodes": E, "dtype": args.dtype, "steps_budget": T, "reps": args.reps,
                  "method": "HIP events around the launches, warm-up first, median of reps",
                  "set_one_launch_ms": float(np.median(t_set)), "set_runs_ms": t_set,
                  "single_policy_launch_ms": float(np.median(t_one)),
                  "k_single_policy_evaluations_ms": float(np.median(t_singles)), "k_single_runs_ms": t_singles,
                  "speedup": float(np.median(t_singles) / np.median(t_set)),
                  "set_vs_one_single_launch": float(np.median(t_set) / np.median(t_one)),
                  "rows_match_single_evaluations": bool(same)}))
