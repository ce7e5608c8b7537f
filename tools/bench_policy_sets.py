#!/usr/bin/env python3
"""Wall time of scoring K policies on the reference's 100 test episodes: ONE evaluate_policies_fused launch against K
evaluate_policy_fused calls (one rollout-policy launch each, with per-step outputs).  Timed with HIP events around
the launches only (env setup and the host copies of the results excluded; rollout_policy() stages its weights per call), after a warm-up, median of
--reps runs.  One JSON line.

    python tools/bench_policy_sets.py [--policies 32] [--reps 7] [--dtype float64]

--safety times the evaluation with per-episode safety statistics (acas2d_evaluate_policies_stats_*) instead, one JSON
line per shape: 100 test episodes x K = 1 and 8 policies at one traffic aircraft, 4 096 episodes at 8 (thread per env)
and at 64 (group) aircraft, float32.  Three arms on the same episodes, their repetitions interleaved in one process (the
order rotates from round to round), median / min / max per arm:
  plain   the plain entry point -- the parent's kernel, unchanged
  stats   the new entry point
  replay  the only other way to these numbers: rollout_policy() (per-step outputs, all n_steps for every env) for each
          policy, then its actions replayed through the latching per-step kernel with record_trace=True until the last
          episode is done, the three trace columns copied aside after every step.  The host reduction
          (records.episode_safety) is NOT in the time.
plain and stats are `--inner` launches per timed window.

    python tools/bench_policy_sets.py --safety [--reps 9] [--inner 10]
"""
import argparse
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
ap.add_argument("--safety", action="store_true", help="time acas2d_evaluate_policies_stats_* (see the docstring)")
ap.add_argument("--inner", type=int, default=10, help="--safety: launches per timed window of the plain and stats arms")
args = ap.parse_args()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def safety_shape(N, E, K, group, reps, inner):
    """One JSON-able row: the three arms of --safety at N aircraft, E episodes, K policies (float32)."""
    dev, f32 = "cuda:0", torch.float32
    cfg = g.ACAS2DConfig(n_traffic=N)
    D, T = cfg.obs_dim, cfg.max_steps + 1
    own, trf, goal = g.reset_parity.draw_episodes(cfg, E, random.Random(13))
    pols = []
    for i in range(K):
        torch.manual_seed(100 + i)
        p = g.ActorCritic(D)
        with torch.no_grad():
            p.action_net.weight.mul_(40.0)
        pols.append(p)
    blocks = g.policy.PolicyBlocks(pols, E, D, dev)
    idx = blocks.index()
    venv = g.ACAS2DVecEnv(len(idx), N, device=dev, dtype=f32, auto_reset=True, config=cfg)
    venv.set_state(own[idx], trf[idx], goal[idx], np.zeros(len(idx), np.int32), observe=True)
    res = (torch.empty(K, E, dtype=torch.uint8, device=dev), torch.empty(K, E, dtype=torch.int32, device=dev),
           torch.empty(K, E, dtype=f32, device=dev))
    st_f, st_i = torch.empty(4, K, E, dtype=f32, device=dev), torch.empty(2, K, E, dtype=torch.int32, device=dev)
    cstats = blocks.c_eval_stats(st_f, st_i)
    plain_fn = g.policy.evaluate_policies_entry(f32, group, False)
    stats_fn = g.policy.evaluate_policies_entry(f32, group, True)

    def launch(fn, *extra):
        for _ in range(inner):
            blocks.call(fn, venv, venv.outputs["obs"], T, *[r.data_ptr() for r in res], *extra)

    # the replay arm: one rollout env and one latching env with traces, reused by every policy
    roll = g.ACAS2DVecEnv(E, N, device=dev, dtype=f32, auto_reset=True, config=cfg)
    lat = g.ACAS2DVecEnv(E, N, device=dev, dtype=f32, auto_reset=False, record_trace=True, config=cfg)
    zero = np.zeros(E, np.int32)
    names = list(g.vec_env.TRACE_COLUMNS)
    cols = torch.tensor([names.index(c) for c in ("d_sep", "a_lat", "d_dev")], device=dev)
    rows = torch.empty(T + 1, E, 3, dtype=f32, device=dev)
    state = {"out": None, "last": [T - 1] * K}

    def replay(measure_last=False):
        for k, p in enumerate(pols):
            roll.set_state(own, trf, goal, zero, observe=True)
            state["out"] = out = roll.rollout_policy(p, T, out=state["out"], group=group)
            if measure_last:                                    # (outside the timed runs: it synchronises)
                done = out["done"]
                state["last"][k] = int(torch.where(done.any(0), done.int().argmax(0), T - 1).max())
            lat.set_state(own, trf, goal, zero, observe=True)
            rows[0] = lat.trace[:, cols]
            for t in range(state["last"][k] + 1):
                lat.step(out["actions"][t])
                rows[t + 1] = lat.trace[:, cols]

    arms = {"plain": lambda: launch(plain_fn), "stats": lambda: launch(stats_fn, cstats), "replay": replay}
    launch(plain_fn)
    launch(stats_fn, cstats)
    replay(measure_last=True)
    torch.cuda.synchronize()
    order, t = list(arms), {a: [] for a in arms}
    for r in range(reps):
        for a in order[r % 3:] + order[:r % 3]:
            t[a].append(timed(arms[a]) / (1 if a == "replay" else inner))
    # the two evaluations agree, and the statistics are there
    launch(plain_fn)
    torch.cuda.synchronize()
    base = [r.clone() for r in res]
    launch(stats_fn, cstats)
    torch.cuda.synchronize()
    same = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(base, res))
    steps = res[1].cpu().numpy()
    med = {a: float(np.median(v)) for a, v in t.items()}
    row = {"bench": "eval_stats", "n_traffic": N, "episodes": E, "policies": K, "entry": stats_fn, "dtype": "float32",
           "steps_budget": T, "reps": reps, "launches_per_window": inner,
           "method": "HIP events, warm-up first, arms interleaved in one process with rotating order; ms per launch "
                     "(replay: per K-policy pass, host reduction excluded)",
           "env_steps_played": int(np.maximum(steps - 1, 0).sum()), "replay_steps": [x + 1 for x in state["last"]],
           "unfinished": int((res[0] == 0).sum()), "outputs_equal_plain_entry": bool(same),
           "mean_min_separation": float(st_f[0].mean()), "episodes_with_los": int((st_i[1] > 0).sum())}
    for a, v in t.items():
        row.update({a + "_ms": med[a], a + "_min_ms": float(min(v)), a + "_max_ms": float(max(v))})
    row["stats_over_plain"] = med["stats"] / med["plain"]
    row["stats_over_plain_per_round"] = float(np.median(np.array(t["stats"]) / np.array(t["plain"])))
    row["replay_over_stats"] = med["replay"] / med["stats"]
    return row


if args.safety:
    for N, E, K, group in ((1, 100, 1, False), (1, 100, 8, False), (8, 4096, 1, False), (64, 4096, 1, True)):
        print(json.dumps(safety_shape(N, E, K, group, args.reps, args.inner)), flush=True)
    sys.exit(0)

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
blocks = g.policy.PolicyBlocks(pols, E, 8, "cuda:0")
idx = blocks.index()
venv = g.ACAS2DVecEnv(len(idx), 1, device="cuda:0", dtype=dt, auto_reset=True)
venv.set_state(own[idx], trf[idx], goal[idx], np.zeros(len(idx), np.int32), observe=True)
res = (torch.empty(K, E, dtype=torch.uint8, device="cuda:0"), torch.empty(K, E, dtype=torch.int32, device="cuda:0"),
       torch.empty(K, E, dtype=dt, device="cuda:0"))
entry = g.policy.evaluate_policies_entry(dt)


def run_set():
    blocks.call(entry, venv, venv.outputs["obs"], T, *[r.data_ptr() for r in res])


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
