#!/usr/bin/env python3
"""Seed robustness of the large-batch PPO defaults (tools/train_ppo.py: 1 024 envs x 256 steps, fused collector +
fused update): for each named hyper-parameter set and each seed, train for --timesteps and evaluate deterministically
on the reference's 100 test episodes (testing_main.py; the reference's own policy scores 100 / 100 goals, mean return
1210.07).  One JSON line per run, one summary line per set.

    python tools/ppo_seed_sweep.py --sets default lr1e-4 --seeds 13 14 15 --timesteps 3e7

--population trains the seeds of a set as ONE population (ppo.PopulationTrainer: member k on its own --envs envs of one
env of len(seeds) x --envs; at --traffic 16, 32, 64 with group=True: the group-cooperative collector and the wide update)
and scores them in one launch.  Opt-in: the sequential path is the default (DESIGN.md 4.2e
says what was measured).  Member k plays the envs at offset k x --envs, so its episodes are not the solo run's: the
runs compare as seeds do, not bit for bit.
--pbt (with --population) makes the population a ppo.PBTTrainer: every --pbt-every iterations the --pbt-fraction worst
members by training return copy one of the best and perturb its learning rate, clip range and entropy coefficient
(DESIGN.md 4.2g).  Opt-in; the members are then no longer independent seeds.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gym_acas2d_amd as g  # noqa: E402
import helpers as H  # noqa: E402

SETS = {
    "default": dict(),                                              # train_ppo.py: n_steps 256, batch 4096, lr 3e-4
    "lr1e-4": dict(learning_rate=1e-4),
    "lr1.5e-4": dict(learning_rate=1.5e-4),
    "batch16k": dict(batch_size=16384),
    "batch1k": dict(batch_size=1024),
    "steps512": dict(n_steps=512),
    "steps1024": dict(n_steps=1024, batch_size=8192),
    "ent1e-3": dict(ent_coef=1e-3),
    "epochs5": dict(n_epochs=5),
    "clip0.1": dict(clip_range=0.1),
    "lr1e-4_steps512": dict(learning_rate=1e-4, n_steps=512),
    "gamma0.995": dict(gamma=0.995),
}
ap = argparse.ArgumentParser()
ap.add_argument("--sets", nargs="+", default=["default"])
ap.add_argument("--seeds", type=int, nargs="+", default=[13, 14, 15])
ap.add_argument("--envs", type=int, default=1024)
ap.add_argument("--traffic", type=int, default=1, help="traffic aircraft (the 100 scored episodes are then drawn for that count)")
ap.add_argument("--timesteps", type=float, default=3.0e7)
ap.add_argument("--out", default=None)
ap.add_argument("--population", action="store_true", help="one PopulationTrainer per set over the seeds")
ap.add_argument("--pbt", action="store_true", help="with --population: exploit / explore between the members (ppo.PBTTrainer)")
ap.add_argument("--pbt-every", type=int, default=8, help="iterations between two exploit steps")
ap.add_argument("--pbt-fraction", type=float, default=0.25, help="the share of members replaced at an exploit step")
ap.add_argument("--gae", choices=("torch", "kernel"), default=None,
                help="kernel: GAE as one hand-written launch (ppo.gae_fused), the same bits as torch's compute_gae; the default "
                     "follows tools/bench_gae.py's measurement (DESIGN.md 4.2f): GAE_DEFAULT below")
ap.add_argument("--target-kl", type=float, default=None,
                help="SB3's target_kl for every run of the sweep (decided inside the fused update's launches, DESIGN.md 4.2h): "
                     "the records then carry the last update's approx_kl, clip_fraction and n_applied")
ap.add_argument("--clip-range-vf", type=float, default=None, metavar="X",
                help="SB3's clip_range_vf for every run of the sweep (inside the fused update's launches, DESIGN.md 4.2j)")
ap.add_argument("--lr-schedule", choices=("constant", "linear"), default="constant",
                help="linear: the learning rate falls linearly to 0 over --timesteps (a factor on the rate; with --pbt on "
                     "whatever rate the exploit steps have left a member)")
ap.add_argument("--clip-schedule", choices=("constant", "linear"), default="constant",
                help="linear: the clip range falls linearly to 0 over --timesteps, likewise")
ap.add_argument("--reward-norm", action="store_true",
                help="SB3's VecNormalize(norm_obs=False, norm_reward=True) for every run of the sweep: rewards divided by the "
                     "running standard deviation of the discounted return before GAE (ppo.RewardNormalizer, DESIGN.md 4.2k); "
                     "the scores stay raw returns")
args = ap.parse_args()
if args.pbt and not args.population:
    ap.error("--pbt needs --population")
REWARD_NORM = True if args.reward_norm else None
# the schedules as PPOConfig takes them (callables: kept out of `kw`, which goes into the records as JSON)
SCHEDULES = dict(learning_rate_schedule=g.ppo.linear_schedule() if args.lr_schedule == "linear" else None,
                 clip_range_schedule=g.ppo.linear_schedule() if args.clip_schedule == "linear" else None)
# "kernel" where learn() with it beat gae="torch" by more than both variants' spreads (the fused-collector
# PPOTrainer by 2 % at 512 steps and 13 % at 128, the population by 3 %); a trainer that were not faster would say "torch"
GAE_DEFAULT = {"population": "kernel", "solo": "kernel"}
if args.gae is None:
    args.gae = GAE_DEFAULT["population" if args.population else "solo"]
sink = open(args.out, "a") if args.out else None


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if sink:
        sink.write(line + "\n")
        sink.flush()


N = args.traffic
GROUP = N in g.ppo.GROUP_TRAFFIC                       # the group-cooperative launches, in every trainer and evaluation
own, trf, goal = H.parity_reset_states(g.ACAS2DConfig(n_traffic=N), 13, 0, 100)
score = dict(dtype=torch.float32, config=g.ACAS2DConfig(n_traffic=N), group=True) if GROUP else {}
for name in args.sets:
    kw = {**dict(n_steps=256, batch_size=4096), **SETS[name], **({} if args.target_kl is None else {"target_kl": args.target_kl}),
          **({} if args.clip_range_vf is None else {"clip_range_vf": args.clip_range_vf})}
    sched = {"lr_schedule": args.lr_schedule, "clip_schedule": args.clip_schedule,
             **({"reward_norm": True} if args.reward_norm else {})}
    goals = []
    if args.population:
        t0 = time.time()
        K = len(args.seeds)
        venv = g.ACAS2DVecEnv(K * args.envs, N, device="cuda:0", dtype=torch.float32, seed=13)
        cfgs = [g.PPOConfig(seed=seed, **kw, **SCHEDULES) for seed in args.seeds]
        if args.pbt:
            pop = g.PBTTrainer(venv, cfgs, g.PBTConfig(ready_every=args.pbt_every, fraction=args.pbt_fraction), gae=args.gae,
                               group=GROUP, reward_norm=REWARD_NORM)
        else:
            pop = g.PopulationTrainer(venv, cfgs, gae=args.gae, group=GROUP, reward_norm=REWARD_NORM)
        hist = pop.learn(int(args.timesteps), log=None)
        out = g.evaluate_policies_fused(pop.policy_set.actor_weights(), own, trf, goal, **score)
        wall = time.time() - t0
        for k, seed in enumerate(args.seeds):
            last = [r for r in hist if r["member"] == k and not r.get("eval") and "exploit" not in r][-1]
            rec = {"set": name, "config": kw, **sched, "seed": seed, "population": K, "member": k, "timesteps": int(args.timesteps),
                   "wall_s": wall, "train_ep_rew_mean_last": last.get("ep_rew_mean"), "std": last.get("std"),
                   **{n: last[n] for n in ("approx_kl", "clip_fraction", "n_applied") if n in last},
                   "eval_mean_return": float(out["total_reward"][k].mean()), "eval_mean_steps": float(out["steps"][k].mean()),
                   "goal": int((out["outcome"][k] == 1).sum()), "collision": int((out["outcome"][k] == 2).sum()),
                   "timeout": int((out["outcome"][k] == 3).sum())}
            if args.pbt:
                steps = [r for r in hist if r["member"] == k and "exploit" in r]
                rec.update(pbt={"every": args.pbt_every, "fraction": args.pbt_fraction, "hyper": steps[-1]["hyper"] if steps else None,
                                "copied_from": [r["exploit"] for r in steps if r["exploit"] is not None]})
            goals.append(rec["goal"])
            emit(rec)
        del pop, venv
    for seed in ([] if args.population else args.seeds):
        t0 = time.time()
        venv = g.ACAS2DVecEnv(args.envs, N, device="cuda:0", dtype=torch.float32, seed=13)
        tr = g.PPOTrainer(venv, g.PPOConfig(seed=seed, **kw, **SCHEDULES), collector="fused", updater="fused", gae=args.gae,
                          reward_norm=REWARD_NORM)
        hist = tr.learn(int(args.timesteps), log=None)
        out = g.evaluate_policy_fused(tr.policy, own, trf, goal, **score)
        rec = {"set": name, "config": kw, **sched, "seed": seed, "timesteps": int(args.timesteps), "wall_s": time.time() - t0,
               "train_ep_rew_mean_last": hist[-1].get("ep_rew_mean"), "std": hist[-1].get("std"),
               **{n: hist[-1][n] for n in ("approx_kl", "clip_fraction", "n_applied") if n in hist[-1]},
               "eval_mean_return": float(out["total_reward"].mean()), "eval_mean_steps": float(out["steps"].mean()),
               "goal": int((out["outcome"] == 1).sum()), "collision": int((out["outcome"] == 2).sum()),
               "timeout": int((out["outcome"] == 3).sum())}
        goals.append(rec["goal"])
        emit(rec)
        del tr, venv
    emit({"set": name, "summary": True, "goals": goals, "min_goals": int(np.min(goals)), "mean_goals": float(np.mean(goals))})
