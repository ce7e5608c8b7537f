#!/usr/bin/env python3
"""The fused PPO minibatch update (FusedUpdate.step: acas2d_ppo_update_f32 / acas2d_ppo_update_wide_f32) beside a replay
of the trainer's captured update graph, one JSON line per case.

  --timing   one minibatch update at B x D (default 4096, 1024 x 29, 53, 101, 197) on a trainer's own rollout buffers:
             HIP events around windows of >= --window seconds of back-to-back updates, every shape warmed up, the two
             variants alternating in one process, median of --reps windows; `spread` is (max - min) / median of a
             variant's windows.
  --learn    PPOTrainer.learn() env-steps/s at --envs x {16, 32, 64} traffic, 128 steps, 4 epochs, minibatch 4096, fused
             collector, updater "graphs" and "fused" alternating, --reps timed runs of --iters iterations each.
  --curves   evidence that learning is unchanged, not a test: --seeds of a fixed budget (--timesteps) at --traffic with each
             updater, the final deterministic evaluation on 100 fresh episodes side by side.
usage: bench_ppo_update.py --timing | --learn | --curves [options]"""
import argparse
import json
import math
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gym_acas2d_amd as g  # noqa: E402

DEV = "cuda:0"


def spread(runs):
    return (max(runs) - min(runs)) / float(np.median(runs))


def timing(args):
    for case in args.cases.split(","):
        B, D = (int(x) for x in case.split("x"))
        N = (D - 5) // 3
        E = 1024
        T = max(8, math.ceil(2 * B / E))
        venv = g.ACAS2DVecEnv(E, N, device=DEV, dtype=torch.float32, seed=13)
        tr = g.PPOTrainer(venv, g.PPOConfig(n_steps=T, batch_size=B, n_epochs=1), collector="fused", updater="graphs")
        tr.collect()                                           # captures the graphs, fills the buffers with a real rollout
        tr.mb_idx.copy_(torch.randperm(T * E, device=DEV)[:B])
        twin = g.ActorCritic(D).to(DEV)                        # the fused update steps a copy: the graph holds tr.policy
        twin.load_state_dict(tr.policy.state_dict())
        fu = g.FusedUpdate(twin, tr.cfg, tr.b_obs, tr.b_act, tr.b_logp, tr.b_adv, tr.b_ret)
        variants = {"graphs": tr._graphs[2].replay, "fused": lambda: fu.step(tr.mb_idx)}

        def window(fn, n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(n):
                fn()
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) * 1e3 / n                 # us per update

        count = {}
        for name, fn in variants.items():                      # warm-up, and the window's length from it
            window(fn, 50)
            count[name] = max(50, int(args.window * 1e6 / window(fn, 200)) + 1)
        runs = {name: [] for name in variants}
        for _ in range(args.reps):
            for name, fn in variants.items():
                runs[name].append(window(fn, count[name]))
        rec = {"bench": "timing", "rows": B, "obs_dim": D, "n_traffic": N, "entry": fu.entry, "reps": args.reps,
               "method": "HIP events, windows of >= %.1f s, variants alternating, median of reps; us per update" % args.window}
        for name in variants:
            rec[name + "_us"] = float(np.median(runs[name]))
            rec[name + "_runs_us"] = runs[name]
            rec[name + "_spread"] = spread(runs[name])
            rec[name + "_updates_per_window"] = count[name]
        rec["graphs_over_fused"] = rec["graphs_us"] / rec["fused_us"]
        rec["finite"] = bool(all(torch.isfinite(p).all() for p in list(twin.parameters()) + list(tr.policy.parameters())))
        print(json.dumps(rec), flush=True)
        del tr, venv, fu
        torch.cuda.empty_cache()


def learn(args):
    for N in (int(x) for x in args.traffic.split(",")):
        cfg = dict(n_steps=128, batch_size=4096, n_epochs=4)
        per_it = args.envs * cfg["n_steps"]
        trainers = {}
        for upd in ("graphs", "fused"):
            venv = g.ACAS2DVecEnv(args.envs, N, device=DEV, dtype=torch.float32, seed=13)
            trainers[upd] = g.PPOTrainer(venv, g.PPOConfig(**cfg), collector="fused", updater=upd)
            trainers[upd].learn(2 * per_it, log=None)          # capture + warm-up
        runs = {upd: [] for upd in trainers}
        for _ in range(args.reps):
            for upd, tr in trainers.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tr.learn(tr.num_timesteps + args.iters * per_it, log=None)
                torch.cuda.synchronize()
                runs[upd].append(args.iters * per_it / (time.perf_counter() - t0))
        rec = {"bench": "learn", "envs": args.envs, "n_traffic": N, "obs_dim": 5 + 3 * N, **cfg, "collector": "fused",
               "iters_per_run": args.iters, "reps": args.reps,
               "method": "wall clock around learn() between device synchronisations, updaters alternating, median of reps"}
        for upd in trainers:
            rec[upd + "_env_steps_per_s"] = float(np.median(runs[upd]))
            rec[upd + "_runs"] = runs[upd]
            rec[upd + "_spread"] = spread(runs[upd])
        rec["fused_over_graphs"] = rec["fused_env_steps_per_s"] / rec["graphs_env_steps_per_s"]
        print(json.dumps(rec), flush=True)
        del trainers
        torch.cuda.empty_cache()


def curves(args):
    N = int(args.traffic.split(",")[0])
    for seed in (int(x) for x in args.seeds.split(",")):
        for upd in ("graphs", "fused"):
            venv = g.ACAS2DVecEnv(args.envs, N, device=DEV, dtype=torch.float32, seed=13)
            tr = g.PPOTrainer(venv, g.PPOConfig(seed=seed), collector="fused", updater=upd)
            t0 = time.perf_counter()
            hist = tr.learn(int(args.timesteps), log=None)
            dt = time.perf_counter() - t0
            out = tr.evaluate(100, random.Random(7))           # the same 100 episodes for every run
            last = hist[-1]
            print(json.dumps({"bench": "curves", "updater": upd, "seed": seed, "envs": args.envs, "n_traffic": N,
                              "timesteps": tr.num_timesteps, "seconds": dt, "train_ep_rew_mean": last.get("ep_rew_mean"),
                              "eval_mean_return": float(out["total_reward"].mean()),
                              "eval_goal": int((out["outcome"] == 1).sum()), "eval_collision": int((out["outcome"] == 2).sum()),
                              "eval_timeout": int((out["outcome"] == 3).sum()), "value_loss": last["value_loss"],
                              "std": last["std"]}), flush=True)
            del tr, venv
            torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--learn", action="store_true")
    ap.add_argument("--curves", action="store_true")
    ap.add_argument("--cases", default="4096x29,4096x53,4096x101,4096x197,1024x29,1024x53,1024x101,1024x197")
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--traffic", default="16,32,64")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--seeds", default="13,14,15")
    ap.add_argument("--timesteps", type=float, default=1.0e7)
    args = ap.parse_args()
    if args.timing:
        timing(args)
    if args.learn:
        learn(args)
    if args.curves:
        curves(args)
