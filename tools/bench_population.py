#!/usr/bin/env python3
"""K PPO learners as ONE population (ppo.PopulationTrainer) against K sequential solo PPOTrainer.learn() runs, in one
process: aggregate env-steps per second of learn(), and where an iteration's time goes.

Per K: both variants are constructed and warmed up (one iteration each), then timed in ALTERNATING windows of --iters
iterations, host clock around work that ends in a synchronise; reported: the median of --windows windows and their
spread (min, max).  Each member / solo run has --envs envs x --traffic aircraft, --n-steps steps per iteration and
minibatches of --batch-size; fused collector and fused update in both variants.  At --traffic 16, 32, 64 the population
is PopulationTrainer(group=True) (the group-cooperative set collector, the wide set update); the sequential PPOTrainer
takes the group and wide launches by itself.

Then, per K, three single operations (median of --reps timings, each ended by a synchronise):
  collect_set   one ACAS2DVecEnv.collect_set() launch of --n-steps steps (with the copy of the first observation)
  update_set    one FusedUpdateSet.step() at B = --batch-size and at B = 1 024 (a batch of 20 calls / 20)
  remainder     an iteration of learn() minus its collect_set launch and its update_set calls: GAE, buffer copies,
                permutations, index gathers, the episode statistics

    python tools/bench_population.py --members 1 2 4 8 16 --out profiles/population_timing.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gym_acas2d_amd as g  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--members", type=int, nargs="+", default=[1, 2, 4, 8, 16])
ap.add_argument("--envs", type=int, default=1024, help="envs per member / solo run")
ap.add_argument("--traffic", type=int, default=1)
ap.add_argument("--n-steps", type=int, default=512)
ap.add_argument("--batch-size", type=int, default=4096)
ap.add_argument("--n-epochs", type=int, default=None, help="epochs per iteration (default: PPOConfig's)")
ap.add_argument("--iters", type=int, default=1, help="iterations per timed window")
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--gae", choices=("torch", "kernel"), default="torch",
                help="GAE of BOTH variants: torch's compute_gae or the one-launch kernel (ppo.gae_fused); the same bits")
ap.add_argument("--out", default=None)
args = ap.parse_args()
DEV = "cuda:0"
sink = open(args.out, "a") if args.out else None


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if sink:
        sink.write(line + "\n")
        sink.flush()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


epochs_kw = {} if args.n_epochs is None else {"n_epochs": args.n_epochs}
cfg = lambda seed: g.PPOConfig(seed=seed, n_steps=args.n_steps, batch_size=args.batch_size, **epochs_kw)  # noqa: E731
per_it = args.n_steps * args.envs                     # one member's env steps per iteration
GROUP = args.traffic in g.ppo.GROUP_TRAFFIC
group_kw = {"group": True} if GROUP else {}
shape = {"envs_per_member": args.envs, "n_traffic": args.traffic, "n_steps": args.n_steps, "batch_size": args.batch_size,
         "n_epochs": cfg(0).n_epochs, "gae": args.gae, "iters_per_window": args.iters, "windows": args.windows, "device": torch.cuda.get_device_name(0)}

# the baseline's solo trainers: the parent path, one learner each, built once and reused for every K
solos = []
for k in range(max(args.members)):
    venv = g.ACAS2DVecEnv(args.envs, args.traffic, device=DEV, seed=13)
    tr = g.PPOTrainer(venv, cfg(13 + k), collector="fused", updater="fused", gae=args.gae)
    tr.learn(per_it, log=None)                        # warm-up: graph capture, first launches
    solos.append(tr)

for K in args.members:
    venv = g.ACAS2DVecEnv(K * args.envs, args.traffic, device=DEV, seed=13)
    pop = g.PopulationTrainer(venv, [cfg(13 + k) for k in range(K)], gae=args.gae, **group_kw)
    pop.learn(per_it, log=None)                       # warm-up

    def run_population():
        pop.learn(pop.num_timesteps + args.iters * per_it, log=None)

    def run_sequential():
        for tr in solos[:K]:
            tr.learn(tr.num_timesteps + args.iters * per_it, log=None)

    t_pop, t_seq = [], []
    for _ in range(args.windows):                     # variants alternating
        t_pop.append(timed(run_population))
        t_seq.append(timed(run_sequential))
    steps = K * args.iters * per_it
    sp, ss = spread(t_pop), spread(t_seq)
    rate = lambda s: {"median": steps / s["median"], "min": steps / s["max"], "max": steps / s["min"]}  # noqa: E731
    emit({"what": "learn", "members": K, **shape, "population_s": sp, "sequential_s": ss,
          "population_steps_per_s": rate(sp), "sequential_steps_per_s": rate(ss),
          "gain": ss["median"] / sp["median"],
          "gain_exceeds_spreads": bool(sp["max"] < ss["min"])})

    # ---- the single operations
    out = pop._fused_out
    t_collect = [timed(lambda: venv.collect_set(pop.policy_set, args.n_steps, pop.noise_seeds, noise_step=0, out=out, **group_kw))
                 for _ in range(args.reps)]
    fu = pop._fused_update
    n = args.n_steps * args.envs
    t_update = {}
    for B in sorted({min(args.batch_size, n), min(1024, n)}):
        idx = pop.member_rows[:, torch.randperm(n, device=DEV)[:B]].contiguous()
        for _ in range(3):
            fu.step(idx)

        def calls():
            for _ in range(20):
                fu.step(idx)
        t_update[B] = spread([timed(calls) / 20 for _ in range(args.reps)])
    t_iter = [timed(run_population) / args.iters for _ in range(args.reps)]
    n_mb = pop.cfg.n_epochs * (n // pop.mb_idx.shape[1] + (1 if pop.mb_tail is not None else 0))
    b_main = pop.mb_idx.shape[1]
    remainder = statistics.median(t_iter) - statistics.median(t_collect) - n_mb * t_update[b_main]["median"]
    emit({"what": "operations", "members": K, **shape, "collect_set_s": spread(t_collect),
          "update_set_s": {str(B): v for B, v in t_update.items()}, "iteration_s": spread(t_iter),
          "minibatches_per_iteration": n_mb, "remainder_s": remainder})
    del pop, venv
    torch.cuda.empty_cache()
