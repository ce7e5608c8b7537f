#!/usr/bin/env python3
"""training_main.py equivalent on the MI355X engine: PPO on E parallel ACAS2D envs, everything on
the GPU.  Prints one JSON line per iteration; evaluates the final policy deterministically on the
reference's 100 test episodes (testing_main.py)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gym_acas2d_amd as g  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=1024)
ap.add_argument("--traffic", type=int, default=1)
ap.add_argument("--timesteps", type=float, default=6.0e7)
ap.add_argument("--n-steps", type=int, default=512)   # (512 x 4096: 100 / 100 goals on three seeds, ppo_seed_sweep.py)
ap.add_argument("--batch-size", type=int, default=4096)
ap.add_argument("--collector", choices=("graphs", "fused", "eager"), default="fused",
                help="fused: the whole collection of an iteration in one hand-written launch (ACAS2DVecEnv.collect)")
ap.add_argument("--updater", choices=("graphs", "fused"), default=None,
                help="fused (default where it is built and measured faster: --traffic 1, 2, 3, 4, 8 -- acas2d_ppo_update_f32 "
                     "-- and 16, 32, 64 -- acas2d_ppo_update_wide_f32; tools/bench_ppo_update.py): every minibatch update as "
                     "two hand-written launches; graphs: captured torch ops")
ap.add_argument("--gae", choices=("torch", "kernel"), default=None,
                help="kernel: the GAE of an iteration as one hand-written launch (ppo.gae_fused: acas2d_gae_f32; the same bits "
                     "as torch's compute_gae; needs --collector fused); the default follows tools/bench_gae.py's measurement "
                     "(DESIGN.md 4.2f): GAE_DEFAULT below")
ap.add_argument("--seed", type=int, default=13)
ap.add_argument("--target-kl", type=float, default=None,
                help="SB3's target_kl: a learner whose minibatch approx_kl exceeds 1.5 x this sits out the rest of that update "
                     "(fused updater: decided inside the update's own launches, DESIGN.md 4.2h; --collector eager: SB3's break); "
                     "the log then carries approx_kl, clip_fraction, n_applied, early_stop and explained_variance.  Not with "
                     "--updater graphs")
ap.add_argument("--clip-range-vf", type=float, default=None, metavar="X",
                help="SB3's clip_range_vf: the value loss on old_values + clamp(values - old_values, -X, X), inside the fused "
                     "update's launches (DESIGN.md 4.2j) or op by op (--collector eager).  It depends on the reward scale: "
                     "returns here are of order 1e3.  Not with --updater graphs")
ap.add_argument("--lr-schedule", choices=("constant", "linear"), default="constant",
                help="linear: the learning rate falls linearly to 0 over --timesteps (SB3's linear schedule, as a factor on the "
                     "rate -- in a --pbt population on whatever rate the exploit steps have left a member)")
ap.add_argument("--clip-schedule", choices=("constant", "linear"), default="constant",
                help="linear: the clip range falls linearly to 0 over --timesteps, likewise")
ap.add_argument("--reward-norm", action="store_true",
                help="SB3's VecNormalize(norm_obs=False, norm_reward=True): every collected reward divided by the running standard "
                     "deviation of the discounted return and clipped to +-10, on the device before GAE (ppo.RewardNormalizer, "
                     "DESIGN.md 4.2k; per member in a population, inherited from the donor at a --pbt exploit step).  Episode "
                     "returns, evaluations and PBT scores stay raw; the log gains reward_std.  Needs --collector fused")
ap.add_argument("--population", type=int, default=0, metavar="K",
                help="train K learners with the seeds --seed ... --seed + K - 1 side by side in one process "
                     "(ppo.PopulationTrainer: one collection launch and two launches per minibatch for all K; each member gets "
                     "--envs envs; float32, --traffic 1, 2, 3, 4, 8 and -- PopulationTrainer(group=True): the group-cooperative "
                     "collector and the wide update -- 16, 32, 64; fused collector and update)")
ap.add_argument("--pbt", action="store_true",
                help="with --population: population-based training (ppo.PBTTrainer) -- every --pbt-every iterations the "
                     "--pbt-fraction worst members by training return copy one of the best and perturb its learning rate, clip "
                     "range and entropy coefficient, scored and decided on the device (DESIGN.md 4.2g)")
ap.add_argument("--pbt-every", type=int, default=8, help="iterations between two exploit steps")
ap.add_argument("--pbt-fraction", type=float, default=0.25, help="the share of members replaced at an exploit step")
ap.add_argument("--disturbance", metavar="sep=..,cpa=..,closing=..,action=..[,seed=..]", action="append", default=None,
                help="train under white sensor noise (standard deviations in pixels and in the units of v_closing, per traffic "
                     "aircraft and step) and actuator disturbance (in units of the action), in the syntax of "
                     "tools/evaluate_checkpoints.py (policy.Disturbance; DESIGN.md 4.2p): the actor and the critic read the "
                     "disturbed observation, the update is given those rows.  Needs --collector fused.  With --population: once "
                     "for all members, or K times, one per member, with equal seeds.  With rho=.. (all four channels) or "
                     "rho_sep=, rho_cpa=, rho_closing=, rho_action= the errors persist from step to step (policy."
                     "CorrelatedDisturbance in a CorrelatedDisturbanceSet, which holds the per-env error state between the "
                     "collection launches; DESIGN.md 4.2r): rho 1 is a constant bias per episode")
ap.add_argument("--disturbance-normalised", action="store_true",
                help="--disturbance's sep, cpa and closing are in units of the normalised observation instead")
ap.add_argument("--out", default=None)


def training_disturbances(texts, n_members, normalised):
    """--disturbance's texts as the trainers take them: a text that names a correlation makes the set a
    CorrelatedDisturbanceSet (its other members white: rho 0), else one Disturbance or one per member as before.  A text with
    delay= or lag= is a DelayedDisturbance, which the trainers refuse in their own words (it is for the evaluator and the
    campaign)."""
    if any(g.DelayedDisturbance.has_response(t) for t in texts):
        ds = [g.DelayedDisturbance.parse(t, normalised=normalised) if g.DelayedDisturbance.has_response(t)
              else g.Disturbance.parse(t, normalised=normalised) for t in texts]
        return g.CorrelatedDisturbanceSet(ds[0] if len(ds) == 1 else ds, n_members)         # raises: no response in a collector
    if any(g.CorrelatedDisturbance.has_rho(t) for t in texts):
        ds = [g.CorrelatedDisturbance.parse(t, normalised=normalised) if g.CorrelatedDisturbance.has_rho(t)
              else g.Disturbance.parse(t, normalised=normalised) for t in texts]
        return g.CorrelatedDisturbanceSet(ds[0] if len(ds) == 1 else ds, n_members)
    ds = [g.Disturbance.parse(t, normalised=normalised) for t in texts]
    return ds[0] if len(ds) == 1 else ds


args = ap.parse_args()
if args.pbt and not args.population:
    ap.error("--pbt needs --population K")
DISTURBANCES = None
if args.disturbance:
    if len(args.disturbance) not in (1, max(args.population, 1)):
        ap.error("--disturbance: once, or once per member of --population (got %d)" % len(args.disturbance))
    if args.collector != "fused" and not args.population:
        ap.error("--disturbance needs --collector fused: the noise is drawn inside the fused collection launch")
    try:
        DISTURBANCES = training_disturbances(args.disturbance, max(args.population, 1), args.disturbance_normalised)
    except ValueError as e:
        ap.error(str(e))
REWARD_NORM = True if args.reward_norm else None
# clip_range_vf and the schedules, as PPOConfig takes them
OPTIONS = dict(clip_range_vf=args.clip_range_vf,
               learning_rate_schedule=g.ppo.linear_schedule() if args.lr_schedule == "linear" else None,
               clip_range_schedule=g.ppo.linear_schedule() if args.clip_schedule == "linear" else None)
# "kernel" where learn() with it beat gae="torch" by more than both variants' spreads (the fused-collector
# PPOTrainer by 2 % at 512 steps and 13 % at 128, the population by 3 %); a trainer that were not faster would say "torch"
GAE_DEFAULT = {"population": "kernel", "solo": "kernel"}
if args.gae is None:
    args.gae = GAE_DEFAULT["population"] if args.population else (GAE_DEFAULT["solo"] if args.collector == "fused" else "torch")
if args.updater is None:
    # fused wherever it is built: it was measured faster than the captured graph at every one of these widths
    # (a width where it were not would be left out of this tuple)
    args.updater = "fused" if args.traffic in (1, 2, 3, 4, 8, 16, 32, 64) else "graphs"
    if args.updater == "graphs":
        print(json.dumps({"note": "updater=graphs: the fused update is built for traffic 1, 2, 3, 4, 8, 16, 32, 64 (obs_dim 8, "
                                  "11, 14, 17, 29, 53, 101, 197), --traffic %d has obs_dim %d"
                                  % (args.traffic, 5 + 3 * args.traffic)}), flush=True)

if args.population:
    import helpers as H
    K = args.population
    venv = g.ACAS2DVecEnv(K * args.envs, args.traffic, device="cuda:0", dtype=torch.float32, seed=13)
    cfgs = [g.PPOConfig(n_steps=args.n_steps, batch_size=args.batch_size, seed=args.seed + k, target_kl=args.target_kl,
                        **OPTIONS) for k in range(K)]
    if args.pbt:
        pop = g.PBTTrainer(venv, cfgs, g.PBTConfig(ready_every=args.pbt_every, fraction=args.pbt_fraction, seed=args.seed),
                           gae=args.gae, group=args.traffic in g.ppo.GROUP_TRAFFIC, reward_norm=REWARD_NORM,
                           disturbances=DISTURBANCES)
    else:
        pop = g.PopulationTrainer(venv, cfgs, gae=args.gae, group=args.traffic in g.ppo.GROUP_TRAFFIC, reward_norm=REWARD_NORM,
                                  disturbances=DISTURBANCES)
    pop.learn(int(args.timesteps), log=lambda r: print(json.dumps(r), flush=True))
    if args.traffic == 1:
        own, trf, goal = H.parity_reset_states(g.ACAS2DConfig(), 13, 0, 100)
        out = g.evaluate_policies_fused(pop.policy_set.actor_weights(), own, trf, goal)
        for k in range(K):
            print(json.dumps({"member": k, "seed": args.seed + k, "eval_100_reference_episodes": {
                "mean_return": float(out["total_reward"][k].mean()), "mean_steps": float(out["steps"][k].mean()),
                "goal": int((out["outcome"][k] == 1).sum()), "collision": int((out["outcome"][k] == 2).sum()),
                "timeout": int((out["outcome"][k] == 3).sum())}}))
    if args.out:
        torch.save({n: t.cpu() for n, t in pop.policy_set.params.items()}, args.out)      # the [K, ...] stacks
    sys.exit(0)

venv = g.ACAS2DVecEnv(args.envs, args.traffic, device="cuda:0", dtype=torch.float32, seed=13)
trainer = g.PPOTrainer(venv, g.PPOConfig(n_steps=args.n_steps, batch_size=args.batch_size, seed=args.seed, target_kl=args.target_kl,
                                         **OPTIONS),
                       collector=args.collector,
                       use_graphs=args.collector != "eager", updater=args.updater if args.collector != "eager" else "graphs", gae=args.gae,
                       reward_norm=REWARD_NORM, disturbance=DISTURBANCES)
hist = trainer.learn(int(args.timesteps), log=lambda r: print(json.dumps(r), flush=True))

if args.traffic == 1:
    import helpers as H
    own, trf, goal = H.parity_reset_states(g.ACAS2DConfig(), 13, 0, 100)
    out = g.evaluate_policy_fused(trainer.policy, own, trf, goal)     # predict + step x 1001 in one launch
    print(json.dumps({"eval_100_reference_episodes": {"mean_return": float(out["total_reward"].mean()),
                                                      "mean_steps": float(out["steps"].mean()),
                                                      "goal": int((out["outcome"] == 1).sum()),
                                                      "collision": int((out["outcome"] == 2).sum()),
                                                      "timeout": int((out["outcome"] == 3).sum())},
                      "reference_trained_policy": {"mean_return": 1210.07, "mean_steps": 704.35, "goal": 100}}))
if args.out:
    torch.save(trainer.policy.state_dict(), args.out)
