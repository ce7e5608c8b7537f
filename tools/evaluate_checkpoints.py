#!/usr/bin/env python3
"""checkpoint_testing_main.py for a whole training run: every `model_<n>_steps.zip` under DIR (and DIR/checkpoints)
plus `best_model.zip`, scored deterministically on the reference's 100 test episodes (the first 100 games of the
seed-13 MT19937 stream, as testing_main.py and tools/train_ppo.py draw them) in ONE launch (evaluate_policies_fused).
One JSON line per checkpoint, in timestep order, best_model.zip last.  --safety adds the per-episode safety statistics
of the same launch (evaluate_policies_fused(safety=True)) over the finished episodes: the mean and the worst minimum
separation, the share of episodes that lost separation (los_steps > 0), the mean of the largest |a_lat| and the mean of
the mean |deviation| from the planned path.
--monte-carlo LANESxEPISODES instead plays a Monte Carlo campaign (policy.MonteCarlo): every checkpoint meets the same
LANES x EPISODES randomly drawn encounters of seed 13, and one JSON line per checkpoint gives its collision rate with the
Wilson 95 % interval, the goal / timeout / loss-of-separation rates, mean steps and mean return with its standard error.
--baseline-zero appends the all-zero policy (the unequipped aircraft: baseline_main.py's constant action [0]) and adds
each checkpoint's risk ratio against it.  --disturbance sep=PX,cpa=PX,closing=V,action=A[,seed=S] plays the campaign under
white sensor noise (standard deviations in pixels and in the units of v_closing, per traffic aircraft and step) and actuator
disturbance (in units of the action) -- policy.Disturbance, float32; the flag may be repeated to sweep levels: the same
encounters at every level, the checkpoint lines of each level carrying its disturbance, and one summary line per level.
With rho=R (all four channels) or rho_sep=, rho_cpa=, rho_closing=, rho_action= among the keys the errors persist: a
first-order Gauss-Markov process per channel with step-to-step correlation R in [0, 1], 1 being a constant bias per episode
(policy.CorrelatedDisturbance); a string without them is the white noise it has always been.
With delay=STEPS and / or lag=L among the keys the aircraft flies the action the policy gave STEPS steps earlier (0 until the
first one arrives: a pilot's response delay, 50 steps being half a second) through a first-order lag with pole L in [0, 1]
(policy.DelayedDisturbance; the rho keys go with it as before).
--search CANDIDATESxGENERATIONS instead runs an encounter search per checkpoint (policy.EncounterSearch: cross-entropy
proposals refit on the device, importance-sampling weights): one JSON line per checkpoint gives the estimated probability of
min_separation <= the collision distance with its standard error, beside a crude campaign of the same number of episodes
(that campaign's share of episodes below the same separation, and its collision rate with the Wilson 95 % interval), and the
closest encounter found.

    python tools/evaluate_checkpoints.py DIR [--dtype float64|float32] [--episodes 100] [--safety]
    python tools/evaluate_checkpoints.py DIR --search 65536x8 [--dtype float32]
    python tools/evaluate_checkpoints.py DIR --monte-carlo 65536x64 [--baseline-zero] [--dtype float32]
    python tools/evaluate_checkpoints.py DIR --monte-carlo 65536x8 --dtype float32 --baseline-zero \
        --disturbance sep=0,cpa=0,closing=0,action=0 --disturbance sep=90,cpa=40,closing=8,action=0.1,seed=7
    python tools/evaluate_checkpoints.py DIR --monte-carlo 65536x8 --dtype float32 --disturbance sep=90,cpa=40,rho=0.99,seed=7
    python tools/evaluate_checkpoints.py DIR --monte-carlo 65536x8 --dtype float32 --disturbance delay=50,lag=0.5
"""
import argparse
import glob
import json
import os
import random
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gym_acas2d_amd as g  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("dir")
ap.add_argument("--dtype", choices=("float64", "float32"), default="float64")
ap.add_argument("--episodes", type=int, default=100)
ap.add_argument("--safety", action="store_true")
ap.add_argument("--monte-carlo", metavar="LANESxEPISODES", default=None)
ap.add_argument("--baseline-zero", action="store_true")
ap.add_argument("--search", metavar="CANDIDATESxGENERATIONS", default=None)
ap.add_argument("--disturbance", metavar="sep=..,cpa=..,closing=..,action=..[,seed=..]", action="append", default=None)
args = ap.parse_args()


def parse_disturbance(text):
    if g.policy.DelayedDisturbance.has_response(text):   # a response delay and / or a lag: policy.DelayedDisturbance
        try:
            return g.policy.DelayedDisturbance.parse(text)
        except ValueError as e:
            sys.exit("--disturbance: %s" % e)
    if g.policy.CorrelatedDisturbance.has_rho(text):     # a Gauss-Markov error per channel: policy.CorrelatedDisturbance
        try:
            return g.policy.CorrelatedDisturbance.parse(text)
        except ValueError as e:
            sys.exit("--disturbance: %s" % e)
    kw = {}
    for item in text.split(","):
        key, _, val = item.partition("=")
        if key.strip() not in ("sep", "cpa", "closing", "action", "seed") or not val:
            sys.exit("--disturbance: %r (sep=, cpa=, closing=, action= and seed= are understood)" % item)
        kw[key.strip()] = int(val, 0) if key.strip() == "seed" else float(val)
    return g.policy.Disturbance(**kw)


if args.disturbance and not args.monte_carlo:
    sys.exit("--disturbance goes with --monte-carlo")

steps_of = lambda p: int(re.search(r"model_(\d+)_steps\.zip$", p).group(1))  # noqa: E731
ckpts = sorted({p for d in (args.dir, os.path.join(args.dir, "checkpoints"))
                for p in glob.glob(os.path.join(d, "model_*_steps.zip"))}, key=steps_of)
best = os.path.join(args.dir, "best_model.zip")
paths = ckpts + ([best] if os.path.exists(best) else [])
if not paths:
    sys.exit("no model_*_steps.zip or best_model.zip under %s" % args.dir)

if args.monte_carlo:
    lanes, episodes = (int(x) for x in args.monte_carlo.lower().split("x"))
    pols, names = list(paths), [os.path.relpath(p, args.dir) for p in paths]
    if args.baseline_zero:
        D = g.ACAS2DConfig().obs_dim
        pols.append((torch.zeros(64, D), torch.zeros(64), torch.zeros(64, 64), torch.zeros(64), torch.zeros(1, 64), torch.zeros(1)))
        names.append("zero (unequipped)")
    for level in [parse_disturbance(t) for t in args.disturbance] if args.disturbance else [None]:
        mc = g.MonteCarlo(pols, lanes, seed=13, dtype=getattr(torch, args.dtype), disturbance=level).run(episodes)
        s = mc.summary(baseline=len(pols) - 1 if args.baseline_zero else None)
        scalars = [k for k, v in s.items() if np.ndim(v) == 1 and k != "hist_edges"]
        for k, name in enumerate(names):
            row = {"checkpoint": name, "timesteps": steps_of(paths[k]) if k < len(ckpts) else None}
            row.update({key: (int(s[key][k]) if s[key].dtype.kind == "i" else float(s[key][k])) for key in scalars})
            row["sep_hist"] = [int(x) for x in s["sep_hist"][k]]
            if level is not None:
                row["disturbance"] = level.to_dict()
            print(json.dumps(row), flush=True)
        last = {"hist_edges": [float(x) for x in s["hist_edges"]], "lanes": lanes, "episodes_per_lane": episodes}
        if level is not None:                            # the level's summary line: what a sweep is read by
            last.update(disturbance=level.to_dict(), collision_rate=[float(x) for x in s["collision_rate"]],
                        los_rate=[float(x) for x in s["los_rate"]])
            if "risk_ratio" in s:
                last["risk_ratio"] = [float(x) for x in s["risk_ratio"]]
        print(json.dumps(last), flush=True)
    sys.exit(0)

if args.search:
    cand, gens = (int(x) for x in args.search.lower().split("x"))
    dt = getattr(torch, args.dtype)
    es = g.EncounterSearch(paths, cand, seed=13, dtype=dt).run(gens)
    est, hist, closest = es.estimate(first_generation=min(2, gens - 1)), es.history(), es.best()
    mc = g.MonteCarlo(paths, cand, seed=13, dtype=dt).run(gens)
    acc, s = mc.accumulators(), mc.summary()
    edge = es.level * mc.inv_bin_width                       # the crude share below `level`: where a bin edge lies on it
    below = acc["sep_hist"][:, :int(edge)].sum(1) if edge == int(edge) else None
    for k, path in enumerate(paths):
        b = closest[k]
        row = {"checkpoint": os.path.relpath(path, args.dir), "timesteps": steps_of(path) if k < len(ckpts) else None,
               "level": es.level, "episodes": cand * gens, "estimate": float(est["p"][k]), "estimate_se": float(est["se"][k]),
               "estimate_generations": int(est["generations"]), "events_per_generation": [int(x) for x in hist[:, k, 5]],
               "crude_below_level": None if below is None else float(below[k]) / (cand * gens),
               "crude_collision_rate": float(s["collision_rate"][k]),
               "crude_collision_rate_95": [float(s["collision_rate_lo"][k]), float(s["collision_rate_hi"][k])],
               "closest": None if b is None else {"generation": b[0], "candidate": b[1], "min_separation": float(b[2]),
                                                  "own": b[3][0].tolist(), "traffic": b[4][0].tolist()}}
        print(json.dumps(row), flush=True)
    sys.exit(0)

own, trf, goal = g.reset_parity.draw_episodes(g.ACAS2DConfig(), args.episodes, random.Random(13))
out = g.evaluate_policies_fused(paths, own, trf, goal, dtype=getattr(torch, args.dtype), safety=args.safety)
for k, p in enumerate(paths):
    r, s, oc = out["total_reward"][k], out["steps"][k], out["outcome"][k]
    row = {"checkpoint": os.path.relpath(p, args.dir), "timesteps": steps_of(p) if p != best else None,
           "mean_return": float(r.mean()), "std_return": float(r.std()), "mean_steps": float(s.mean()),
           "goal": int((oc == 1).sum()), "collision": int((oc == 2).sum()), "timeout": int((oc == 3).sum()),
           "unfinished": int(out["unfinished"][k])}
    if args.safety:
        fin = oc != 0                                    # an unfinished episode holds zeros, not statistics
        stat = lambda key, f: float(f(out[key][k][fin])) if fin.any() else None  # noqa: E731
        row.update({"mean_min_separation": stat("min_separation", np.mean), "worst_min_separation": stat("min_separation", np.min),
                    "los_share": stat("los_steps", lambda a: (a > 0).mean()), "mean_max_abs_a_lat": stat("max_abs_a_lat", np.mean),
                    "mean_abs_deviation": stat("mean_abs_deviation", np.mean)})
    print(json.dumps(row), flush=True)
