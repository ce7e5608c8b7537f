#!/usr/bin/env python3
"""What clip_range_vf and the schedule factors cost a minibatch update (ppo.FusedUpdateSet: acas2d_ppo_update_sb3_set_f32
beside acas2d_ppo_update_guarded_set_f32), one JSON line per case.

One update of K members on 4 096 rows each, at --cases (default D = 8 and 53, K = 1 and 8), three variants on the same
build, each on its own twin of the same population:
  guarded   FusedUpdateSet.step() through the guarded entry (diagnostics=True, no limit): the yardstick
  neutral   the new entry with neutral options: factors of 1, clip_range_vf 0 for every member (old_val is not read)
  clipped   the new entry with value clipping on for every member (clip_range_vf 0.5 against old values 0.8 off the
            critic's, so rows clip on both sides) and factors != 1 on the rate and both clips
HIP events around windows of >= --window seconds of back-to-back calls, every variant warmed up, the variants alternating in
one process, median of --reps windows; `spread` is (max - min) / median of a variant's windows.
`<variant>_exceeds_spreads`: every window of the variant was slower than every guarded one.  A record, not a gate.
usage: bench_sb3_update.py [--out profiles/sb3_update_timing.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gym_acas2d_amd as g  # noqa: E402

DEV = "cuda:0"
FACTORS = (0.5, 0.75, 1.5)                                 # on learning_rate, clip_range, clip_range_vf
sink = None


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if sink:
        sink.write(line + "\n")
        sink.flush()


def spread(runs):
    return (max(runs) - min(runs)) / float(np.median(runs))


def window(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n                     # us per update


def case(D, K, B, args):
    gen = torch.Generator(device=DEV).manual_seed(D + K)
    n = K * B
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=gen)  # noqa: E731
    obs, act, adv, ret = rnd(n, D).clamp(-1, 1), 0.7 * rnd(n), 2.0 * rnd(n), 2.0 + 3.0 * rnd(n)
    members = []
    for k in range(K):
        torch.manual_seed(13 + k)
        members.append(g.ActorCritic(D).to(DEV))
    with torch.no_grad():                                  # a second-epoch minibatch: ratios near 1, a few of them clipped
        out = [m.forward(obs[k * B:(k + 1) * B]) for k, m in enumerate(members)]
        old_logp = torch.cat([g.ppo._normal_logp(o[0], m.log_std, act[k * B:(k + 1) * B].unsqueeze(-1))
                              for k, (m, o) in enumerate(zip(members, out))]) + 0.1 * rnd(n)
        old_val = (torch.cat([o[1] for o in out]) + 0.8 * rnd(n)).contiguous()
    base = dict(learning_rate=0.0)                         # the same minibatch every call: the weights stay
    const = lambda x: (lambda p: x)  # noqa: E731
    configs = {"guarded": [g.PPOConfig(seed=13 + k, **base) for k in range(K)],
               "neutral": [g.PPOConfig(seed=13 + k, learning_rate_schedule=const(1.0), **base) for k in range(K)],
               "clipped": [g.PPOConfig(seed=13 + k, clip_range_vf=0.5, learning_rate_schedule=const(FACTORS[0]),
                                       clip_range_schedule=const(FACTORS[1]), clip_range_vf_schedule=const(FACTORS[2]), **base)
                           for k in range(K)]}
    idx = torch.stack([k * B + torch.randperm(B, device=DEV, generator=gen) for k in range(K)]).contiguous()
    fus = {}
    for name, cfgs in configs.items():
        pset = g.ActorCriticSet.from_members(members)
        fus[name] = g.FusedUpdateSet(pset, cfgs, obs, act, old_logp, adv, ret, diagnostics=True, old_val=old_val)
        fus[name].begin_update()
    assert not fus["guarded"].options and fus["neutral"].options and fus["clipped"].options
    variants = {name: (lambda fu=fu: fu.step(idx)) for name, fu in fus.items()}
    count = {}
    for name, fn in variants.items():                      # warm-up, and the window's length from it
        window(fn, 5)
        count[name] = max(5, int(args.window * 1e6 / window(fn, 10)) + 1)
    runs = {name: [] for name in variants}
    for _ in range(args.reps):
        for name, fn in variants.items():
            runs[name].append(window(fn, count[name]))
    rec = {"bench": "sb3_update", "obs_dim": D, "members": K, "rows_per_member": B, "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "factors": list(FACTORS),
           "value_loss_last": {name: fu.stats[:, 5].cpu().tolist()[0] for name, fu in fus.items()},
           "method": "HIP events, windows of >= %.1f s, variants alternating, median of reps; us per minibatch update of all "
                     "members" % args.window}
    for name in variants:
        rec[name + "_us"] = float(np.median(runs[name]))
        rec[name + "_runs_us"] = runs[name]
        rec[name + "_spread"] = spread(runs[name])
        rec[name + "_calls_per_window"] = count[name]
    for name in ("neutral", "clipped"):
        rec[name + "_over_guarded"] = rec[name + "_us"] / rec["guarded_us"]
        rec[name + "_exceeds_spreads"] = bool(min(runs[name]) > max(runs["guarded"]))
    emit(rec)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="8x1,8x8,53x1,53x8", help="obs_dim x members, comma-separated")
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sb3_update.py measures on the GPU"
    sink = open(args.out, "a") if args.out else None
    for c in args.cases.split(","):
        D, K = (int(x) for x in c.split("x"))
        case(D, K, args.rows, args)
