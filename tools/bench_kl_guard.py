#!/usr/bin/env python3
"""What the target_kl guard costs a minibatch update (ppo.FusedUpdateSet: acas2d_ppo_update_guarded_set_f32 beside
acas2d_ppo_update_set_f32 / acas2d_ppo_update_wide_set_f32), one JSON line per case.

One update of K members on 4 096 rows each, at --cases (default D = 8 and 53, K = 1 and 8), three variants on the same
build, each on its own twin of the same population:
  unguarded   FusedUpdateSet.step() through the unguarded entry: the yardstick
  guarded     the same update through the guarded entry with the limit off (target_kl 0: statistics only)
  stopped     the guarded entry with every member stopped: what the launches the host still issues after a stop cost
HIP events around windows of >= --window seconds of back-to-back calls, every variant warmed up, the variants alternating in
one process, median of --reps windows; `spread` is (max - min) / median of a variant's windows.
`guarded_exceeds_spreads`: every guarded window was slower than every unguarded one.
usage: bench_kl_guard.py [--out profiles/kl_guard_timing.jsonl]"""
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
        old_logp = torch.cat([g.ppo._normal_logp(m.forward(obs[k * B:(k + 1) * B])[0], m.log_std, act[k * B:(k + 1) * B].unsqueeze(-1))
                              for k, m in enumerate(members)]) + 0.1 * rnd(n)
    cfgs = [g.PPOConfig(seed=13 + k, learning_rate=0.0) for k in range(K)]     # the same minibatch every call: the weights stay
    idx = torch.stack([k * B + torch.randperm(B, device=DEV, generator=gen) for k in range(K)]).contiguous()
    fus = {}
    for name in ("unguarded", "guarded", "stopped"):
        pset = g.ActorCriticSet.from_members(members)
        fus[name] = g.FusedUpdateSet(pset, cfgs, obs, act, old_logp, adv, ret, diagnostics=name != "unguarded")
    fus["stopped"].stopped.fill_(1)
    variants = {name: (lambda fu=fu: fu.step(idx)) for name, fu in fus.items()}
    count = {}
    for name, fn in variants.items():                      # warm-up, and the window's length from it
        window(fn, 5)
        count[name] = max(5, int(args.window * 1e6 / window(fn, 10)) + 1)
    runs = {name: [] for name in variants}
    for _ in range(args.reps):
        for name, fn in variants.items():
            runs[name].append(window(fn, count[name]))
    steps = {name: fu.step_count.cpu().tolist() for name, fu in fus.items()}
    assert steps["stopped"] == [0] * K and fus["stopped"].diag.abs().max().item() == 0.0       # nothing ran
    rec = {"bench": "kl_guard", "obs_dim": D, "members": K, "rows_per_member": B, "entry": fus["unguarded"].entry,
           "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "approx_kl_last": fus["guarded"].diag[:, 2].cpu().tolist()[0], "clip_fraction_last": fus["guarded"].diag[:, 3].cpu().tolist()[0],
           "method": "HIP events, windows of >= %.1f s, variants alternating, median of reps; us per minibatch update of all "
                     "members" % args.window}
    for name in variants:
        rec[name + "_us"] = float(np.median(runs[name]))
        rec[name + "_runs_us"] = runs[name]
        rec[name + "_spread"] = spread(runs[name])
        rec[name + "_calls_per_window"] = count[name]
    rec["guarded_over_unguarded"] = rec["guarded_us"] / rec["unguarded_us"]
    rec["stopped_over_unguarded"] = rec["stopped_us"] / rec["unguarded_us"]
    rec["guarded_exceeds_spreads"] = bool(min(runs["guarded"]) > max(runs["unguarded"]))
    emit(rec)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="8x1,8x8,53x1,53x8", help="obs_dim x members, comma-separated")
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_kl_guard.py measures on the GPU"
    sink = open(args.out, "a") if args.out else None
    for c in args.cases.split(","):
        D, K = (int(x) for x in c.split("x"))
        case(D, K, args.rows, args)
