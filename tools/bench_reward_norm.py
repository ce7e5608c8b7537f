#!/usr/bin/env python3
"""Reward normalisation as one ABI call (ppo.RewardNormalizer: acas2d_reward_normalize_f32) beside its torch float64
restatement row by row (ppo.normalize_rewards_reference), one JSON line per case.

  --timing   one normalize() over [T][E] with K members at --cases TxExK (default 512x1024x1, 128x1024x1, 512x4096x4) on
             random rewards with dones, in place: the kernel; the torch restatement op by op ("eager") and as a replay of
             it captured in a hipGraph ("graph"); and, as a yardstick for a sweep over the same rows, acas2d_gae_f32 on
             the same shape ("gae").  HIP events around windows of >= --window seconds of back-to-back calls, every variant
             warmed up, the variants alternating in one process, median of --reps windows; `spread` is (max - min) /
             median of a variant's windows.  Before anything is timed the kernel's output and state are compared with the
             restatement's from the same start (`max_ulp`, `differing`, `rel_stats`).
  --learn    learn() env-steps/s of PPOTrainer(collector="fused", updater="fused", gae="kernel") with reward_norm=True
             against reward_norm=None at 1 024 envs x 8 traffic, 512 steps, minibatch 4 096: alternating, --reps timed runs
             of --iters iterations each.
usage: bench_reward_norm.py --timing | --learn [--out profiles/reward_norm_timing.jsonl]"""
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
sink = None


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if sink:
        sink.write(line + "\n")
        sink.flush()


def spread(runs):
    return (max(runs) - min(runs)) / float(np.median(runs))


def timing(args):
    for case in args.cases.split(","):
        T, E, K = (int(x) for x in case.split("x"))
        gen = torch.Generator(device=DEV).manual_seed(T + E)
        raw = torch.randn(T, E, device=DEV, generator=gen)
        raw[torch.rand(T, E, device=DEV, generator=gen) < 0.05] = 1000.0
        done = torch.rand(T, E, device=DEV, generator=gen) < 0.01
        val = 50.0 * torch.randn(T, E, device=DEV, generator=gen)
        last_value = 50.0 * torch.randn(E, device=DEV, generator=gen)
        gamma = 0.99
        norm = g.RewardNormalizer(E, K, gamma=gamma, device=DEV)
        fresh = norm.state_dict()
        k_buf, r_buf = raw.clone(), raw.clone()
        r_returns, r_stats = norm.returns.clone(), norm.stats.clone()
        const = g.gae_constants(gamma, 0.95, K, torch.device(DEV))
        adv, ret = torch.empty_like(raw), torch.empty_like(raw)

        def kernel():
            norm.normalize(k_buf, done, out=k_buf)

        def reference():
            g.normalize_rewards_reference(r_buf, done, r_returns, r_stats, norm.gamma, n_members=K, out=r_buf)

        def gae():
            g.gae_fused(raw, val, done, last_value, n_members=K, constants=const, out={"adv": adv, "ret": ret})

        # the same start, one call each: the kernel against the restatement
        kernel()
        reference()
        torch.cuda.synchronize()
        ordered = lambda t: torch.where(t.view(torch.int32) < 0, -(t.view(torch.int32) & 0x7fffffff), t.view(torch.int32)).long()  # noqa: E731
        ulps = (ordered(k_buf) - ordered(r_buf)).abs()
        rel = ((norm.stats - r_stats).abs() / r_stats.abs().clamp_min(1e-300)).max().item()
        agreement = {"max_ulp": int(ulps.max()), "differing": int((ulps != 0).sum()), "rel_stats": rel}

        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            reference()
        torch.cuda.current_stream(DEV).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            reference()

        def restart():                                         # (every window from a fresh state on the raw rewards: the
            norm.load_state_dict(fresh)                        # buffers are normalised in place, call after call)
            r_returns.copy_(fresh["returns"])
            r_stats.copy_(fresh["stats"])
            k_buf.copy_(raw)
            r_buf.copy_(raw)

        variants = {"kernel": kernel, "graph": graph.replay, "eager": reference, "gae": gae}

        def window(fn, n):
            restart()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(n):
                fn()
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) * 1e3 / n                 # us per call

        count = {}
        for name, fn in variants.items():                      # warm-up, and the window's length from it
            window(fn, 3)
            count[name] = max(3, int(args.window * 1e6 / window(fn, 5)) + 1)
        runs = {name: [] for name in variants}
        for _ in range(args.reps):
            for name, fn in variants.items():
                runs[name].append(window(fn, count[name]))
        rec = {"bench": "timing", "n_steps": T, "envs": E, "members": K, "reps": args.reps, **agreement,
               "pipeline_depth": int(g.native.lib().acas2d_reward_norm_pipeline_depth()),
               "workspace_bytes": int(g.native.lib().acas2d_reward_norm_workspace_bytes(E, T, K)),
               "device": torch.cuda.get_device_name(0),
               "method": "HIP events, windows of >= %.1f s, variants alternating, median of reps; us per call" % args.window}
        for name in variants:
            rec[name + "_us"] = float(np.median(runs[name]))
            rec[name + "_runs_us"] = runs[name]
            rec[name + "_spread"] = spread(runs[name])
            rec[name + "_calls_per_window"] = count[name]
        rec["graph_over_kernel"] = rec["graph_us"] / rec["kernel_us"]
        rec["eager_over_kernel"] = rec["eager_us"] / rec["kernel_us"]
        rec["kernel_over_gae"] = rec["kernel_us"] / rec["gae_us"]
        rec["beats_reference_beyond_spreads"] = bool(max(runs["kernel"]) < min(min(runs["graph"]), min(runs["eager"])))
        emit(rec)
        del graph
        torch.cuda.empty_cache()


def learn(args):
    E, N, cfg = 1024, 8, dict(n_steps=512, batch_size=4096)
    per_it = E * cfg["n_steps"]
    trainers = {}
    for name, rn in (("off", None), ("on", True)):
        venv = g.ACAS2DVecEnv(E, N, device=DEV, dtype=torch.float32, seed=13)
        tr = g.PPOTrainer(venv, g.PPOConfig(**cfg), collector="fused", updater="fused", gae="kernel", reward_norm=rn)
        tr.learn(2 * per_it, log=None)                         # capture + warm-up
        trainers[name] = tr
    runs = {name: [] for name in trainers}
    for _ in range(args.reps):
        for name, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.learn(tr.num_timesteps + args.iters * per_it, log=None)
            torch.cuda.synchronize()
            runs[name].append(args.iters * per_it / (time.perf_counter() - t0))
    rec = {"bench": "learn", "trainer": "PPOTrainer", "envs": E, "n_traffic": N, **cfg, "iters_per_run": args.iters,
           "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "method": "wall clock around learn() between device synchronisations, variants alternating, median of reps; "
                     "env steps per second"}
    for name in trainers:
        rec[name + "_env_steps_per_s"] = float(np.median(runs[name]))
        rec[name + "_runs"] = runs[name]
        rec[name + "_spread"] = spread(runs[name])
    rec["on_over_off"] = rec["on_env_steps_per_s"] / rec["off_env_steps_per_s"]
    rec["difference_exceeds_spreads"] = bool(max(runs["on"]) < min(runs["off"]) or min(runs["on"]) > max(runs["off"]))
    emit(rec)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--learn", action="store_true")
    ap.add_argument("--cases", default="512x1024x1,128x1024x1,512x4096x4")
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_reward_norm.py measures on the GPU"
    sink = open(args.out, "a") if args.out else None
    if args.timing:
        timing(args)
    if args.learn:
        learn(args)
