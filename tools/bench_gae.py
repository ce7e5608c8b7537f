#!/usr/bin/env python3
"""GAE as one hand-written launch (ppo.gae_fused: acas2d_gae_f32) beside torch's compute_gae, one JSON line per case.

  --timing   one GAE over [T][E] at --cases (default 512x1024, 128x1024, 512x8192) on random buffers with dones: the kernel,
             a replay of compute_gae captured in a hipGraph (what PPOTrainer replays) and compute_gae op by op (what
             PopulationTrainer runs).  HIP events around windows of >= --window seconds of back-to-back calls, every variant
             warmed up, the variants alternating in one process, median of --reps windows; `spread` is (max - min) / median
             of a variant's windows.  The three outputs are compared bit for bit before anything is timed.
  --learn    learn() env-steps/s with gae="kernel" against gae="torch", alternating, --reps timed runs of --iters
             iterations each: PPOTrainer at 1 024 x 8 traffic, 512 steps, minibatch 4 096; PPOTrainer at 1 024 x 16
             traffic, 128 steps, 4 epochs; PopulationTrainer K = 4 at 1 024 envs x 1 traffic per member, 512 steps.
             `gain_exceeds_spreads`: every "kernel" run beat every "torch" run.
usage: bench_gae.py --timing | --learn [--out profiles/gae_timing.jsonl]"""
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
        T, E = (int(x) for x in case.split("x"))
        gen = torch.Generator(device=DEV).manual_seed(T + E)
        rew = torch.randn(T, E, device=DEV, generator=gen)
        val = 50.0 * torch.randn(T, E, device=DEV, generator=gen)
        done = torch.rand(T, E, device=DEV, generator=gen) < 0.01
        last_value = 50.0 * torch.randn(E, device=DEV, generator=gen)
        gamma, lam = 0.99, 0.95
        const = g.gae_constants(gamma, lam, 1, torch.device(DEV))
        k_adv, k_ret = torch.empty_like(rew), torch.empty_like(rew)
        g_adv, g_ret = torch.empty_like(rew), torch.empty_like(rew)
        e_out = [None, None]

        def kernel():
            g.gae_fused(rew, val, done, last_value, constants=const, out={"adv": k_adv, "ret": k_ret})

        def body():                                            # PPOTrainer._gae without the forward
            adv, ret = g.compute_gae(rew, val, done, last_value, gamma, lam)
            g_adv.copy_(adv)
            g_ret.copy_(ret)

        def eager():
            e_out[0], e_out[1] = g.compute_gae(rew, val, done, last_value, gamma, lam)

        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            body()
        torch.cuda.current_stream(DEV).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            body()
        variants = {"kernel": kernel, "graph": graph.replay, "eager": eager}
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        same = all(torch.equal(a.view(torch.int32), b.view(torch.int32))
                   for a, b in ((k_adv, g_adv), (k_ret, g_ret), (k_adv, e_out[0]), (k_ret, e_out[1])))

        def window(fn, n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(n):
                fn()
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) * 1e3 / n                 # us per GAE

        count = {}
        for name, fn in variants.items():                      # warm-up, and the window's length from it
            window(fn, 5)
            count[name] = max(5, int(args.window * 1e6 / window(fn, 10)) + 1)
        runs = {name: [] for name in variants}
        for _ in range(args.reps):
            for name, fn in variants.items():
                runs[name].append(window(fn, count[name]))
        rec = {"bench": "timing", "n_steps": T, "envs": E, "reps": args.reps, "bitwise_equal": bool(same),
               "pipeline_depth": int(g.native.lib().acas2d_gae_pipeline_depth()),
               "bytes": 17 * T * E, "device": torch.cuda.get_device_name(0),
               "method": "HIP events, windows of >= %.1f s, variants alternating, median of reps; us per GAE" % args.window}
        for name in variants:
            rec[name + "_us"] = float(np.median(runs[name]))
            rec[name + "_runs_us"] = runs[name]
            rec[name + "_spread"] = spread(runs[name])
            rec[name + "_calls_per_window"] = count[name]
        rec["graph_over_kernel"] = rec["graph_us"] / rec["kernel_us"]
        rec["eager_over_kernel"] = rec["eager_us"] / rec["kernel_us"]
        emit(rec)
        del graph
        torch.cuda.empty_cache()


def learn(args):
    cases = (("PPOTrainer", 1, 1024, 8, dict(n_steps=512, batch_size=4096)),
             ("PPOTrainer", 1, 1024, 16, dict(n_steps=128, batch_size=4096, n_epochs=4)),
             ("PopulationTrainer", 4, 1024, 1, dict(n_steps=512, batch_size=4096)))
    for kind, K, E, N, cfg in cases:
        per_it = E * cfg["n_steps"]                            # one learner's env steps per iteration
        trainers = {}
        for gae in ("torch", "kernel"):
            venv = g.ACAS2DVecEnv(K * E, N, device=DEV, dtype=torch.float32, seed=13)
            if kind == "PPOTrainer":
                tr = g.PPOTrainer(venv, g.PPOConfig(**cfg), collector="fused", updater="fused", gae=gae)
            else:
                tr = g.PopulationTrainer(venv, [g.PPOConfig(seed=13 + k, **cfg) for k in range(K)], gae=gae)
            tr.learn(2 * per_it, log=None)                     # capture + warm-up
            trainers[gae] = tr
        runs = {gae: [] for gae in trainers}
        for _ in range(args.reps):
            for gae, tr in trainers.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tr.learn(tr.num_timesteps + args.iters * per_it, log=None)
                torch.cuda.synchronize()
                runs[gae].append(K * args.iters * per_it / (time.perf_counter() - t0))
        rec = {"bench": "learn", "trainer": kind, "members": K, "envs_per_member": E, "n_traffic": N, **cfg,
               "iters_per_run": args.iters, "reps": args.reps, "device": torch.cuda.get_device_name(0),
               "method": "wall clock around learn() between device synchronisations, variants alternating, median of reps; "
                         "aggregate env steps per second"}
        for gae in trainers:
            rec[gae + "_env_steps_per_s"] = float(np.median(runs[gae]))
            rec[gae + "_runs"] = runs[gae]
            rec[gae + "_spread"] = spread(runs[gae])
        rec["kernel_over_torch"] = rec["kernel_env_steps_per_s"] / rec["torch_env_steps_per_s"]
        rec["gain_exceeds_spreads"] = bool(min(runs["kernel"]) > max(runs["torch"]))
        emit(rec)
        del trainers
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--learn", action="store_true")
    ap.add_argument("--cases", default="512x1024,128x1024,512x8192")
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_gae.py measures on the GPU"
    sink = open(args.out, "a") if args.out else None
    if args.timing:
        timing(args)
    if args.learn:
        learn(args)
