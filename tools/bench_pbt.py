#!/usr/bin/env python3
"""The two launches of population-based training (csrc/acas2d_pbt.hip) beside a torch restatement, one JSON line per case.

  episodes   ppo.member_episodes (acas2d_member_episodes_f32) over a collection of K members x 1 024 envs x 512 steps,
             about 1 % of the entries done, against masked sums in torch (torch.where + sum over a [T, K, EM] view, five of
             them, no read-back).
  exploit    ppo.population_exploit (acas2d_population_exploit_f32) with n_replace = K // 4 at obs_dim D, against what a host
             does without it: read the scores back, rank and draw in Python (tests/pbt_ref.py), one index_copy_ per
             parameter stack and Adam buffer, and a rewrite of the hyper rows.
K in {4, 16}, D in {8, 197}.  Both variants run in one process and alternate; HIP events around windows of >= --window
seconds of back-to-back calls, every variant warmed up, median of --reps windows, `spread` = (max - min) / median.  The two
variants' results are compared before anything is timed (the exploit bit for bit; the episode integers exactly, the return
sums to 1e-12 relative: the orders of summation differ).  There is no pass mark: the launches' claim is "no host decision,
two launches", not a ratio.
usage: bench_pbt.py [--out profiles/pbt_timing.jsonl]"""
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
import pbt_ref as R  # noqa: E402

DEV = "cuda:0"
sink = None


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if sink:
        sink.write(line + "\n")
        sink.flush()


def measure(variants, args):
    def window(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / n                     # us per call

    count = {}
    for name, fn in variants.items():                          # warm-up, and the window's length from it
        window(fn, 3)
        count[name] = max(3, int(args.window * 1e6 / window(fn, 5)) + 1)
    runs = {name: [] for name in variants}
    for _ in range(args.reps):
        for name, fn in variants.items():
            runs[name].append(window(fn, count[name]))
    out = {}
    for name in variants:
        out[name + "_us"] = float(np.median(runs[name]))
        out[name + "_runs_us"] = runs[name]
        out[name + "_spread"] = (max(runs[name]) - min(runs[name])) / float(np.median(runs[name]))
        out[name + "_calls_per_window"] = count[name]
    return out


def episodes(K, args):
    T, EM = 512, 1024
    E = K * EM
    gen = torch.Generator(device=DEV).manual_seed(K)
    done = torch.rand(T, E, device=DEV, generator=gen) < 0.01
    outcome = torch.randint(0, 4, (T, E), device=DEV, generator=gen, dtype=torch.uint8)
    epret = 1e3 * torch.randn(T, E, device=DEV, generator=gen)
    eplen = torch.randint(2, 1002, (T, E), device=DEV, generator=gen, dtype=torch.int32)
    acc = g.member_episodes(done, outcome, epret, eplen, K)
    t_out = {}

    def kernel():
        g.member_episodes(done, outcome, epret, eplen, K, acc=acc)

    def torch_masked():
        d = done.view(T, K, EM)
        t_out["count"] = d.sum((0, 2))
        t_out["return_sum"] = torch.where(d, epret.view(T, K, EM).double(), 0.0).sum((0, 2))
        t_out["steps"] = torch.where(d, eplen.view(T, K, EM).long() - 1, 0).sum((0, 2))
        o = outcome.view(T, K, EM)
        t_out["outcomes"] = torch.stack([(d & (o == c)).sum((0, 2)) for c in range(4)], 1)
        t_out["score"] = (t_out["return_sum"] / t_out["count"]).float()

    torch_masked()
    torch.cuda.synchronize()
    same = all(torch.equal(acc[n], t_out[n]) for n in ("count", "steps", "outcomes")) and \
        bool(((acc["return_sum"] - t_out["return_sum"]).abs() <= 1e-12 * t_out["return_sum"].abs()).all())
    rec = {"bench": "episodes", "members": K, "n_steps": T, "envs_per_member": EM, "done_share": 0.01, "equal": bool(same),
           "device": torch.cuda.get_device_name(0),
           "method": "HIP events, windows of >= %.1f s, variants alternating, median of reps; us per call" % args.window}
    rec.update(measure({"kernel": kernel, "torch": torch_masked}, args))
    rec["torch_over_kernel"] = rec["torch_us"] / rec["kernel_us"]
    emit(rec)


def exploit(K, D, args):
    Rn = K // 4
    dev = torch.device(DEV)
    gen = torch.Generator(device=DEV).manual_seed(K + D)
    cfgs = [g.PPOConfig(seed=13 + k, learning_rate=1e-4 * (1 + k)) for k in range(K)]
    rollout = [torch.zeros(2, D, device=dev)] + [torch.zeros(2, device=dev) for _ in range(4)]

    def population():
        ps = g.ActorCriticSet(K, D, dev)
        for p in ps.params.values():
            p.copy_(torch.randn(p.shape, device=dev, generator=torch.Generator(device=DEV).manual_seed(D)))
        fu = g.FusedUpdateSet(ps, cfgs, *rollout)
        fu.m.copy_(torch.randn(fu.m.shape, device=dev, generator=torch.Generator(device=DEV).manual_seed(1)))
        fu.v.copy_(torch.rand(fu.v.shape, device=dev, generator=torch.Generator(device=DEV).manual_seed(2)))
        fu.step_count.copy_(torch.arange(K, device=dev, dtype=torch.int32))
        return ps, fu

    (ps_k, fu_k), (ps_t, fu_t) = population(), population()
    score = torch.randn(K, device=dev, generator=gen)
    pbt = g.PBTConfig(ready_every=1)
    mask, lo, hi = 0, np.full(8, -np.inf, np.float32), np.full(8, np.inf, np.float32)
    for name in pbt.perturb:
        s = R.HYPER_SLOTS.index(name)
        mask |= 1 << s
        lo[s], hi[s] = pbt.bounds[name]
    hyper0 = fu_t.hyper.cpu().numpy().copy()                   # donors are never written: every call does the same work

    def kernel():
        g.population_exploit(ps_k, fu_k, score, Rn, 0, 7)

    def torch_host():
        donor, hyper = R.exploit(score.cpu().numpy(), hyper0, Rn, 0, 7, mask, 0.8, 1.2, lo, hi)       # read-back + ranking
        dst = np.nonzero(donor != np.arange(K))[0]
        dst_d, src_d = torch.as_tensor(dst, device=dev), torch.as_tensor(donor[dst].astype(np.int64), device=dev)
        for t in list(ps_t.params.values()) + [fu_t.m, fu_t.v, fu_t.step_count]:
            t.index_copy_(0, dst_d, t.index_select(0, src_d))
        fu_t.hyper.copy_(torch.as_tensor(hyper))

    kernel()
    torch_host()
    torch.cuda.synchronize()
    bits = lambda t: t.contiguous().view(torch.uint8)  # noqa: E731
    same = all(torch.equal(bits(a), bits(b)) for a, b in
               list(zip(ps_k.params.values(), ps_t.params.values())) +
               [(fu_k.m, fu_t.m), (fu_k.v, fu_t.v), (fu_k.step_count, fu_t.step_count), (fu_k.hyper, fu_t.hyper)])
    n = int(g.native.lib().acas2d_ppo_workspace_floats(D))
    rec = {"bench": "exploit", "members": K, "obs_dim": D, "n_replace": Rn, "bytes_copied": Rn * (3 * n - 2) * 4 + Rn * 36,
           "bitwise_equal": bool(same), "device": torch.cuda.get_device_name(0),
           "method": "HIP events, windows of >= %.1f s, variants alternating, median of reps; us per call" % args.window}
    rec.update(measure({"kernel": kernel, "torch": torch_host}, args))
    rec["torch_over_kernel"] = rec["torch_us"] / rec["kernel_us"]
    emit(rec)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--widths", type=int, nargs="+", default=[8, 197])
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pbt.py measures on the GPU"
    sink = open(args.out, "a") if args.out else None
    for K in args.members:
        episodes(K, args)
    for K in args.members:
        for D in args.widths:
            exploit(K, D, args)
