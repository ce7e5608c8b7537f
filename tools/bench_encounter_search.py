#!/usr/bin/env python3
"""An encounter search's launches (policy.EncounterSearch: acas2d_encounter_*) beside the only way to the same result
without them, one JSON line per case.  A case is CANDIDATESxGENERATIONSxN_TRAFFICxK (default 65536x8x1x1, 65536x8x1x8,
65536x8x8x1, 65536x8x8x8), float32, K randomly initialised policies, 8 bins, rho 0.1, alpha 0.7:

  (a) search     EncounterSearch.run(GENERATIONS), wall clock between device synchronisations (the object is built before)
  (b) host_loop  per generation and policy: records.search_sample() on uniforms drawn beforehand (a NumPy Philox, not timed),
                 records.encounter_from_uniforms(), evaluate_policies_fused(safety=True) -- which stages the states through
                 set_state -- records.search_select() and records.search_refit(); wall clock likewise
  (c) launches   HIP events around each of (a)'s launches of one generation: sample, evaluate, select, refit; summed over the
                 generations, and the three new ones as a share of the evaluation

(a) and (b) run with weighted=False: every elite weight is 1, every sum exact, so the two compute the same bits and their
buffers are compared for equality before anything is timed.  (c) runs with the default weighted=True (the select launch then
takes the exponentials).  One warm-up of every variant, then --reps repetitions, the variants alternating in one process; the
median and min - max are printed, `spread` is (max - min) / median.

--finding: what a search finds for the committed reference policy (tests/golden/ref_policy_best_model.npz) and the all-zero
policy at 1 aircraft, 65 536 candidates x 8 generations, beside a MonteCarlo campaign of the same number of episodes; measured
once, one JSON line.
usage: bench_encounter_search.py [--cases ...] [--reps 5] [--finding] [--out profiles/encounter_search_timing.jsonl]"""
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
SEED = 13
LAUNCHES = ("sample", "evaluate", "select", "refit")


def policies(N, K):
    out = []
    for seed in range(K):
        torch.manual_seed(seed + 1)
        pol = g.ActorCritic(5 + 3 * N)
        with torch.no_grad():
            pol.action_net.weight.mul_(40.0)
        out.append(pol)
    return out


def philox_uniforms(seed, lanes, generation, n_entities, rounds=7):
    """u [lanes, 4 n_entities]: the reset stream's philox4x32 on counter (lane, 0, generation, entity), key = seed, as
    (w + 0.5) 2^-32 -- what the sampler draws, in NumPy."""
    m32 = np.uint64(0xFFFFFFFF)
    lane = np.repeat(np.arange(lanes, dtype=np.uint64), n_entities)
    c0, c1 = lane & m32, lane >> np.uint64(32)
    c2 = np.full_like(c0, generation)
    c3 = np.tile(np.arange(n_entities, dtype=np.uint64), lanes)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    for _ in range(rounds):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    w = np.stack([c0, c1, c2, c3], axis=1).astype(np.float64)
    return ((w + 0.5) / 4294967296.0).reshape(lanes, 4 * n_entities)


def spread(runs):
    return (max(runs) - min(runs)) / float(np.median(runs))


def make(pols, L, N, **kw):
    return g.EncounterSearch(pols, L, seed=SEED, n_traffic=N, device=DEV, **kw)


def host_loop(pols, cfg, u, L, es):
    """(b): returns the final proposals [K, n_coord, B] and the log rows [G, K, 12]."""
    R = g.records
    active = R.search_active_coordinates(cfg)
    K = len(pols)
    p = np.full((K, 4 * (cfg.n_traffic + 1), es.n_bins), 1.0 / es.n_bins)
    rows = []
    for gen in range(len(u)):
        cdf, lr = R.search_tables(p)
        row = []
        for k in range(K):
            c, bins, log_w = R.search_sample((p[k], cdf[k], lr[k]), active, u[gen])
            own, trf, goal = R.encounter_from_uniforms(cfg, c, np.float32)
            res = g.evaluate_policies_fused([pols[k]], own, trf, goal, dtype=torch.float32, device=DEV, config=cfg, safety=True)
            sel = R.search_select(res["min_separation"][0], res["outcome"][0], log_w, es.n_quantile, es.level, False)
            p[k] = R.search_refit(p[k], active, bins, sel["elite_w"], es.alpha, es.p_floor)
            row.append(sel["row"][:12])
        rows.append(row)
    return p, np.array(rows)


def case(L, G, N, K, reps):
    pols = policies(N, K)
    cfg = g.ACAS2DConfig(n_traffic=N)
    u = [philox_uniforms(SEED, L, gen, N + 1) for gen in range(G)]

    def search():
        es = make(pols, L, N, weighted=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        es.run(G)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, es

    def loop():
        es = make(pols, L, N, weighted=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = host_loop(pols, cfg, u, L, es)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def launches():
        es = make(pols, L, N)
        total = dict.fromkeys(LAUNCHES, 0.0)
        for _ in range(G):
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in LAUNCHES]
            torch.cuda.synchronize()
            es._generation(events=ev)
            torch.cuda.synchronize()
            for name, (a, b) in zip(LAUNCHES, ev):
                total[name] += a.elapsed_time(b) * 1e-3
        return total

    _, es = search()                                           # warm-up, and the agreement
    _, (p_ref, rows_ref) = loop()
    agree = bool(np.array_equal(es.proposal().view(np.uint64), p_ref.view(np.uint64)) and
                 np.array_equal(es.history()[:, :, :12].view(np.uint64), rows_ref.view(np.uint64)))
    launches()
    runs = {"search": [], "host_loop": []}
    per = {name: [] for name in LAUNCHES}
    for _ in range(reps):
        runs["search"].append(search()[0])
        runs["host_loop"].append(loop()[0])
        for name, t in launches().items():
            per[name].append(t)
    rec = {"bench": "encounter_search", "candidates": L, "generations": G, "n_traffic": N, "policies": K, "dtype": "float32",
           "n_bins": es.n_bins, "n_quantile": es.n_quantile, "reps": reps, "bit_equal_to_host_loop": agree,
           "device": torch.cuda.get_device_name(0),
           "method": "one warm-up, variants alternating, median of reps; search / host_loop: wall clock between synchronisations, "
                     "weighted=False; launches: HIP events around the C calls of every generation, summed, weighted=True; seconds"}
    for name, r in list(runs.items()) + [("launch_" + k, v) for k, v in per.items()]:
        rec[name + "_s"] = float(np.median(r))
        rec[name + "_runs_s"] = r
        rec[name + "_spread"] = spread(r)
        print("  %-16s median %.5f s   min %.5f   max %.5f" % (name, np.median(r), min(r), max(r)), flush=True)
    new = [sum(per[k][i] for k in ("sample", "select", "refit")) / per["evaluate"][i] for i in range(reps)]
    rec["search_over_host_loop"] = rec["search_s"] / rec["host_loop_s"]
    rec["search_below_host_loop_beyond_spreads"] = bool(max(runs["search"]) < min(runs["host_loop"]))
    rec["new_launches_over_evaluate"] = float(np.median(new))
    rec["new_launches_over_evaluate_runs"] = new
    return rec


def finding(L=65536, G=8):
    ref = os.path.join(ROOT, "tests", "golden", "ref_policy_best_model.npz")
    zero = tuple(torch.zeros(*s) for s in ((64, 8), (64,), (64, 64), (64,), (1, 64), (1,)))
    pols = [g.load_sb3_policy(ref), zero]
    es = make(pols, L, 1).run(G)
    h, est, best = es.history(), es.estimate(), es.best()
    mc = g.MonteCarlo(pols, L, seed=SEED, n_traffic=1, device=DEV).run(G)
    s = mc.summary()
    edge = es.level * mc.inv_bin_width                       # (96 x 64 / 768 = 8: a bin edge lies on the level)
    assert edge == int(edge)
    below = mc.accumulators()["sep_hist"][:, :int(edge)].sum(1)
    lo, hi = g.records.wilson_interval(below, L * G)
    first = [int(np.argmax(h[:, k, 5] > 0)) if (h[:, k, 5] > 0).any() else None for k in range(2)]
    return {"bench": "encounter_search_finding", "policies": ["ref_policy_best_model", "zero"], "candidates": L, "generations": G,
            "n_traffic": 1, "dtype": "float32", "level": es.level, "episodes": L * G,
            "estimate": [float(x) for x in est["p"]], "estimate_se": [float(x) for x in est["se"]],
            "estimate_per_generation": est["p_generation"].T.tolist(), "ess_per_generation": est["ess"].T.tolist(),
            "n_event_per_generation": h[:, :, 5].T.tolist(), "gamma_per_generation": h[:, :, 4].T.tolist(),
            "first_generation_with_an_event": first,
            "closest": [None if b is None else {"generation": b[0], "candidate": b[1], "min_separation": float(b[2])} for b in best],
            "monte_carlo_below_level": [int(x) for x in below], "monte_carlo_below_level_rate": [float(x) / (L * G) for x in below],
            "monte_carlo_below_level_wilson_95": [[float(a), float(b)] for a, b in zip(lo, hi)],
            "monte_carlo_collisions": [int(x) for x in s["collisions"]],
            "monte_carlo_collision_rate": [float(x) for x in s["collision_rate"]],
            "monte_carlo_wilson_95": [[float(a), float(b)] for a, b in zip(s["collision_rate_lo"], s["collision_rate_hi"])],
            "device": torch.cuda.get_device_name(0), "method": "measured once; the event is min_separation <= level"}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="65536x8x1x1,65536x8x1x8,65536x8x8x1,65536x8x8x8")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--finding", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_encounter_search.py measures on the GPU"
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    for c in [x for x in args.cases.split(",") if x]:
        L, G, N, K = (int(x) for x in c.split("x"))
        print("case %s" % c, flush=True)
        emit(case(L, G, N, K, args.reps))
    if args.finding:
        emit(finding())
