"""Monte Carlo campaigns, host side (no GPU): the NumPy reducers of records.py that specify the accumulators of
acas2d_monte_carlo_* -- separation_bin(), monte_carlo_reduce(), monte_carlo_summary() -- against numbers written out
here, the three entry points in the header, the loader and the built library, and their argument validation (every
pointer below is a host address: the calls are refused before any launch)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import scoring_rejections_support as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("acas2d_monte_carlo_f32", "acas2d_monte_carlo_f64", "acas2d_monte_carlo_group_f32")


@pytest.fixture(scope="module")
def g():
    import gym_acas2d_amd as g
    return g


# ---- separation_bin ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_separation_bin_edges(g, dtype):
    """16 bins of 48 (hist_max = 768 = 4 x the safe distance): 0, just below / on / just above an edge, the last bin's
    lower edge, hist_max and beyond, inf, NaN.  1 / 48 is no binary fraction, so the products are rounded in `dtype`:
    the expected bins below are those of the rounded product, worked out per format."""
    sb = g.records.separation_bin
    inv = 16.0 / 768.0
    dt = dtype
    below, above = np.nextafter(dt(96), dt(0)), np.nextafter(dt(96), dt(1000))
    # 96 x fl(1 / 48), exactly (rational arithmetic) and then rounded to the format:
    #   float32  fl(1/48) > 1/48: 96 -> 2 + 6.0e-8 -> 2.0 (bin 2); its lower neighbour 95.99999 -> 2 - 9.9e-8 -> 1.9999999 (bin 1)
    #   float64  fl(1/48) < 1/48: 96 -> 2 - 1.1e-16 -> 2.0 after rounding (bin 2, although the exact product lies below
    #            the edge); its lower neighbour -> 2 - 4.1e-16 -> 1.9999999999999996 (bin 1)
    want_below = 1
    vals = [0.0, below, 96.0, above, 720.0, 767.9, 768.0, 5000.0, np.inf, -np.inf, np.nan, 47.0, 48.5]
    want = [0, want_below, 2, 2, 15, 15, 15, 15, 15, 15, 15, 0, 1]
    got = sb(np.array(vals, dtype), 16, inv, dtype)
    assert got.dtype == np.int64 and got.tolist() == want
    for v, w in zip(vals, want):                                          # scalars too
        assert int(sb(v, 16, inv, dtype)) == w
    # an exact bin width: every edge belongs to the bin above it
    assert sb(np.array([127.99, 128.0, 128.01, 511.9, 512.0], dtype), 4, 1.0 / 128.0, dtype).tolist() == [0, 1, 1, 3, 3]
    assert sb(np.array([3.0e38, 1.0e30], dtype), 4, 1.0e9, dtype).tolist() == [3, 3]       # the product overflows / is huge
    assert sb(np.array([5.0, np.nan], dtype), 1, 1.0, dtype).tolist() == [0, 0]            # one bin takes everything


# ---- the GPU tests' support: wide keys and the rounding edge ------------------------------------------------------------------
def test_wide_keys_cross_2_to_the_32_where_the_gpu_tests_claim():
    """monte_carlo_support.WIDE_*: the seed's halves are non-zero and distinct; the launch's last counter is 2^32 - 1; the
    lane crosses 2^32 at local lane 37, strictly inside the 70 lanes / episodes / envs, and that lane is neither the first
    nor the last env of its wave at 64, 32, 16, 8 or 4 envs per wave -- so at every shape the campaigns, evaluators and
    collectors run at those keys."""
    import eval_stats_support as ES
    import helpers as H
    import monte_carlo_support as MS
    import noise_scoring_support as NS
    import test_collect_disturbed as CD
    import test_monte_carlo as TM
    lo, hi = MS.WIDE_SEED & 0xFFFFFFFF, MS.WIDE_SEED >> 32
    assert MS.WIDE_SEED == H.WIDE_SEED and 0 < lo != hi > 0 and hi < 2 ** 32
    assert MS.WIDE_FIRST_EPISODE + MS.EPISODES - 1 == 2 ** 32 - 1 == NS.WIDE_NOISE_EPISODE
    c = MS.WIDE_CROSSING
    assert MS.WIDE_LANE_OFFSET + c == 2 ** 32 and (MS.WIDE_LANE_OFFSET + c - 1) >> 32 == 0
    assert 0 < c < min(MS.LANES, ES.E, CD.E1) - 1
    assert MS.TRUNCATED["env_offset"] == (MS.WIDE_LANE_OFFSET + c) & 0xFFFFFFFF == 0          # lane 37's low word: lane 0 of offset 0
    shapes = ([(s.N, s.group) for s in TM.WIDE_SHAPES + NS.WIDE_CAMPAIGN_SHAPES] + list(NS.WIDE_EVAL_SHAPES) + list(CD.WIDE_SHAPES))
    assert {(1, False), (8, False), (16, True)} == set(shapes)
    for N, group in shapes:
        wave = MS.envs_per_wave((N, group))
        if group:                                             # the table of work shapes has it: (4, N / 4), the default choice at N
            assert any(s.dtype == "float32" and s.n_traffic == N and s.override is None and (s.C, s.G) == (4, N // 4) and
                       s.envs_per_wave == wave for s in H.SHAPES), (N, group)
        assert 0 < c % wave < wave - 1, (N, group, wave)
    for wave in (64, 32, 16, 8, 4):
        assert 0 < c % wave < wave - 1, wave


# (format, min_sep, the hist_max found, the bin edge the rounded product lands on)
EDGES = ((np.float32, 137.25, 2196.0000135493465, 1), (np.float32, 201.7, 1075.7333425837921, 3), (np.float32, 58.9, 104.71111691895858, 9),
         (np.float64, 137.25, 2196.0, 1), (np.float64, 333.3333, 1777.7776000000001, 3), (np.float64, 58.9, 188.48000000000002, 5))


@pytest.mark.parametrize("dtype,min_sep,want,edge", EDGES, ids=["%s-%r" % (np.dtype(e[0]).name, e[1]) for e in EDGES])
def test_edge_hist_max_meets_its_three_conditions(g, dtype, min_sep, want, edge):
    """monte_carlo_support.edge_hist_max() on written-out values: the double it returns, and -- in rational arithmetic, not
    through the function's own expressions -- that the kernel's inverse width is dtype(16 / hist_max), that min_sep lies
    inside the histogram, and that the product is `edge` exactly once rounded to the format while the exact one is below."""
    import fractions

    import monte_carlo_support as MS
    F = fractions.Fraction
    m = dtype(min_sep)
    hist_max = MS.edge_hist_max(m, 16, dtype)
    assert isinstance(hist_max, float) and hist_max == want
    inv = dtype(16 / hist_max)                                   # what policy.MonteCarlo hands the kernel, rounded as it reads it
    exact = F(float(m)) * F(float(inv))
    assert float(m) < hist_max
    assert exact < edge and float(dtype(m * inv)) == float(edge)
    # the format's rounding of the exact product, worked out here: the distance to the edge is at most half a unit in the
    # last place below it (units below a power of two are half those above; `edge` may be one)
    bits = 24 if dtype == np.float32 else 53
    ulp_below = F(2) ** (math.floor(math.log2(edge - 0.5 if edge > 1 else 0.75)) - bits + 1)
    assert 0 < edge - exact <= ulp_below / 2
    # ... so the bins differ: the kernel's rule says `edge`, exact arithmetic the bin below
    assert int(g.records.separation_bin(m, 16, 16 / hist_max, dtype)) == edge
    assert int(MS.exact_bins(m, 16, 16 / hist_max, dtype)) == edge - 1


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_edge_hist_max_raises_where_there_is_no_edge(dtype):
    """A power of two times an inverse width is exact: no rounding, no such width -- an error, never a fallback."""
    import monte_carlo_support as MS
    with pytest.raises(ValueError, match="no bin width"):
        MS.edge_hist_max(dtype(128.0), 16, dtype)


# ---- monte_carlo_reduce -----------------------------------------------------------------------------------------------------
INF = np.inf
# [counter][policy][lane]; 4 bins of 128 (inv_bin_width = 1 / 128, exact)
OUTCOME = [[[1, 2, 3, 1, 1], [1, 1, 1, 2, 3]], [[2, 1, 1, 1, 3], [1, 1, 2, 1, 1]], [[1, 1, 1, 1, 1], [3, 1, 1, 1, 2]]]
STEPS = [[[10, 5, 100, 20, 30], [11, 12, 13, 4, 100]], [[6, 10, 10, 10, 100], [10, 10, 7, 10, 10]],
         [[10, 10, 10, 10, 10], [100, 10, 10, 10, 3]]]
RETURN = [[[1.5, -2.0, 0.25, 3.0, 0.5], [1.0, 2.0, 3.0, -4.0, 0.5]], [[-1.0, 1.0, 0.5, 0.5, 0.0], [1.0, 1.0, -3.0, 1.0, 1.0]],
          [[0.25, 0.25, 0.25, 0.25, 0.25], [0.0, 1.0, 1.0, 1.0, -5.0]]]
MIN_SEP = [[[250, 90, 300, 150, 500], [250, 150, 350, 80, INF]], [[95, 90, 310, 100, 500], [250, 120, 85, 80, 200]],
           [[240, 300, 100, 150, 450], [400, 110, 85, 300, 70]]]
LOS = [[[0, 3, 0, 2, 0], [0, 1, 0, 4, 0]], [[5, 2, 0, 1, 0], [0, 2, 6, 3, 0]], [[0, 0, 1, 1, 0], [0, 1, 2, 0, 3]]]
WANT = {"outcome_count": [[0, 11, 2, 2], [0, 10, 3, 2]], "sum_steps": [351, 320], "los_episodes": [7, 8],
        "sum_los_steps": [15, 22], "sep_hist": [[5, 4, 3, 3], [7, 4, 2, 2]],
        "lane_return_sum": [[0.75, -0.75, 1.0, 3.75, 0.75], [2.0, 4.0, 1.0, -2.0, -3.5]],
        "lane_return_sq": [[3.3125, 5.0625, 0.375, 9.3125, 0.3125], [2.0, 6.0, 19.0, 18.0, 26.25]],
        # lane 1 of policy 0 (90 at counters 0 and 1), lanes 0, 2, 3 of policy 1: a tie keeps the FIRST counter
        "lane_worst_sep": [[95, 90, 100, 100, 450], [250, 110, 85, 80, 70]],
        "lane_worst_episode": [[1, 0, 2, 1, 2], [0, 2, 1, 0, 2]]}


def _results(dtype, counters=(0, 1, 2)):
    return [{"outcome": np.array(OUTCOME[c], np.uint8), "steps": np.array(STEPS[c], np.int32),
             "total_reward": np.array(RETURN[c], np.float64), "min_separation": np.array(MIN_SEP[c], dtype),
             "los_steps": np.array(LOS[c], np.int32)} for c in counters]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_monte_carlo_reduce_against_written_out_numbers(g, dtype):
    r = g.records
    acc = r.monte_carlo_reduce(_results(dtype), 4, 1.0 / 128.0, dtype)
    assert tuple(acc) == r.MONTE_CARLO_KEYS
    for k in r.MONTE_CARLO_INT_KEYS:
        assert acc[k].dtype == np.int64 and acc[k].tolist() == WANT[k], k
    assert acc["lane_return_sum"].dtype == acc["lane_return_sq"].dtype == np.float64
    assert acc["lane_worst_sep"].dtype == dtype and acc["lane_worst_episode"].dtype == np.uint32
    for k in r.MONTE_CARLO_LANE_KEYS:
        assert acc[k].tolist() == WANT[k], k
    assert acc["outcome_count"].sum(1).tolist() == acc["sep_hist"].sum(1).tolist() == [15, 15]
    # chaining: [0, 1] and then [2] is [0, 1, 2], bit for bit; the inputs are left alone
    first = r.monte_carlo_reduce(_results(dtype, (0, 1)), 4, 1.0 / 128.0, dtype)
    keep = {k: v.copy() for k, v in first.items()}
    both = r.monte_carlo_reduce(_results(dtype, (2,)), 4, 1.0 / 128.0, dtype, acc=first, first_episode=2)
    for k in r.MONTE_CARLO_KEYS:
        assert _same_bits(both[k], acc[k]), k
        assert _same_bits(first[k], keep[k]), k
    # first_episode names the counters; a lane that never beat +inf keeps counter 0
    late = r.monte_carlo_reduce(_results(dtype, (0,)), 4, 1.0 / 128.0, dtype, first_episode=7)
    assert late["lane_worst_episode"].tolist() == [[7] * 5, [7, 7, 7, 7, 0]] and late["lane_worst_sep"][1, 4] == np.inf
    with pytest.raises(ValueError):
        r.monte_carlo_reduce([], 4, 1.0 / 128.0, dtype)


def test_monte_carlo_reduce_adds_the_returns_in_counter_order(g):
    """float64 adds do not commute with regrouping: 1e16 + 1 + 1 is 1e16 counter by counter, 1e16 + 2 otherwise."""
    def one(ret):
        return {"outcome": np.array([[1]], np.uint8), "steps": np.array([[2]], np.int32), "total_reward": np.array([[ret]]),
                "min_separation": np.array([[300.0]]), "los_steps": np.array([[0]], np.int32)}
    acc = g.records.monte_carlo_reduce([one(1e16), one(1.0), one(1.0)], 4, 1.0 / 128.0)
    assert acc["lane_return_sum"][0, 0] == 1e16 and acc["lane_return_sum"][0, 0] != 1e16 + 2.0
    # a float32 launch's return enters as the float64 value of the float32 number
    acc = g.records.monte_carlo_reduce([one(0.1)], 4, 1.0 / 128.0, np.float32)
    assert acc["lane_return_sum"][0, 0] == float(np.float32(0.1)) and acc["lane_return_sq"][0, 0] == float(np.float32(0.1)) ** 2


# ---- monte_carlo_summary ----------------------------------------------------------------------------------------------------
def _acc(g, counts, lane_sum, lane_sq):
    K = len(counts)
    acc = g.records.monte_carlo_empty(K, len(lane_sum[0]), 4)
    acc["outcome_count"][:] = counts
    acc["lane_return_sum"][:] = lane_sum
    acc["lane_return_sq"][:] = lane_sq
    acc["sum_steps"][:] = [70000, 50000, 1000][:K]
    acc["los_episodes"][:] = [25, 5, 0][:K]
    acc["sum_los_steps"][:] = [400, 30, 0][:K]
    acc["sep_hist"][:] = [[10, 15, 25, 50], [5, 0, 45, 50], [0, 0, 0, 100]][:K]
    return acc


def test_monte_carlo_summary_by_hand(g):
    acc = _acc(g, [[0, 88, 10, 2], [0, 95, 5, 0]], [[30.0, 20.0], [60.0, 40.0]], [[500.0, 400.0], [80.0, 70.0]])
    s = g.records.monte_carlo_summary(acc, baseline=0, hist_max=512.0)
    assert s["episodes"].tolist() == [100, 100] and s["goals"].tolist() == [88, 95]
    assert s["collisions"].tolist() == [10, 5] and s["timeouts"].tolist() == [2, 0]
    assert s["goal_rate"].tolist() == [0.88, 0.95] and s["collision_rate"].tolist() == [0.1, 0.05]
    assert s["timeout_rate"].tolist() == [0.02, 0.0] and s["los_rate"].tolist() == [0.25, 0.05]
    assert s["mean_steps"].tolist() == [700.0, 500.0] and s["mean_los_steps"].tolist() == [4.0, 0.3]
    # Wilson, 10 of 100 at z = 1.959964: centre (p + z^2 / 2n) / (1 + z^2 / n), half width z sqrt(p q / n + z^2 / 4n^2) / (1 + z^2 / n)
    z, n, p = 1.959963984540054, 100.0, 0.1
    den = 1.0 + z * z / n
    mid, half = (p + z * z / (2 * n)) / den, z * math.sqrt(p * (1 - p) / n + z * z / (4 * n * n)) / den
    assert s["collision_rate_lo"][0] == pytest.approx(mid - half, rel=1e-12)
    assert s["collision_rate_hi"][0] == pytest.approx(mid + half, rel=1e-12)
    assert abs(s["collision_rate_lo"][0] - 0.05523) < 1e-5 and abs(s["collision_rate_hi"][0] - 0.17437) < 1e-5   # the tables' values
    assert abs(s["collision_rate_lo"][1] - 0.02154) < 2e-5 and abs(s["collision_rate_hi"][1] - 0.11175) < 1e-5   # 5 of 100
    assert s["risk_ratio"].tolist() == [1.0, 0.5]
    # mean 50 / 100; variance (900 / 100 - 0.25) x 100 / 99; standard error sqrt(variance / 100)
    assert s["mean_return"].tolist() == [0.5, 1.0]
    assert s["return_sem"][0] == pytest.approx(math.sqrt((9.0 - 0.25) * 100.0 / 99.0 / 100.0), rel=1e-12)
    assert s["return_sem"][1] == pytest.approx(math.sqrt((1.5 - 1.0) * 100.0 / 99.0 / 100.0), rel=1e-12)
    assert s["sep_hist"].tolist() == [[10, 15, 25, 50], [5, 0, 45, 50]] and s["hist_edges"].tolist() == [0, 128, 256, 384, 512]
    assert g.records.monte_carlo_summary(acc, baseline=1)["risk_ratio"].tolist() == [2.0, 1.0]
    assert "risk_ratio" not in g.records.monte_carlo_summary(acc)


def test_monte_carlo_summary_without_collisions_in_the_baseline(g):
    """inf against a baseline that never collided, nan for a policy that did not either (0 / 0); an empty campaign is
    nan throughout -- no exception, no warning turned into one."""
    acc = _acc(g, [[0, 100, 0, 0], [0, 95, 5, 0], [0, 50, 0, 50]], [[1.0, 1.0]] * 3, [[1.0, 1.0]] * 3)
    with np.errstate(all="raise"):
        s = g.records.monte_carlo_summary(acc, baseline=0)
    assert math.isnan(s["risk_ratio"][0]) and s["risk_ratio"][1] == np.inf and math.isnan(s["risk_ratio"][2])
    assert s["collision_rate_lo"][0] == pytest.approx(0.0, abs=1e-15) and 0.03 < s["collision_rate_hi"][0] < 0.04
    with np.errstate(all="raise"):
        e = g.records.monte_carlo_summary(g.records.monte_carlo_empty(2, 3, 4), baseline=1)
    assert e["episodes"].tolist() == [0, 0] and np.isnan(e["collision_rate"]).all() and np.isnan(e["risk_ratio"]).all()
    assert np.isnan(e["mean_return"]).all()


def test_summary_sums_the_lanes_in_order(g):
    acc = g.records.monte_carlo_empty(1, 3, 4)
    acc["outcome_count"][0] = [0, 3, 0, 0]
    acc["lane_return_sum"][0] = [1e16, 1.0, 1.0]                        # lane after lane: 1e16; pairwise would give 1e16 + 2
    assert g.records.monte_carlo_summary(acc)["mean_return"][0] == 1e16 / 3.0


# ---- header, loader, library ------------------------------------------------------------------------------------------------
def test_entries_in_header_loader_and_library(g):
    with open(os.path.join(ROOT, "include", "acas2d.h")) as f:
        header = f.read()
    L = g.native.lib()
    for name in ENTRIES + ("acas2d_monte_carlo_size",):
        assert (" %s(" % name) in header and name in g.native.EXPORTS and hasattr(L, name), name
    assert "typedef struct Acas2dMonteCarlo {" in header and "#define ACAS2D_ABI_VERSION 7" in header
    assert L.acas2d_abi_version() == g.native.ABI_VERSION == 7
    assert C.sizeof(g.native.CMonteCarlo) == L.acas2d_monte_carlo_size() == 96
    fields = [n for n, _ in g.native.CMonteCarlo._fields_]
    assert fields == ["outcome_count", "sum_steps", "los_episodes", "sum_los_steps", "sep_hist", "lane_return_sum",
                      "lane_return_sq", "lane_worst_sep", "lane_worst_episode", "n_bins", "episodes_per_lane", "inv_bin_width",
                      "first_episode", "_pad"]
    assert all(f in header for f in fields)
    for name in ENTRIES:                                   # the stats siblings' arguments without the three per-episode outputs
        stats = getattr(L, name.replace("monte_carlo", "evaluate_policies_stats")).argtypes
        assert list(getattr(L, name).argtypes) == list(stats[:11]) + [C.POINTER(g.native.CMonteCarlo), stats[-1]]
    me = g.policy.monte_carlo_entry
    assert (me(torch.float32), me(torch.float64), me(torch.float32, True)) == ENTRIES
    with pytest.raises(ValueError, match="float32 only"):
        me(torch.float64, group=True)


def test_monte_carlo_validation_is_in_the_golden_grid():
    """The campaign's rejections -- a NULL mc, each NULL accumulator, episodes_per_lane, n_bins, the 32-bit episode counter,
    the step budget, the work shapes and everything the evaluators refuse: tests/test_scoring_rejections_host.py holds the
    three entries to the whole text of each.  Here: that its grid has them."""
    for entry in ENTRIES:
        for by_id in SR.covered(entry).values():
            # first_episode + episodes_per_lane = 2^32 exactly fits the counter: the work shape stops that call
            assert "episode counter" not in by_id["counter-fits"]
    assert "exceeds the 32-bit episode counter" in SR.covered(ENTRIES[0])["1"]["counter-wraps"]
