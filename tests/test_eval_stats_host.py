"""Per-episode safety statistics of the fused evaluator, host side (no GPU): records.episode_safety() -- the NumPy
restatement of the six definitions of include/acas2d.h (Acas2dEvalStats) -- against the reference's own record lists,
the argument validation of acas2d_evaluate_policies_stats_f32 / _f64 / _group_f32, and the entry point
evaluate_policies_fused() chooses with and without safety=."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers as H
import scoring_rejections_support as SR

SAFE = 192.0                                             # settings.py: SAFE_DISTANCE (config.safe_distance)


@pytest.fixture(scope="module")
def g():
    import gym_acas2d_amd as g
    return g


def _episodes(N):
    """The captured episodes of tests/golden/ref_records_n{N}.npz as (d_sep, a_lat, d_dev, outcome, steps) per episode."""
    fx = H.load("ref_records_n%d.npz" % N)
    off = fx["off_records"]
    for i in range(len(off) - 1):
        sl = slice(off[i], off[i + 1])
        yield (fx["d_sep_record"][sl], fx["a_lat_record"][sl], fx["d_dev_record"][sl], int(fx["outcome"][i]),
               int(fx["steps"][i]))


@pytest.mark.parametrize("N", (1, 3))
def test_episode_safety_on_the_reference_record_lists(g, N):
    """Every definition restated independently with whole-array NumPy on rows 1.. of the reference's lists."""
    both_signs = [False, False]
    n_eps = 0
    for d_sep, a_lat, d_dev, outcome, steps in _episodes(N):
        assert len(d_sep) == len(a_lat) == len(d_dev) == steps          # the lists hold row 0 and steps - 1 step rows
        assert not (np.isnan(d_sep).any() or np.isnan(a_lat).any() or np.isnan(d_dev).any())
        got = g.records.episode_safety(d_sep, a_lat, d_dev, SAFE)
        rows = d_sep[1:]
        assert got["min_sep"] == rows.min() and got["min_sep_step"] == 1 + int(np.argmin(rows))
        assert d_sep[got["min_sep_step"]] == got["min_sep"]            # its position in d_sep_record
        assert got["los_steps"] == int((rows < 192).sum())
        assert got["max_a_lat"] == np.abs(a_lat[1:]).max() and got["max_dev"] == np.abs(d_dev[1:]).max()
        seq = 0.0
        for v in d_dev[1:]:
            seq = seq + abs(float(v))
        assert got["sum_dev"] == seq
        assert got["sum_dev"] == pytest.approx(np.abs(d_dev[1:]).sum(), rel=1e-12)
        if outcome == 2:                                                # a collision: the closest row is the last one
            assert got["min_sep_step"] == steps - 1 and 94.0 < got["min_sep"] < 98.0 and got["los_steps"] > 0
        both_signs[0] |= bool((d_dev[1:] < 0).any())
        both_signs[1] |= bool((d_dev[1:] > 0).any())
        n_eps += 1
    assert n_eps == 6 and all(both_signs)


def test_episode_safety_excludes_row_0(g):
    """n = 3, episode 1: the minimum of the step rows is 285.642 at step row 1, while row 0 holds 286.1 -- and rows
    that would change every statistic if row 0 counted."""
    d_sep, a_lat, d_dev, _, _ = list(_episodes(3))[1]
    got = g.records.episode_safety(d_sep, a_lat, d_dev, SAFE)
    assert got["min_sep_step"] == 1 and got["min_sep"] == d_sep[1] and abs(got["min_sep"] - 285.642) < 1e-3
    assert abs(d_sep[0] - 286.1) < 0.05 and d_sep[0] > d_sep[1]
    low = g.records.episode_safety(np.r_[1.0, d_sep[1:]], np.r_[1e9, a_lat[1:]], np.r_[-1e9, d_dev[1:]], SAFE)
    for k, v in got.items():
        assert low[k] == v, k


def test_episode_safety_order_ties_nan_and_dtype(g):
    es = g.records.episode_safety
    # the FIRST row that attains the minimum; |.| of signed a_lat / d_dev; rows below the safe distance, strictly
    got = es([0, 5, 3, 3, 192, 191.5], [0, -7, 2, 1, 0, 0], [0, 1, -4, 2, 0, -0.5], SAFE)
    assert (got["min_sep"], got["min_sep_step"], got["los_steps"]) == (3.0, 2, 4)
    assert (got["max_a_lat"], got["max_dev"], got["sum_dev"]) == (7.0, 4.0, 7.5)
    # a NaN never replaces a held value and never counts as a loss of separation; it does poison the sum
    nan = float("nan")
    got = es([0, nan, 50, nan], [0, 3, nan, 1], [0, nan, 2, 1], SAFE)
    assert (got["min_sep"], got["min_sep_step"], got["los_steps"], got["max_a_lat"], got["max_dev"]) == (50.0, 2, 1, 3.0, 2.0)
    assert np.isnan(got["sum_dev"])
    got = es([0, nan], [0, nan], [0, nan], SAFE)
    assert got["min_sep"] == np.inf and got["min_sep_step"] == 0 and got["max_a_lat"] == 0 and got["max_dev"] == 0
    # the sum is sequential IN dtype
    dev = np.r_[0.0, np.full(4000, 0.1)]
    z = np.zeros_like(dev)
    f32 = es(z + 500, z, dev, SAFE, dtype=np.float32)
    seq = np.float32(0)
    for v in dev[1:].astype(np.float32):
        seq = np.float32(seq + v)
    assert f32["sum_dev"].dtype == np.float32 and f32["sum_dev"] == seq and f32["sum_dev"] != np.float32(dev[1:].sum())
    with pytest.raises(ValueError):
        es([0, 1], [0, 1, 2], [0, 1], SAFE)


def test_safety_columns_speaks_the_fused_evaluators_keys(g):
    eps = list(_episodes(3))
    cols = {"d_sep": [list(e[0]) for e in eps], "a_lat": [list(e[1]) for e in eps], "d_dev": [list(e[2]) for e in eps],
            "Time Steps": [e[4] for e in eps]}
    out = g.records.safety_columns(cols, SAFE)
    assert tuple(out) == g.records.SAFETY_KEYS == ("min_separation", "min_separation_step", "los_steps", "max_abs_a_lat",
                                                   "max_abs_deviation", "mean_abs_deviation")
    for i, (d_sep, a_lat, d_dev, _, steps) in enumerate(eps):
        one = g.records.episode_safety(d_sep, a_lat, d_dev, SAFE)
        assert out["min_separation"][i] == one["min_sep"] and out["min_separation_step"][i] == one["min_sep_step"]
        assert out["los_steps"][i] == one["los_steps"] and out["max_abs_a_lat"][i] == one["max_a_lat"]
        assert out["max_abs_deviation"][i] == one["max_dev"]
        assert out["mean_abs_deviation"][i] == one["sum_dev"] / (steps - 1)
    one_row = g.records.safety_columns({"d_sep": [[7.0]], "a_lat": [[0.0]], "d_dev": [[3.0]], "Time Steps": [1]}, SAFE)
    assert one_row["mean_abs_deviation"] == [0.0] and one_row["min_separation_step"] == [0]


def test_evaluate_policies_stats_validation_is_in_the_golden_grid(g):
    """The stats entry points reject a NULL stats, each NULL member of it, a traffic count of the wrong sibling and
    everything the plain entry points reject: tests/test_scoring_rejections_host.py holds the three entries to the whole
    text of each.  Here: that its grid has them, and the one call it does not make."""
    assert [n for n, _ in g.native.CEvalStats._fields_] == ["min_sep", "min_sep_step", "los_steps", "max_a_lat", "max_dev", "sum_dev"]
    for tail in ("f32", "f64", "group_f32"):
        SR.covered("acas2d_evaluate_policies_stats_" + tail)
    # the widest group shape, which the grid does not call at
    assert SR.call(g, "acas2d_evaluate_policies_stats_group_f32", 64, {"T": 0}) == (
        SR.EINVAL, "acas2d_evaluate_policies_stats_group: n_traffic = 64, n_steps = 0")


def test_stats_struct_and_prototypes(g):
    """struct Acas2dEvalStats is six pointers, and the stats entry points take the plain siblings' arguments with the
    stats pointer in front of the stream."""
    L = g.native.lib()
    assert C.sizeof(g.native.CEvalStats) == 6 * C.sizeof(C.c_void_p)
    for tail in ("f32", "f64", "group_f32"):
        plain = getattr(L, "acas2d_evaluate_policies_" + tail).argtypes
        stats = getattr(L, "acas2d_evaluate_policies_stats_" + tail).argtypes
        assert list(stats) == list(plain[:-1]) + [C.POINTER(g.native.CEvalStats), plain[-1]]


def test_evaluate_policies_fused_entry_points(g, monkeypatch):
    """safety=False resolves the plain entry point (today's call), safety=True its stats sibling; evaluate_policies_fused
    looks its entry point up through this one function."""
    ep = g.policy.evaluate_policies_entry
    f32, f64 = torch.float32, torch.float64
    assert ep(f32) == ep(f32, False, False) == "acas2d_evaluate_policies_f32"
    assert ep(f64) == "acas2d_evaluate_policies_f64" and ep(f32, group=True) == "acas2d_evaluate_policies_group_f32"
    assert ep(f32, safety=True) == "acas2d_evaluate_policies_stats_f32"
    assert ep(f64, safety=True) == "acas2d_evaluate_policies_stats_f64"
    assert ep(f32, group=True, safety=True) == "acas2d_evaluate_policies_stats_group_f32"
    L = g.native.lib()
    for dt in (f32, f64):
        for group in (False, True):
            for safety in (False, True):
                if group and dt == f64:
                    with pytest.raises(ValueError, match="float32 only"):
                        ep(dt, group, safety)
                else:
                    assert hasattr(L, ep(dt, group, safety)) and ep(dt, group, safety) in g.native.EXPORTS
    # the function asks for its entry point before it touches the device: record what it asks for
    asked = []

    def spy(dtype, group=False, safety=False):
        asked.append(ep(dtype, group, safety))
        raise LookupError("stop here")

    monkeypatch.setattr(g.policy, "evaluate_policies_entry", spy)
    z = np.zeros((4, 4))
    for kw, want in (({}, "acas2d_evaluate_policies_f32"), ({"safety": False}, "acas2d_evaluate_policies_f32"),
                     ({"safety": True}, "acas2d_evaluate_policies_stats_f32")):
        with pytest.raises(LookupError):
            g.evaluate_policies_fused([object()], z, np.zeros((4, 1, 4)), dtype=f32, **kw)
        assert asked[-1] == want
