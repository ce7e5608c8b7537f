"""The kernels of the delayed evaluator and campaign (eval_stats_delayed_kernel, monte_carlo_delayed_kernel,
csrc/acas2d_scoring_delayed.hip) from the code-object metadata of the unit compiled with the flags the Makefile gives it
(helpers.kernel_metadata), as test_correlated_build.py reads their siblings': the eighteen kernels exist at the correlated kernels'
nine shapes and nothing else does, none spills a VGPR or has a private segment, each takes at most 256 VGPRs (two waves per SIMD),
and the LDS a launch asks for -- all of it dynamic: the tile, the reset slots, the group shapes' hidden vectors, the error state
of 3 C + 1 values per lane and the lag's one value per lane behind them -- stays within the launcher's 64 KiB per workgroup, two
workgroups within a compute unit's 160 KiB.  (The dead time's line is device memory, Acas2dResponse::ring: no LDS.)

Observed: profiles/response_isa.txt has the table (vgpr_count eval / campaign next to the correlated siblings', LDS bytes)."""
import re

import pytest

import helpers as H

SHAPES = ((1, 1), (2, 1), (3, 1), (4, 1), (8, 1), (4, 2), (4, 4), (4, 8), (4, 16))
KERNELS = ("eval_stats_delayed_kernel", "monte_carlo_delayed_kernel")
IDS = ["%s-%d,%d" % (name.split("_delayed")[0], C, G) for name in KERNELS for C, G in SHAPES]
_META = {}


def kernels_of(tmp_path_factory):
    if "k" not in _META:                                      # one compilation for the module
        _META["k"] = H.kernel_metadata(tmp_path_factory.mktemp("scoring_delayed"), "acas2d_scoring_delayed.hip")[1]
    return _META["k"]


def by_shape(kernels):
    out = {}
    for k in kernels:
        m = re.match(r"_ZN6acas2d\d+(eval_stats_delayed_kernel|monte_carlo_delayed_kernel)IfLi(\d+)ELi(\d+)ELb1EEE", k.name)
        if m:
            out[m.group(1), int(m.group(2)), int(m.group(3))] = k
    return out


def correlated_lds_bytes(C, G, correlated=True):
    """geometry_for() of csrc/acas2d_launch.inl for a float32 policy launch at the packed shape (C, G): bytes per workgroup
    (test_correlated_build.lds_bytes)."""
    N, epw, waves, hidden = C * G, 64 // G, 4, 64
    tile = (epw * (5 + 3 * N) + 3) // 4 * 4
    if N + 1 <= 32:
        stride = 2
        while stride < N + 1:
            stride *= 2
        scratch = (64 // stride) * ((4 * N + 1 + 3) // 4 * 4)
    else:
        scratch = 4 * N + 1
    elems = (tile + scratch + 3) // 4 * 4 + (epw * hidden if G > 1 else 0) + (64 * (3 * C + 1) if correlated else 0)
    return elems * waves * 4


def lds_bytes(C, G):
    """... with held = kCorrSlots(C) + 1: the correlated launch's bytes and one float per lane of four waves."""
    return correlated_lds_bytes(C, G) + 4 * 64 * 4


@H.needs_hipcc
def test_eighteen_kernels_none_spills(tmp_path_factory):
    kernels = kernels_of(tmp_path_factory)
    found = by_shape(kernels)
    assert sorted(found) == sorted((name, C, G) for name in KERNELS for C, G in SHAPES)
    assert len(kernels) == 18                                                       # the unit holds nothing else
    for (name, C, G), k in sorted(found.items()):
        print("%s<float, %d, %d>: vgpr %d sgpr %d sgpr spills %d; LDS per workgroup %d bytes, all dynamic (%d without the lag's slot)"
              % (name, C, G, k.field("vgpr_count"), k.field("sgpr_count"), k.field("sgpr_spill_count"), lds_bytes(C, G),
                 correlated_lds_bytes(C, G)))
        assert k.field("vgpr_spill_count") == 0 and k.field("private_segment_fixed_size") == 0, (name, C, G)
        assert k.field("group_segment_fixed_size") == 0, (name, C, G)               # nothing static beside what the launcher sizes
        assert k.field("sgpr_spill_count") < 400, (name, C, G)                       # the float32 unit's own limit


@H.needs_hipcc
@pytest.mark.parametrize("key", [(name, C, G) for name in KERNELS for C, G in SHAPES], ids=IDS)
def test_at_most_256_vgprs(tmp_path_factory, key):
    k = by_shape(kernels_of(tmp_path_factory))[key]
    print("%s: vgpr %d" % (k.name, k.field("vgpr_count")))
    assert k.field("vgpr_count") <= 256, (k.name, k.field("vgpr_count"))


@pytest.mark.parametrize("shape", SHAPES, ids=["%d,%d" % s for s in SHAPES])
def test_lds_within_the_launchers_limit(shape):
    """(tests/test_response_host.py holds the launcher itself to it: every shape gets past geometry_for().)"""
    C, G = shape
    assert lds_bytes(C, G) == correlated_lds_bytes(C, G, False) + 4 * 64 * (3 * C + 2) * 4
    assert lds_bytes(C, G) <= 64 * 1024                      # the launcher's limit per workgroup
    assert 2 * lds_bytes(C, G) <= 160 * 1024                 # two workgroups -- eight waves -- per compute unit


def test_the_largest_launch_is_the_two_lane_group():
    assert max(SHAPES, key=lambda s: lds_bytes(*s)) == (4, 2)
    assert (correlated_lds_bytes(4, 2), lds_bytes(4, 2)) == (63232, 64256)
