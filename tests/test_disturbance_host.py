"""Sensor noise and actuator disturbance, host side (no GPU): the NumPy specification in records.py -- disturbance_words(),
disturbance_normals(), disturb_observation(), disturb_action() -- against numbers written out here, policy.Disturbance, the
five entry points in the header, the loader and the built library, and their argument validation (every pointer below is
a host address: the calls are refused before any launch)."""
import ctypes as C
import dataclasses
import json
import math
import os

import numpy as np
import pytest
import torch

import scoring_rejections_support as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVAL = ("acas2d_evaluate_policies_disturbed_f32", "acas2d_evaluate_policies_disturbed_group_f32")
CAMPAIGN = ("acas2d_monte_carlo_disturbed_f32", "acas2d_monte_carlo_disturbed_group_f32")
WIDE_SEED = 0x9E3779B97F4A7C15


@pytest.fixture(scope="module")
def g():
    import gym_acas2d_amd as g
    return g


# ---- the draws ----------------------------------------------------------------------------------------------------------------
# (seed, lane, episode, step, slot) -> the block, from Philox4x32-7 in plain Python integers (below) on the counter
# (lane lo, lane hi, episode, step | slot << 20) and the key (seed lo, seed hi ^ 0x64697374)
KNOWN = (((7, 0, 5, 0, 0), (3821301219, 3132813609, 693968140, 2045481059)),
         ((7, (1 << 32) + 5, 5, (1 << 20) - 2, 64), (269486190, 2603867219, 1373766412, 1483235371)),      # the largest step: max_steps
         ((WIDE_SEED, 69, 0, 120, 1), (2323075674, 2715829625, 2552941233, 3368324030)),
         ((13, 3, 0xFFFFFFFF, 1, 8), (240745920, 2189407157, 1332662275, 1811362345)))


def philox_ints(c, k, rounds=7):
    c, k = list(c), list(k)
    for _ in range(rounds):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def test_words_on_written_out_counters(g):
    for (seed, lane, ep, step, slot), want in KNOWN:
        assert g.records.disturbance_words(seed, lane, ep, step, slot).tolist() == list(want), (seed, lane, ep, step, slot)
        ctr = [lane & 0xFFFFFFFF, lane >> 32, ep, step | slot << 20]
        assert philox_ints(ctr, [seed & 0xFFFFFFFF, (seed >> 32) ^ 0x64697374]) == list(want)
    # broadcast: [lanes, 1] x [slots] -> [lanes, slots, 4], each block the scalar call's
    lanes, slots = np.array([[0], [(1 << 32) + 5]]), np.array([0, 64])
    w = g.records.disturbance_words(7, lanes, 5, 0, slots)
    assert w.shape == (2, 2, 4) and w.dtype == np.uint32 and w[0, 0].tolist() == list(KNOWN[0][1])
    assert w[1, 1].tolist() == g.records.disturbance_words(7, (1 << 32) + 5, 5, 0, 64).tolist()
    assert g.records.DISTURBANCE_TAG == 0x64697374 and g.records.DISTURBANCE_SLOT_SHIFT == 20
    for bad in ((7, 0, 0, 1 << 20, 0), (7, 0, 0, 0, 65), (7, 0, 1 << 32, 0, 0)):
        with pytest.raises(ValueError):
            g.records.disturbance_words(*bad)


def test_blocks_differ_from_the_resets_under_the_same_seed(g):
    """The reset draws entity e of (lane, episode) with counter (lane lo, lane hi, episode, e) under the key (seed lo, seed
    hi); the disturbance's step 0, slot 0 has the same counter as e = 0, and step e, slot 0 the same as entity e: only the
    tag in the key keeps them apart."""
    lanes = np.arange(70)[:, None, None]
    eps = np.array([0, 5])[None, :, None]
    ent = np.arange(9)[None, None, :]
    for seed in (13, WIDE_SEED):
        ctr = np.stack(np.broadcast_arrays(lanes, 0 * lanes, eps, ent), axis=-1)
        reset = g.records.philox4x32(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32]))
        for slot in (0, 1):
            dist = g.records.disturbance_words(seed, lanes, eps, ent, slot)
            assert reset.shape == dist.shape == (70, 2, 9, 4)
            assert not (reset == dist).all(-1).any()
        # (the untagged key WOULD collide at slot 0: the tag is what the assertion above tests)
        untagged = g.records.disturbance_words(seed ^ (0x64697374 << 32), lanes, eps, ent, 0)
        assert (untagged == reset).all()


def test_normals_from_words(g):
    """The uniforms are the kernels' float32 ones: k + 0.5 as it is below k = 2^23, and from there on -- a tie in float32 --
    the even neighbour: k = 0x800000 stays, k = 0x800001 and 0xFFFFFD go up by one, 0xFFFFFE stays, and k = 0xFFFFFF gives
    u = 1, whose normal is 0."""
    w = np.array([[0x80000000, 0x00000000, 0xFFFFFFFF, 0x40000000], [0x80000100, 0x3FFFFF00, 0xFFFFFE00, 0x00000000],
                  [0xFFFFFD00, 0x7FFFFF00, 0x7FFFFFFF, 0x80000000]], np.uint32)
    us = [[0x800000 / 2 ** 24, 0.5 / 2 ** 24, 1.0, (0x400000 + 0.5) / 2 ** 24],
          [0x800002 / 2 ** 24, (0x3FFFFF + 0.5) / 2 ** 24, 0xFFFFFE / 2 ** 24, 0.5 / 2 ** 24],
          [0xFFFFFE / 2 ** 24, (0x7FFFFF + 0.5) / 2 ** 24, (0x7FFFFF + 0.5) / 2 ** 24, 0x800000 / 2 ** 24]]
    got = g.records.disturbance_normals(w)
    assert got.shape == (3, 3) and got.dtype == np.float64
    for row, u in zip(got, us):
        r1, r3 = math.sqrt(-2.0 * math.log(u[0])), math.sqrt(-2.0 * math.log(u[2]))
        want = [r1 * math.cos(2 * math.pi * u[1]), r1 * math.sin(2 * math.pi * u[1]), r3 * math.cos(2 * math.pi * u[3])]
        assert np.allclose(row, want, rtol=1e-14, atol=1e-300)
    assert got[0, 2] == 0.0 and got[1, 2] == pytest.approx(2.0 ** -11, rel=1e-6)        # r(1 - 2^-23) = sqrt(2^-22 (1 + ...))
    # ... and what float32 makes of k + 0.5, worked out here in integers: exact below 2^23, then ties to even
    k = np.array([0, 1, 0x7FFFFF, 0x800000, 0x800001, 0xFFFFFC, 0xFFFFFD, 0xFFFFFE, 0xFFFFFF], np.uint32)
    twice = np.where(k < 0x800000, 2 * k.astype(np.int64) + 1, 2 * (k.astype(np.int64) + (k & 1)))
    assert ((k.astype(np.float32) + np.float32(0.5)).astype(np.float64) * 2 == twice).all()
    # a quarter of a million blocks: three standard normals, uncorrelated (5 standard errors)
    z = g.records.disturbance_normals(g.records.disturbance_words(3, np.arange(1 << 18), 0, 0, 1))
    n = z.shape[0]
    assert (np.abs(z.mean(0)) < 5 / math.sqrt(n)).all() and (np.abs(z.var(0) - 1) < 5 * math.sqrt(2 / n)).all()
    assert (np.abs(np.corrcoef(z.T)[np.triu_indices(3, 1)]) < 5 / math.sqrt(n)).all()


# ---- the arithmetic -----------------------------------------------------------------------------------------------------------
def f32(x):
    return np.float32(x)


def test_disturb_observation_by_hand(g):
    do = g.records.disturb_observation
    own = [0.1, 0.2, 0.3, 0.4, 0.5]
    obs = np.array(own + [0.5, 0.25, -0.75, 0.99, -0.99, 0.99], np.float32)
    z = np.array([[1.0, -2.0, 0.5], [3.0, -3.0, 3.0]], np.float32)
    out = do(obs, (0.25, 0.125, 0.5), z)
    assert out.dtype == np.float32 and out[:5].tolist() == obs[:5].tolist()
    # aircraft 0: 0.5 + 0.25, 0.25 - 0.25, -0.75 + 0.25 (exact in float32); aircraft 1: all three leave the box at its upper /
    # lower / upper end
    assert out[5:].tolist() == [0.75, 0.0, -0.5, 1.0, -1.0, 1.0]
    # ... and the other ends: the separation at 0, the other two at -1 and +1
    out = do(np.array(own + [0.1, -0.9, 0.9], np.float32), (0.25, 0.125, 0.5), np.array([[-1.0, -1.0, 1.0]], np.float32))
    assert out[5:].tolist() == [0.0, -1.0, 1.0]
    out = do(np.array(own + [0.9, 0.9, -0.9], np.float32), (0.25, 0.125, 0.5), np.array([[1.0, 1.0, -1.0]], np.float32))
    assert out[5:].tolist() == [1.0, 1.0, -1.0]
    # two roundings: fl(fl(s z) + x), not the fused fl(s z + x).  s = z = 1 + 2^-12: s z = 1 + 2^-11 + 2^-24 is a tie between
    # float32 neighbours and rounds to the even one, 1 + 2^-11; plus x = -1 that is 2^-11, where a fused multiply-add would
    # keep the 2^-24
    s = zz = f32(1 + 2.0 ** -12)
    assert float(s) * float(zz) - 1.0 == 2.0 ** -11 + 2.0 ** -24
    out = do(np.array(own + [0.5, -1.0, 0.0], np.float32), (0.0, s, 0.0), np.array([[9.0, zz, 9.0]], np.float32))
    assert float(out[6]) == 2.0 ** -11 and out[5] == 0.5 and out[7] == 0.0
    # a zero sigma leaves an entry alone, outside the box too; the others are still clamped
    wild = np.array(own + [1.5, -3.0, 7.0], np.float32)
    assert do(wild, (0.0, 0.0, 0.0), z[:1]).tolist() == wild.tolist()
    assert do(wild, (0.0, 1.0, 0.0), z[:1])[5:].tolist() == [1.5, -1.0, 7.0]
    assert do(wild, (1.0, 0.0, 1.0), z[:1])[5:].tolist() == [1.0, -3.0, 1.0]
    # NaN stays NaN (in the entry or in the normal); the own-ship entries are never touched, NaN or not
    nan = np.array([np.nan] * 5 + [np.nan, 0.5, 0.5], np.float32)
    out = do(nan, (0.5, 0.5, 0.5), np.array([[1.0, np.nan, 0.0]], np.float32))
    assert np.isnan(out[:7]).all() and out[7] == 0.5
    # batches: [E, D] with [E, N, 3]
    both = do(np.stack([obs, obs]), (0.25, 0.125, 0.5), np.stack([z, 0 * z]))
    assert both[0, 5:].tolist() == [0.75, 0.0, -0.5, 1.0, -1.0, 1.0] and both[1].tolist() == obs.tolist()
    with pytest.raises(ValueError):
        do(obs, (0.1, 0.1, 0.1), z[:1])
    assert g.records.OBSERVATION_BOX == ((0.0, 1.0), (-1.0, 1.0), (-1.0, 1.0))
    lo, hi = g.ACAS2DConfig(n_traffic=1).obs_low_high()
    assert tuple(zip(lo[5:], hi[5:])) == g.records.OBSERVATION_BOX


def test_disturb_action_by_hand(g):
    da = g.records.disturb_action
    a = np.array([0.5, 0.9, -0.9, 1.0, np.nan, 0.25], np.float32)
    z = np.array([1.0, 1.0, -1.0, -8.0, 1.0, np.nan], np.float32)
    out = da(a, 0.25, z)
    assert out.dtype == np.float32 and out[:4].tolist() == [0.75, 1.0, -1.0, -1.0] and np.isnan(out[4:]).all()
    assert da(np.array([3.0], np.float32), 0.0, np.array([1.0], np.float32)).tolist() == [3.0]     # zero: untouched
    assert da(np.float32(0.5), 0.5, np.float32(-1.0)) == 0.0


# ---- Disturbance ----------------------------------------------------------------------------------------------------------------
def test_disturbance_converts_pixels_to_normalised_units(g):
    D = g.policy.Disturbance
    cfg = g.ACAS2DConfig(n_traffic=3, max_steps=150)
    c = cfg.to_c()
    d = D(sep=30.0, cpa=20.0, closing=8.0, action=0.1, seed=WIDE_SEED, config=cfg)
    assert d.s_sep == float(np.float32(30.0 / c.d_sep_max)) and d.s_cpa == float(np.float32(20.0 / c.d_cpa_max))
    assert d.s_closing == float(np.float32(8.0 / c.v_closing_max)) and d.s_action == float(np.float32(0.1)) and d.seed == WIDE_SEED
    assert d.sigma == (d.s_sep, d.s_cpa, d.s_closing)
    # the default config's ranges: d_sep_max = diagonal + 2 x 2 000 px of path, d_cpa_max = the diagonal, v_closing_max = 400
    diag = math.sqrt(1600.0 ** 2 + 1000.0 ** 2)
    e = D(sep=diag + 4000.0, cpa=diag / 2, closing=100.0)
    assert (e.s_sep, e.s_cpa, e.s_closing, e.s_action, e.seed) == (1.0, 0.5, 0.25, 0.0, 0)
    n = D.normalised(sep=0.05, cpa=0.1, closing=0.1, action=0.3, seed=7)
    assert n.sigma == tuple(float(np.float32(v)) for v in (0.05, 0.1, 0.1)) and n.s_action == float(np.float32(0.3))
    # comparable, hashable, serialisable
    assert n == D.normalised(0.05, 0.1, 0.1, 0.3, 7) and n != D.normalised(0.05, 0.1, 0.1, 0.3, 8) and len({n, D.normalised(0.05, 0.1, 0.1, 0.3, 7)}) == 1
    assert D.from_dict(n.to_dict()) == n and D.from_dict(d.to_dict()) == d
    assert D.from_dict(json.loads(json.dumps(d.to_dict()))) == d
    assert D().is_zero() and not n.is_zero() and D() == D.normalised()
    cd = d.to_c(noise_episode=5)
    assert (cd.s_sep, cd.s_cpa, cd.s_closing, cd.s_action, cd.noise_seed, cd.noise_episode) == (
        d.s_sep, d.s_cpa, d.s_closing, d.s_action, WIDE_SEED, 5)
    with pytest.raises(dataclasses.FrozenInstanceError):
        d.s_sep = 1.0


# ---- header, loader, library ------------------------------------------------------------------------------------------------
def test_entries_in_header_loader_and_library(g):
    with open(os.path.join(ROOT, "include", "acas2d.h")) as f:
        header = f.read()
    L = g.native.lib()
    for name in EVAL + CAMPAIGN + ("acas2d_disturbance_draw_f32", "acas2d_disturbance_size"):
        assert (" %s(" % name) in header and name in g.native.EXPORTS and hasattr(L, name), name
    assert "typedef struct Acas2dDisturbance {" in header and "#define ACAS2D_ABI_VERSION 7" in header
    assert L.acas2d_abi_version() == g.native.ABI_VERSION == 7
    assert C.sizeof(g.native.CDisturbance) == L.acas2d_disturbance_size() == 32
    fields = [n for n, _ in g.native.CDisturbance._fields_]
    assert fields == ["s_sep", "s_cpa", "s_closing", "s_action", "noise_seed", "noise_episode", "_pad"]
    assert all(f in header for f in fields)
    ptr = C.POINTER(g.native.CDisturbance)
    for name in EVAL:                                      # the stats siblings' arguments, the disturbance before stream
        sib = getattr(L, name.replace("disturbed", "stats")).argtypes
        assert list(getattr(L, name).argtypes) == list(sib[:-1]) + [ptr, sib[-1]]
    for name in CAMPAIGN:
        sib = getattr(L, name.replace("_disturbed", "")).argtypes
        assert list(getattr(L, name).argtypes) == list(sib[:-1]) + [ptr, sib[-1]]
    ee, me = g.policy.evaluate_policies_entry, g.policy.monte_carlo_entry
    assert (ee(torch.float32, disturbed=True), ee(torch.float32, True, True, True)) == EVAL
    assert (me(torch.float32, disturbed=True), me(torch.float32, True, True)) == CAMPAIGN
    for f in (ee, me):
        with pytest.raises(ValueError, match="float32 only"):
            f(torch.float64, disturbed=True)
    assert ee(torch.float32, False, True) == "acas2d_evaluate_policies_stats_f32" and me(torch.float64) == "acas2d_monte_carlo_f64"


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_validation_is_in_the_golden_grid(g):
    """Everything the undisturbed sibling refuses, in its words under the entry's own name; a NULL disturbance; every
    standard deviation negative, NaN or infinite; max_steps + 1 >= 2^20: tests/test_scoring_rejections_host.py holds these
    four entries to the whole text of each.  Here: that its grid has them, and the calls it does not make."""
    for entry in EVAL + CAMPAIGN:
        by_n = SR.covered(entry)
        assert "the step field of the noise counter" in by_n[str(SR.ENTRIES[entry][2][0])]["max-steps-%d" % ((1 << 20) - 1)]
        for by_id in by_n.values():
            # max_steps = 2^20 - 2 is admissible: the call passes the noise counter's check and is stopped by the work shape
            assert "the step field of the noise counter" not in by_id["max-steps-admissible"]
    # the evaluators look at n_traffic = 0 with the campaign's step budget too
    for entry, N in zip(EVAL, (1, 16)):
        assert SR.call(g, entry, N, {"n": 0, "T": 2000}) == (SR.EINVAL, "%s: n_traffic = 0, n_steps = 2000" % entry[:-4])


def test_draw_validation_needs_no_gpu(g):
    L = g.native.lib()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    name = "acas2d_disturbance_draw"

    def rejects(msg, seed=7, lane=0, lanes=2, ep=0, step=0, steps=2, slots=2, out=a):
        assert L.acas2d_disturbance_draw_f32(seed, lane, lanes, ep, step, steps, slots, out, None) == -22
        assert msg.encode() in L.acas2d_last_error(), L.acas2d_last_error()

    rejects(name + ": NULL out", out=None)
    for kw in ({"lanes": 0}, {"steps": 0}, {"slots": 0}, {"lanes": -1}):
        rejects("(at least 1 each)", **kw)
    rejects("negative first_lane / first_step", lane=-1)
    rejects("negative first_lane / first_step", step=-1)
    rejects("exceeds the step field of the noise counter", step=(1 << 20) - 1, steps=2)
    rejects("n_slots = 66 (at most 65", slots=66)
    rejects("at most 2^38", lanes=0x7FFFFFFF, steps=1 << 20, slots=65)
