"""tests/edge_observations.py admitted on the CPU (no GPU): the table holds what it says, the rotation brings every value to
every channel of every traffic slot, the NumPy specification passes check_reference() under every disturbance of the
injected-row tests -- and three wrong disturbed() do not: a clamp by fmin / fmax, no early return for s == 0, a fused
multiply-add."""
import numpy as np
import pytest

import edge_observations as EO

F = np.float32
E = 70


@pytest.fixture(scope="module")
def records():
    import gym_acas2d_amd as g
    return g.records


def rows(records, N, shift=0):
    rng = np.random.default_rng(N)
    return EO.inject(rng.uniform(0, 1, (E, 5 + 3 * N)).astype(F), records.OBSERVATION_BOX, shift)


def normals(N, seed=1):
    return np.random.default_rng(seed).standard_normal((E, N, 3)).astype(F)


def sigma_of(name):
    d = EO.DISTURBANCES[name]
    return tuple(float(F(d[k])) for k in ("sep", "cpa", "closing"))


def test_the_table(records):
    tab = EO.table(records.OBSERVATION_BOX)
    assert tab.shape == (3, EO.V) and tab.dtype == F
    for (lo, hi), v in zip(records.OBSERVATION_BOX, tab):
        named = dict(zip(EO.NAMES, v))
        assert named["lo"] == F(lo) and named["hi"] == F(hi)
        assert named["below lo"] < F(lo) < named["above lo"] and named["below hi"] < F(hi) < named["above hi"]
        assert not ((v > named["below lo"]) & (v < F(lo))).any() and not ((v > F(hi)) & (v < named["above hi"])).any()
        assert EO.bits(named["+0"]) == 0 and EO.bits(named["-0"]) == 0x80000000
        assert EO.bits(named["+denormal"]) == 1 and EO.bits(named["-denormal"]) == 0x80000001
        assert named["+FLT_MAX"] == np.finfo(F).max == -named["-FLT_MAX"] and named["+1.5"] == 1.5 == -named["-1.5"]
        assert np.isposinf(named["+inf"]) and np.isneginf(named["-inf"]) and np.isnan(named["NaN"])


@pytest.mark.parametrize("N", (1, 3, 64))
def test_every_value_meets_every_channel_of_every_slot(records, N):
    idx = EO.value_index(E, N)
    assert idx.shape == (E, N, 3)
    for n in range(N):
        for c in range(3):
            assert set(idx[:, n, c].tolist()) == set(range(EO.V)), (n, c)
    row = rows(records, N)
    tab = EO.table(records.OBSERVATION_BOX)
    assert np.array_equal(EO.bits(row[:, 5:]).reshape(E, N, 3), EO.bits(tab)[np.arange(3), idx])
    assert (np.diff(idx.reshape(E, 3 * N), axis=1) % EO.V != 0).all()             # neighbours in a row differ
    assert not np.array_equal(EO.bits(rows(records, N, shift=3)), EO.bits(row))   # a later launch reads another row
    plain = np.random.default_rng(N).uniform(0, 1, (E, 5 + 3 * N)).astype(F)
    assert np.array_equal(row[:, :5], plain[:, :5])                               # the own-ship five stay


@pytest.mark.parametrize("name", list(EO.DISTURBANCES))
def test_the_specification_passes(records, name):
    row, z, sigma = rows(records, 3), normals(3), sigma_of(name)
    ref = records.disturb_observation(row, sigma, z)
    EO.check_reference(row, ref, sigma, records.OBSERVATION_BOX, vanishing=name == "vanishing")
    assert EO.same_but_for_nan_bits(ref, ref)
    if name == "overflowing":                                                     # inf - inf: a NaN nobody injected
        assert (np.isnan(ref) & ~np.isnan(row)).any()


def wrong(kind, x, s, z, lo, hi):
    """disturbed() with one defect, in NumPy."""
    x, s, z = np.asarray(x, F), F(s), np.asarray(z, F)
    if s == 0 and kind != "no early return":
        return x.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        if kind == "fused":
            y = (x.astype(np.float64) + np.float64(s) * z.astype(np.float64)).astype(F)     # the product unrounded: exact in float64
        else:
            y = (x + (s * z).astype(F)).astype(F)
        if kind == "fmin fmax":
            return np.fmin(np.fmax(y, F(lo)), F(hi)).astype(F)
        return np.where(y < F(lo), F(lo), np.where(y > F(hi), F(hi), y)).astype(F)


@pytest.mark.parametrize("kind", ("fmin fmax", "no early return", "fused"))
def test_a_wrong_disturbed_is_seen(records, kind):
    """Under at least one of the injected-row tests' disturbances the defect changes bits that same_but_for_nan_bits()
    compares: the table holds the value that shows it."""
    seen = []
    for name in EO.DISTURBANCES:
        row, z, sigma = rows(records, 3), normals(3), sigma_of(name)
        ref = records.disturb_observation(row, sigma, z)
        got = row.copy()
        for c, (lo, hi) in enumerate(records.OBSERVATION_BOX):
            got[:, 5 + c::3] = wrong(kind, row[:, 5 + c::3], sigma[c], z[..., c], lo, hi)
        if not EO.same_but_for_nan_bits(got, ref):
            seen.append(name)
    assert seen, kind
    if kind == "no early return":
        assert {"sep", "cpa", "closing", "action"} <= set(seen)


def test_check_saturated(records):
    N = 3
    row = np.random.default_rng(0).uniform(0, 1, (4096, 5 + 3 * N)).astype(F)
    row[:, 6::3] = 2 * row[:, 6::3] - 1
    row[:, 7::3] = 2 * row[:, 7::3] - 1
    z = np.random.default_rng(1).standard_normal((4096, N + 1, 3)).astype(F)
    sat = EO.SATURATING
    read = records.disturb_observation(row, (sat["sep"], sat["cpa"], sat["closing"]), z[:, 1:])
    flown = records.disturb_action(np.zeros(4096, F), sat["action"], z[:, 0, 0])
    EO.check_saturated(read, flown, records.OBSERVATION_BOX)
    with pytest.raises(AssertionError):
        EO.check_saturated(row, flown, records.OBSERVATION_BOX)                   # an undisturbed row sits at no end
