"""Hand-placed entries for the row the noise collectors read (acas2d_collect_set_disturbed_*, acas2d_collect_set_correlated_*):
the values of tests/test_collect_disturbed.py's and tests/test_collect_correlated.py's injected-row tests, the disturbances
they are read under, and what the reference must show before a kernel is looked at.  No GPU is needed here: everything is
NumPy (tests/test_disturbance_host.py admits the table on the CPU).

The device function disturbed() forms x + s z with two roundings and holds it to the channel's box by comparisons: a NaN stays
a NaN, -0 stays -0, and a channel with s == 0 is neither added to nor clamped.  The reset and a well-behaved scene give
entries inside the box that are none of these, so the table puts them there by hand -- the simulator does produce them
(traffic abeam on a parallel course: sep 1.19, d_cpa NaN, closing -0; head-on at 7 000 px: d_cpa 3.71; a coincident aircraft:
sep 0 and two NaN).

values(lo, hi), per channel of records.OBSERVATION_BOX, NAMES in order:
  both ends of the box, nextafter of each end outwards and inwards, +0 and -0, the smallest denormal of either sign, +-1.5,
  +-FLT_MAX, +-inf and a quiet NaN  (the separation's lower end IS +0 and its neighbours ARE the denormals: kept, the
  rotation counts positions).
inject(obs, boxes, shift) writes value (i + 5 n + 7 c + shift) % 17 of channel c's list into entry 5 + 3 n + c of env i: over
17 or more envs every value meets every channel of every traffic slot, neighbours in a row differ, and `shift` gives a later
launch another row.  The own-ship five stay as they are.

DISTURBANCES: one channel at a time at 0.1 with the other three exactly 0 (the last, "action", never enters the sensor gate),
"saturating" (2 / 4 / 4 / 4: most entries leave the box), "vanishing" (all 1e-30: nothing is added to an ordinary entry and
everything is clamped) and "overflowing" (all FLT_MAX: s z is +-inf wherever |z| > 1, and inf - inf generates NaN)."""
import numpy as np

F = np.float32
FLT_MAX = F(np.finfo(F).max)
DENORMAL = np.nextafter(F(0), F(1))
NAMES = ("lo", "hi", "below lo", "above lo", "below hi", "above hi", "+0", "-0", "+denormal", "-denormal", "+1.5", "-1.5",
         "+FLT_MAX", "-FLT_MAX", "+inf", "-inf", "NaN")
V = len(NAMES)
SEED = 7
SATURATING = dict(sep=2.0, cpa=4.0, closing=4.0, action=4.0)
DISTURBANCES = {
    "sep": dict(sep=0.1, cpa=0.0, closing=0.0, action=0.0),
    "cpa": dict(sep=0.0, cpa=0.1, closing=0.0, action=0.0),
    "closing": dict(sep=0.0, cpa=0.0, closing=0.1, action=0.0),
    "action": dict(sep=0.0, cpa=0.0, closing=0.0, action=0.1),
    "saturating": SATURATING,
    "vanishing": dict(sep=1e-30, cpa=1e-30, closing=1e-30, action=1e-30),
    "overflowing": dict(sep=float(FLT_MAX), cpa=float(FLT_MAX), closing=float(FLT_MAX), action=float(FLT_MAX)),
}


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def values(lo, hi):
    lo, hi, inf = F(lo), F(hi), F(np.inf)
    v = np.array([lo, hi, np.nextafter(lo, -inf), np.nextafter(lo, inf), np.nextafter(hi, -inf), np.nextafter(hi, inf),
                  0.0, -0.0, DENORMAL, -DENORMAL, 1.5, -1.5, FLT_MAX, -FLT_MAX, inf, -inf, np.nan], F)
    assert v.shape == (V,)
    return v


def table(boxes):
    """[3, V]: channel c's values."""
    return np.stack([values(lo, hi) for lo, hi in boxes])


def value_index(E, N, shift=0):
    """[E, N, 3]: which of the V values entry (env, traffic slot, channel) takes."""
    i, n, c = np.ogrid[:E, :N, :3]
    return (i + 5 * n + 7 * c + shift) % V


def inject(obs, boxes, shift=0):
    """A copy of the rows obs [E, 5 + 3 N] with every traffic entry replaced from the table."""
    out = np.array(obs, F, copy=True)
    E, N = out.shape[0], (out.shape[1] - 5) // 3
    assert out.ndim == 2 and out.shape[1] == 5 + 3 * N and E >= V, out.shape
    out[:, 5:] = table(boxes)[np.arange(3), value_index(E, N, shift)].reshape(E, 3 * N)
    return out


def check_reference(row, ref, sigma, boxes, vanishing=False):
    """What records.disturb_observation() must have made of an injected row, asserted on the reference alone:
      a channel with sigma 0 is the injected bits everywhere -- out-of-box values, -0, +-inf and the NaN included;
      in a channel with sigma != 0 every entry that is no NaN lies in the box, every injected NaN is still one, and both ends
      of the box are taken;
      vanishing: the entries that were inside the box and are neither zero nor a denormal keep their bits."""
    for c, (lo, hi) in enumerate(boxes):
        x, y = row[:, 5 + c::3], ref[:, 5 + c::3]
        if sigma[c] == 0:
            assert np.array_equal(bits(y), bits(x)), c
            continue
        nan = np.isnan(y)
        assert np.isnan(x).any() and nan[np.isnan(x)].all(), c
        assert ((y[~nan] >= F(lo)) & (y[~nan] <= F(hi))).all(), c
        assert (y == F(lo)).any() and (y == F(hi)).any(), c
        if vanishing:
            keep = (x >= F(lo)) & (x <= F(hi)) & (np.abs(x) >= np.finfo(F).tiny)
            assert keep.any() and np.array_equal(bits(y[keep]), bits(x[keep])), c


def check_saturated(read, flown, boxes):
    """Teeth of the saturating disturbance, on a reference's rows alone: read [..., 5 + 3 N] as the actor read them, flown
    [...] as the env was sent.  In each sensor channel at least 10 % of the entries sit at each end of the box and at least
    5 % strictly inside (for a true entry inside its box the normal distribution gives at least 31 % and 17 %: sigma is twice
    the box's width); at least 10 % of the flown actions are exactly +1 and at least 10 % exactly -1."""
    for c, (lo, hi) in enumerate(boxes):
        x = np.asarray(read)[..., 5 + c::3]
        at_lo, at_hi, inside = (x == F(lo)).mean(), (x == F(hi)).mean(), ((x > F(lo)) & (x < F(hi))).mean()
        assert at_lo >= 0.10 and at_hi >= 0.10 and inside >= 0.05, (c, at_lo, at_hi, inside)
    up, down = (np.asarray(flown) == F(1)).mean(), (np.asarray(flown) == F(-1)).mean()
    assert up >= 0.10 and down >= 0.10, (up, down)


def same_but_for_nan_bits(got, ref):
    """Bit for bit, but where the reference entry is a NaN any NaN will do: inf - inf GENERATES one, and a generated NaN's sign
    differs between x86 and the GPU (tests/test_gae_kernel.py, make_inputs)."""
    got, ref = np.asarray(got), np.asarray(ref)
    nan = np.isnan(ref)
    return (got.dtype == ref.dtype == F and got.shape == ref.shape and bool(np.isnan(got[nan]).all()) and
            np.array_equal(bits(got[~nan]), bits(ref[~nan])))
