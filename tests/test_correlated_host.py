"""Time-correlated and biased errors, the parts that need no GPU: the specification in NumPy (records.correlation_gain(),
correlated_errors()) against its statistics and against three steps written out by hand, policy.CorrelatedDisturbance, the
refusals of the collectors and trainers, the command-line syntax, and the C ABI of acas2d_evaluate_policies_correlated_* /
acas2d_monte_carlo_correlated_* -- every rejection of the disturbed siblings (tests/golden/scoring_rejections.json) under the new
entries' names, then the correlation's own, with host pointers only: every case must be a rejection."""
import ctypes as C
import dataclasses
import json
import math
import os
import types
from fractions import Fraction

import numpy as np
import pytest

import scoring_rejections_support as SR

f32 = np.float32
NAN, INF = float("nan"), float("inf")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g():
    import gym_acas2d_amd as g
    return g


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- the specification ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def normals():
    z = np.random.default_rng(20261020).standard_normal((256, 4096)).astype(f32)
    z.setflags(write=False)
    return z


def test_the_limits_of_the_scan(g, normals):
    white = g.records.correlated_errors(normals, 0.0)
    assert white.dtype == f32 and np.array_equal(bits(white), bits(normals))                 # rho = 0: the input's bits
    bias = g.records.correlated_errors(normals, 1.0)
    assert np.array_equal(bits(bias), np.broadcast_to(bits(normals[0]), normals.shape))       # rho = 1: row 0 in every row


@pytest.mark.parametrize("rho", (0.5, 0.9, 0.99))
def test_unit_variance_and_the_correlation_asked_for(g, normals, rho):
    """Over 4 096 lanes: a sample variance has standard error sqrt(2 / n), a sample correlation at most 1 / sqrt(n); five of each."""
    e = g.records.correlated_errors(normals, rho).astype(np.float64)
    n = normals.shape[1]
    for row in (0, 1, 255):
        assert abs(e[row].var() - 1.0) < 5 * math.sqrt(2 / n), (row, e[row].var())
    r = np.corrcoef(e[254], e[255])[0, 1]
    assert abs(r - rho) < 5 / math.sqrt(n), r


def test_a_coefficient_per_channel(g, normals):
    """rho broadcasts against normals[0]: each column is the scan of its own coefficient."""
    z = normals[:64, :12].reshape(64, 4, 3)
    rho = np.asarray([0.9, 1.0, 0.0], f32)
    e = g.records.correlated_errors(z, rho)
    for c in range(3):
        assert np.array_equal(bits(e[..., c]), bits(g.records.correlated_errors(z[..., c], rho[c])))
    with pytest.raises(ValueError):
        g.records.correlated_errors(z, -0.1)
    with pytest.raises(ValueError):
        g.records.correlated_errors(z, NAN)


def test_the_gain(g):
    gain = g.records.correlation_gain
    assert gain(0.0) == 1.0 and gain(1.0) == 0.0 and gain(0.0).dtype == f32
    assert float(gain(f32(0.9))) == 0.43588992953300476
    for rho in (f32(0.9), f32(0.99), f32(0.5)):                        # a float64 root of the float64 1 - rho^2, rounded once
        assert float(gain(rho)) == float(f32(math.sqrt(1.0 - float(rho) * float(rho))))
    assert gain(np.asarray([0.0, 1.0], f32)).tolist() == [1.0, 0.0]
    for bad in (-0.5, 1.0000001, NAN, INF):
        with pytest.raises(ValueError):
            gain(bad)


def test_three_steps_by_hand(g):
    """e_1 = z_1; e_t = fl(fl(rho e_{t-1}) + fl(q z_t)).  The values are chosen so that at BOTH later steps the three roundings
    differ from either fused multiply-add and from the expression evaluated in float64 and rounded once."""
    rho, z = f32(0.9), [f32(0.095), f32(0.036), f32(-0.506)]
    q = f32(math.sqrt(1.0 - float(rho) * float(rho)))
    exact = lambda a, b, c: f32(float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))))  # noqa: E731  (one rounding)
    e = [z[0]]
    for t in (1, 2):
        a, b = f32(rho * e[-1]), f32(q * z[t])                         # float32 x float32 -> float32: one rounding each
        three = f32(a + b)
        assert three != exact(rho, e[-1], b) and three != exact(q, z[t], a)
        assert three != f32(float(rho) * float(e[-1]) + float(q) * float(z[t]))
        e.append(three)
    assert [int(x) for x in bits(e)] == [0x3DC28F5C, 0x3DCF3DC4, 0xBE04985E]
    got = g.records.correlated_errors(np.asarray(z, f32), rho)
    assert np.array_equal(bits(got), bits(e))
    # ... broadcast: the same three steps in every column
    assert np.array_equal(bits(g.records.correlated_errors(np.tile(np.asarray(z, f32)[:, None], (1, 5)), rho)), np.tile(bits(e)[:, None], (1, 5)))


# ---- policy.CorrelatedDisturbance ------------------------------------------------------------------------------------------------------
SIGMAS = dict(sep=0.05, cpa=0.1, closing=0.1, action=0.3, seed=7)
RHO = dict(rho_sep=0.9, rho_cpa=1.0, rho_closing=0.0, rho_action=0.5)


def test_the_class(g):
    D, W = g.CorrelatedDisturbance, g.Disturbance
    d = D.normalised(**SIGMAS, **RHO)
    assert isinstance(d, W) and d.sigma == W.normalised(**SIGMAS).sigma and d.seed == 7
    assert (d.rho_sep, d.rho_cpa, d.rho_closing, d.rho_action) == (float(f32(0.9)), 1.0, 0.0, 0.5) and d.rho == (float(f32(0.9)), 1.0, 0.0)
    # rho= is all four; one given by name overrides it
    assert D.normalised(rho=0.5) == D.normalised(rho_sep=0.5, rho_cpa=0.5, rho_closing=0.5, rho_action=0.5)
    assert D.normalised(rho=0.5, rho_cpa=1.0).rho == (0.5, 1.0, 0.5) and D.normalised(rho=0.5, rho_action=0.0).rho_action == 0.0
    # pixels through the config, as Disturbance
    assert D(sep=90, cpa=40, closing=8, action=0.1, seed=7, rho=0.9).sigma == W(sep=90, cpa=40, closing=8, action=0.1, seed=7).sigma
    # equality: the class and every field -- never a Disturbance, not even with all four 0
    assert d == D.normalised(**SIGMAS, **RHO) and hash(d) == hash(D.normalised(**SIGMAS, **RHO))
    assert d != D.normalised(**SIGMAS, **dict(RHO, rho_action=0.25)) and d != D.normalised(**dict(SIGMAS, seed=8), **RHO)
    assert D.normalised(**SIGMAS) != W.normalised(**SIGMAS) and W.normalised(**SIGMAS) != D.normalised(**SIGMAS)
    assert not d.is_zero() and D.normalised(rho=0.9, seed=3).is_zero()
    with pytest.raises(dataclasses.FrozenInstanceError):
        d.rho_sep = 0.1
    for bad in (-0.5, -1e-30, 1.0000001, NAN, INF):
        for name in D.RHO + ("rho",):
            with pytest.raises(ValueError, match=r"must lie in \[0, 1\]"):
                D.normalised(**{name: bad})


def test_round_trips(g):
    D, W = g.CorrelatedDisturbance, g.Disturbance
    d = D.normalised(**SIGMAS, **RHO)
    sd = d.to_dict()
    assert sd == dict(W.normalised(**SIGMAS).to_dict(), **{k: float(f32(v)) for k, v in RHO.items()})
    assert D.from_dict(json.loads(json.dumps(sd))) == d
    assert set(W.normalised(**SIGMAS).to_dict()) == {"s_sep", "s_cpa", "s_closing", "s_action", "seed"}    # Disturbance's stays its own
    P = D.parse
    assert P("sep=0.05,cpa=0.1,closing=0.1,action=0.3,seed=7,rho_sep=0.9,rho_cpa=1,rho_closing=0,rho_action=0.5", normalised=True) == d
    assert P("rho=0.5, sep=0.04, rho_cpa = 1", normalised=True) == D.normalised(sep=0.04, rho=0.5, rho_cpa=1.0)
    assert P("rho=0.99") == D(rho=0.99) and P("sep=90,rho=0.9,seed=0x10") == D(sep=90, rho=0.9, seed=16)
    for bad in ("rho=", "rho=0.5,rho=0.6", "rho_sep=x", "rho=0.5,speed=3", "rho=1.5"):
        with pytest.raises(ValueError):
            P(bad)
    both = d.to_c(5)
    assert isinstance(both[0], g.native.CDisturbance) and isinstance(both[1], g.native.CCorrelation) and both[0].noise_episode == 5
    assert [getattr(both[1], n) for n, _ in g.native.CCorrelation._fields_] == [float(f32(0.9)), 1.0, 0.0, 0.5]
    assert isinstance(W.normalised(**SIGMAS).to_c(5), g.native.CDisturbance)


def test_the_command_line_syntax(g):
    """A string without a rho key builds the Disturbance it has always built; the tool routes on exactly that."""
    D, W = g.CorrelatedDisturbance, g.Disturbance
    old = "sep=90,cpa=40,closing=8,action=0.1,seed=7"
    assert not D.has_rho(old) and D.has_rho(old + ",rho=0.9") and D.has_rho("rho_cpa=1") and not D.has_rho("sep=1")
    assert W.parse(old) == W(sep=90, cpa=40, closing=8, action=0.1, seed=7) and type(W.parse(old)) is W
    with pytest.raises(ValueError, match=r"sep=, cpa=, closing=, action= and seed= are understood, each once"):
        W.parse(old + ",rho=0.9")                                      # Disturbance.parse() itself is what it was
    with open(os.path.join(ROOT, "tools", "evaluate_checkpoints.py")) as f:
        tool = f.read()
    assert "CorrelatedDisturbance.has_rho(text)" in tool and "return g.policy.Disturbance(**kw)" in tool


def test_entry_names(g):
    import torch
    P = g.policy
    assert P.evaluate_policies_entry(torch.float32, False, True, correlated=True) == "acas2d_evaluate_policies_correlated_f32"
    assert P.evaluate_policies_entry(torch.float32, True, True, correlated=True) == "acas2d_evaluate_policies_correlated_group_f32"
    assert P.monte_carlo_entry(torch.float32, correlated=True) == "acas2d_monte_carlo_correlated_f32"
    assert P.monte_carlo_entry(torch.float32, True, correlated=True) == "acas2d_monte_carlo_correlated_group_f32"
    assert P.monte_carlo_entry(torch.float32, True, disturbed=True) == "acas2d_monte_carlo_disturbed_group_f32"     # as before
    for entry in (P.evaluate_policies_entry, P.monte_carlo_entry):
        with pytest.raises(ValueError, match="float32 only"):
            entry(torch.float64, correlated=True)


def test_collectors_and_trainers_are_white_noise_only(g):
    d = g.CorrelatedDisturbance.normalised(**SIGMAS, **RHO)
    white = g.Disturbance.normalised(**SIGMAS)
    for arg, K in ((d, 1), (d, 3), ([white, d], 2), ([g.CorrelatedDisturbance.normalised(**SIGMAS)] * 2, 2)):
        with pytest.raises(ValueError, match="the collectors are white-noise only"):
            g.DisturbanceSet(arg, K)
    assert len(g.DisturbanceSet([white, white], 2)) == 2               # ... and only that
    # the three trainers check their argument in _set_disturbances(), before any launch: on a float32 env it goes to DisturbanceSet
    import torch
    for cls, K in ((g.ppo.PPOTrainer, 1), (g.ppo.PopulationTrainer, 2), (g.ppo.PBTTrainer, 2)):
        trainer = cls.__new__(cls)
        trainer.venv = types.SimpleNamespace(dtype=torch.float32)
        with pytest.raises(ValueError, match="the collectors are white-noise only"):
            trainer._set_disturbances(d, K, cls.__name__)
        assert trainer.disturbances is None
        trainer._set_disturbances(white, K, cls.__name__)
        assert len(trainer.disturbances) == K


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------
CORRELATED = {e.replace("_disturbed", "_correlated"): e for e, v in SR.ENTRIES.items() if v[0] in ("dist", "mcdist")}
VALID_RHO = (0.9, 1.0, 0.0, 0.5)


def name_of(entry):
    return entry[:-len("_f32")]


def test_the_struct_and_the_exports(g):
    L = g.native.lib()
    with open(os.path.join(ROOT, "include", "acas2d.h")) as f:
        header = f.read()
    assert "typedef struct Acas2dCorrelation {" in header and "#define ACAS2D_ABI_VERSION 7" in header
    assert C.sizeof(g.native.CCorrelation) == L.acas2d_correlation_size() == 16
    assert [n for n, _ in g.native.CCorrelation._fields_] == ["rho_sep", "rho_cpa", "rho_closing", "rho_action"]
    assert len(CORRELATED) == 4
    ptr = C.POINTER(g.native.CCorrelation)
    for entry, sibling in CORRELATED.items():
        assert entry in g.native.EXPORTS and entry + "(" in header
        fn, sib = getattr(L, entry), getattr(L, sibling)
        assert fn.argtypes == sib.argtypes[:-1] + [ptr, C.c_void_p] and fn.restype == C.c_int     # the sibling's, then correlation, stream


def test_every_rejection_of_the_disturbed_sibling(g):
    """... with a VALID correlation: the same code, the same words up to the entry's own name."""
    golden = SR.golden()
    seen = 0
    for entry, sibling in CORRELATED.items():
        kind, group, Ns, bad_n = SR.ENTRIES[sibling]
        for N in Ns:
            for vid, over in SR.violations(kind, group, bad_n):
                if N == Ns[0] or any(tag in vid for tag in SR.N_DEPENDENT):
                    rc, text = SR.call(g, entry, N, over, VALID_RHO)
                    assert rc == SR.EINVAL, (entry, N, vid, rc, text)          # first: nothing may get through to a launch
                    want = golden["text"][sibling][str(N)][vid]
                    assert text == want.replace("_disturbed", "_correlated"), (entry, N, vid)
                    seen += 1
    assert seen == sum(len(v) for e in CORRELATED.values() for v in golden["text"][e].values()) > 300


BAD_RHO = (-0.5, -1e-30, 1.0000001, NAN, INF)


def test_the_correlations_own_rejections(g):
    for entry, sibling in CORRELATED.items():
        _, group, Ns, _ = SR.ENTRIES[sibling]
        for N in Ns:
            rc, text = SR.call(g, entry, N, {}, None)
            assert rc == SR.EINVAL and text == "%s: NULL correlation" % name_of(entry), (entry, N, text)
            for i in range(4):
                for bad in BAD_RHO:
                    rho = list(VALID_RHO)
                    rho[i] = bad
                    rc, text = SR.call(g, entry, N, {}, rho)
                    assert rc == SR.EINVAL, (entry, N, i, bad, rc, text)
                    shown = [float(f32(r)) for r in rho]
                    assert text == "%s: rho_sep = %g, rho_cpa = %g, rho_closing = %g, rho_action = %g (each in [0, 1])" % (
                        (name_of(entry),) + tuple(shown)), (entry, N, i, bad, text)


def test_every_shape_gets_past_the_launchers_lds_limit(g):
    """The correlation is checked last of all: a call that is turned away for its NULL correlation has passed the work shape
    and geometry_for() with the error state's LDS -- at every traffic count the entries are built for."""
    for entry, sibling in CORRELATED.items():
        group = SR.ENTRIES[sibling][1]
        for N in ((8, 16, 32, 64) if group else (1, 2, 3, 4, 8)):
            rc, text = SR.call(g, entry, N, {"n_envs": 1024, "K": 1}, None)
            assert rc == SR.EINVAL and text == "%s: NULL correlation" % name_of(entry), (entry, N, text)


def test_precedence(g):
    """A bad sigma wins over a bad rho; so does everything else the sibling rejects, down to its last check (the group entries'
    alignment); a NULL correlation and a bad rho win over nothing."""
    golden = SR.golden()
    bad_rho = (0.9, NAN, 0.0, 0.5)
    for entry, sibling in CORRELATED.items():
        kind, group, Ns, bad_n = SR.ENTRIES[sibling]
        N = Ns[0]
        late = ["s_action=nan", "null-disturbance", "max-steps-1048576", "steps-0", "traffic-0", "offset-negative", "holds-255",
                "traffic-%d" % bad_n[0], "launch-limit"] + (["misaligned-w2t", "misaligned-b1"] if group else [])
        by_id = dict(SR.violations(kind, group, bad_n))
        for vid in late:
            want = golden["text"][sibling][str(N)][vid].replace("_disturbed", "_correlated")
            for corr in (bad_rho, None):
                rc, text = SR.call(g, entry, N, by_id[vid], corr)
                assert rc == SR.EINVAL and text == want, (entry, vid, corr, text)
        # NULL in front of the values (there are none to read)
        rc, text = SR.call(g, entry, N, {}, None)
        assert rc == SR.EINVAL and text.endswith("NULL correlation")
