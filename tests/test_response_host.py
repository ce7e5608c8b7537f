"""Pilot response delay and actuation lag, the parts that need no GPU: the specification in NumPy (records.response_delay(),
response_lag(), response_gain()) on series made by hand, policy.DelayedDisturbance, the entry names, the refusals of the
collectors and trainers, the command-line syntax, and the C ABI of acas2d_evaluate_policies_delayed_* /
acas2d_monte_carlo_delayed_* -- every rejection of the disturbed siblings (tests/golden/scoring_rejections.json) under the new
entries' names, the correlation's, then the response's own, with host pointers only: every case must be a rejection."""
import ctypes as C
import dataclasses
import json
import os
import subprocess
import sys
import types
from fractions import Fraction

import numpy as np
import pytest

import scoring_rejections_support as SR

f32 = np.float32
NAN, INF = float("nan"), float("inf")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = SR.A


@pytest.fixture(scope="module")
def g():
    import gym_acas2d_amd as g
    return g


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- the specification ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def series():
    a = np.random.default_rng(20261021).uniform(-1, 1, (40, 6)).astype(f32)
    a[3, 2], a[7, 1] = -0.0, NAN                              # a sign and a NaN to carry
    a.setflags(write=False)
    return a


def test_the_dead_time(g, series):
    delay = g.records.response_delay
    assert delay(series, 0).dtype == f32 and np.array_equal(bits(delay(series, 0)), bits(series))          # 0: the input's bits
    for d in (1, 3, 39):
        out = delay(series, d)
        assert np.array_equal(bits(out[d:]), bits(series[:-d])) and not bits(out[:d]).any()                # +0.0 until it arrives
    for d in (40, 41, 32767):
        assert not bits(delay(series, d)).any()                                                            # never arrives
    assert delay(series[:, 0], 2).shape == (40,)
    for bad in (-1, 1.5):
        with pytest.raises(ValueError):
            delay(series, bad)


def test_the_limits_of_the_lag(g, series):
    lag = g.records.response_lag
    assert lag(series, 0.0).dtype == f32 and np.array_equal(bits(lag(series, 0.0)), bits(series))          # 0: the input's bits
    finite = np.where(np.isnan(series), f32(0.25), series)
    assert not bits(lag(finite, 1.0)).any()                                                                # 1: gain 0, u stays +0.0
    for bad in (-0.5, 1.0000001, NAN, INF):
        with pytest.raises(ValueError):
            lag(series, bad)
    # one step of it, with a state that outlives the call: `first` puts 0 in the held value's place
    step = g.records.response_lag_step
    u = lag(finite, 0.75)
    assert np.array_equal(bits(step(u[4], finite[5], 0.75, False)), bits(u[5]))
    assert np.array_equal(bits(step(u[4], finite[0], 0.75, True)), bits(u[0]))
    assert np.array_equal(bits(step(u[4], finite[5], 0.0, False)), bits(finite[5]))


def test_the_gain(g):
    gain = g.records.response_gain
    assert gain(0.0) == 1.0 and gain(1.0) == 0.0 and gain(0.5) == 0.5 and type(gain(0.5)) is f32
    for lam in (f32(0.9), f32(0.75), f32(0.1), f32(1e-9)):          # the float64 difference (exact), rounded once
        assert float(gain(lam)) == float(f32(float(Fraction(1) - Fraction(float(lam)))))
    assert float(gain(f32(0.9))) == 0.10000002384185791


def test_a_step_input_through_half_a_lag_by_hand(g):
    """u_s = fl(fl(0.5 u_{s-1}) + fl(0.5 x 1)): 1 - 2^-(s+1), exact in float32 for 24 steps, then 1 for good."""
    u = g.records.response_lag(np.ones(30, f32), 0.5)
    assert u.dtype == f32 and u[:4].tolist() == [0.5, 0.75, 0.875, 0.9375]
    assert [float(x) for x in u[:24]] == [1.0 - 2.0 ** -(s + 1) for s in range(24)]
    assert (u[24:] == 1.0).all()                                                # 1 - 2^-25 rounds to 1 (a tie, to even)
    # ... and behind a dead time of two steps
    late = g.records.response_lag(g.records.response_delay(np.ones(6, f32), 2), 0.5)
    assert late.tolist() == [0.0, 0.0, 0.5, 0.75, 0.875, 0.9375]
    # a pole that is no power of two, the three roundings written out: u_s = fl(fl(lam u_{s-1}) + fl(g c_s)), u_0 from u = 0
    lam, c = f32(0.9), [f32(0.095), f32(0.036), f32(-0.506)]
    gn = f32(1.0 - float(lam))
    want = [f32(f32(lam * f32(0)) + f32(gn * c[0]))]
    for s in (1, 2):
        want.append(f32(f32(lam * want[-1]) + f32(gn * c[s])))
    assert [int(x) for x in bits(want)] == [0x3C1BA5E6, 0x3C4710CE, 0xBD2277C7]
    assert np.array_equal(bits(g.records.response_lag(np.asarray(c, f32), lam)), bits(want))


def test_the_clamp_engages(g):
    """Commands inside [-1, 1] cannot leave the box: fl(lam u) + fl(g c) <= lam + g <= 1 + 2^-25, which rounds to 1.  The clamp is
    for what is not inside: a command built so that the sum rounds above 1, and a NaN."""
    lag, step = g.records.response_lag, g.records.response_lag_step
    c = f32(1) + f32(2.0 ** -22)
    raw = f32(f32(f32(0.5) * f32(1)) + f32(f32(0.5) * c))               # u_{s-1} = 1: 0.5 + (0.5 + 2^-23) = 1 + 2^-23, one ulp above 1
    assert raw > 1 and float(raw) == float(np.nextafter(f32(1), f32(2)))
    assert bits(step(np.asarray([1.0, -1.0], f32), np.asarray([c, -c], f32), 0.5, False)).tolist() == bits([1.0, -1.0]).tolist()
    u = lag(np.asarray([1.0] * 25 + [c], f32), 0.5)
    assert u[24] == 1.0 and u[25] == 1.0
    assert lag(np.asarray([3.0, -3.0, 3.0], f32), 0.5).tolist() == [1.0, -1.0, 1.0]       # 1.5; -0.5 - 1.5; 0.5 + 1.5
    # a NaN command: fmin(fmax(NaN, -1), 1) = -1, as fminf(fmaxf()) gives -- and the state goes on from there
    assert lag(np.asarray([1.0, NAN, 1.0], f32), 0.5).tolist() == [0.5, -1.0, 0.0]


# ---- policy.DelayedDisturbance ---------------------------------------------------------------------------------------------------------
SIGMAS = dict(sep=0.05, cpa=0.1, closing=0.1, action=0.3, seed=7)
RHO = dict(rho_sep=0.9, rho_cpa=1.0, rho_closing=0.0, rho_action=0.5)


def test_the_class(g):
    D, Cd, W = g.DelayedDisturbance, g.CorrelatedDisturbance, g.Disturbance
    d = D.normalised(**SIGMAS, **RHO, delay=50, lag=0.9)
    assert isinstance(d, Cd) and isinstance(d, W) and d.sigma == W.normalised(**SIGMAS).sigma and d.rho == Cd.normalised(**RHO).rho
    assert (d.delay, d.lag) == (50, float(f32(0.9))) and type(d.delay) is int
    assert D(sep=90, rho=0.9, delay=3).sigma == W(sep=90).sigma and D(delay=3, lag=0.5).is_zero()
    # equality: the class and every field -- never one of its bases, not even with delay 0 and lag 0
    assert d == D.normalised(**SIGMAS, **RHO, delay=50, lag=0.9) and hash(d) == hash(D.normalised(**SIGMAS, **RHO, delay=50, lag=0.9))
    assert d != D.normalised(**SIGMAS, **RHO, delay=49, lag=0.9) and d != D.normalised(**SIGMAS, **RHO, delay=50, lag=0.5)
    for base in (Cd.normalised(**SIGMAS, **RHO), ):
        assert D.normalised(**SIGMAS, **RHO) != base and base != D.normalised(**SIGMAS, **RHO)
    assert D.normalised(**SIGMAS) != W.normalised(**SIGMAS) and W.normalised(**SIGMAS) != D.normalised(**SIGMAS)
    with pytest.raises(dataclasses.FrozenInstanceError):
        d.delay = 1
    for bad in (-1, 32768, 1.5, NAN, True):
        with pytest.raises(ValueError, match="delay = "):
            D.normalised(delay=bad)
    for bad in (-0.5, -1e-30, 1.0000001, NAN, INF):
        with pytest.raises(ValueError, match=r"the lag must lie in \[0, 1\]"):
            D.normalised(lag=bad)
    assert D.normalised(delay=32767, lag=1.0).delay == 32767 and D.normalised(delay=2.0).delay == 2


def test_round_trips(g):
    D, Cd = g.DelayedDisturbance, g.CorrelatedDisturbance
    d = D.normalised(**SIGMAS, **RHO, delay=50, lag=0.9)
    sd = d.to_dict()
    assert sd == dict(Cd.normalised(**SIGMAS, **RHO).to_dict(), delay=50, lag=float(f32(0.9)))
    assert D.from_dict(json.loads(json.dumps(sd))) == d
    assert "delay" not in Cd.normalised(**SIGMAS, **RHO).to_dict()                                  # the base's stays its own
    P = D.parse
    assert P("sep=0.05,cpa=0.1,closing=0.1,action=0.3,seed=7,rho_sep=0.9,rho_cpa=1,rho_closing=0,rho_action=0.5,delay=50,lag=0.9",
             normalised=True) == d
    assert P("delay=50") == D(delay=50) and P("lag = 0.5, sep=90") == D(sep=90, lag=0.5) and P("rho=0.9,delay=0x10") == D(rho=0.9, delay=16)
    for bad in ("delay=", "delay=5,delay=6", "lag=x", "delay=2.5", "delay=5,speed=3", "lag=1.5", "delay=-1"):
        with pytest.raises(ValueError):
            P(bad)
    three = d.to_c(5)
    assert [type(c) for c in three] == [g.native.CDisturbance, g.native.CCorrelation, g.native.CResponse] and three[0].noise_episode == 5
    assert (three[2].delay_steps, three[2].lag, three[2].ring, three[2].ring_envs) == (50, float(f32(0.9)), None, 0)
    assert len(Cd.normalised(**SIGMAS, **RHO).to_c(5)) == 2


def test_the_command_line_syntax(g):
    D = g.DelayedDisturbance
    old = "sep=90,cpa=40,rho=0.9,seed=7"
    assert not D.has_response(old) and D.has_response(old + ",delay=50") and D.has_response("lag=0.5") and not D.has_response("sep=1")
    with pytest.raises(ValueError, match="are understood, each once"):
        g.CorrelatedDisturbance.parse(old + ",delay=50")             # CorrelatedDisturbance.parse() itself is what it was
    with open(os.path.join(ROOT, "tools", "evaluate_checkpoints.py")) as f:
        tool = f.read()
    assert "DelayedDisturbance.has_response(text)" in tool and tool.index("has_response(text)") < tool.index("has_rho(text)")


def test_the_training_tool_refuses_a_delay():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_ppo.py"), "--collector", "fused", "--disturbance",
                        "sep=90,delay=50"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 2 and "the collectors know no response delay or lag" in r.stderr, r.stderr[-400:]


def test_entry_names(g):
    import torch
    P = g.policy
    for group, sfx in ((False, "_f32"), (True, "_group_f32")):
        assert P.evaluate_policies_entry(torch.float32, group, True, disturbed=True, delayed=True) == "acas2d_evaluate_policies_delayed" + sfx
        assert P.monte_carlo_entry(torch.float32, group, disturbed=True, delayed=True) == "acas2d_monte_carlo_delayed" + sfx
        assert P.monte_carlo_entry(torch.float32, group, delayed=True) == "acas2d_monte_carlo_delayed" + sfx
        # ... and the others as before
        assert P.evaluate_policies_entry(torch.float32, group, True, disturbed=True, correlated=True) == "acas2d_evaluate_policies_correlated" + sfx
        assert P.monte_carlo_entry(torch.float32, group, disturbed=True) == "acas2d_monte_carlo_disturbed" + sfx
        assert P.evaluate_policies_entry(torch.float32, group, True) == "acas2d_evaluate_policies_stats" + sfx
        assert P.monte_carlo_entry(torch.float32, group) == "acas2d_monte_carlo" + sfx
    assert P.monte_carlo_entry(torch.float64) == "acas2d_monte_carlo_f64"
    for entry in (P.evaluate_policies_entry, P.monte_carlo_entry):
        with pytest.raises(ValueError, match="float32 only"):
            entry(torch.float64, delayed=True)


def test_collectors_and_trainers_refuse_it(g):
    d = g.DelayedDisturbance.normalised(**SIGMAS, **RHO, delay=5, lag=0.75)
    white = g.Disturbance.normalised(**SIGMAS)
    for arg, K in ((d, 1), (d, 3), ([white, d], 2), ([g.DelayedDisturbance.normalised(**SIGMAS)] * 2, 2)):
        with pytest.raises(ValueError, match="the collectors are white-noise only"):
            g.DisturbanceSet(arg, K)
        with pytest.raises(ValueError, match="the collectors know no response delay or lag"):
            g.CorrelatedDisturbanceSet(arg, K)
    assert len(g.CorrelatedDisturbanceSet([white, g.CorrelatedDisturbance.normalised(**SIGMAS, **RHO)], 2)) == 2      # ... and only that
    import torch
    for cls, K in ((g.ppo.PPOTrainer, 1), (g.ppo.PopulationTrainer, 2), (g.ppo.PBTTrainer, 2)):
        trainer = cls.__new__(cls)
        trainer.venv = types.SimpleNamespace(dtype=torch.float32)
        with pytest.raises(ValueError, match="the collectors are white-noise only"):
            trainer._set_disturbances(d, K, cls.__name__)
        assert trainer.disturbances is None
    # collect(disturbance=): the env turns its argument into a DisturbanceSet in front of everything that needs a device
    v = types.SimpleNamespace(dtype=torch.float32)
    with pytest.raises(ValueError, match="the collectors are white-noise only"):
        g.ACAS2DVecEnv._disturbed_entry(v, "collect", d, 1, False)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------
DELAYED = {e.replace("_disturbed", "_delayed"): e for e, v in SR.ENTRIES.items() if v[0] in ("dist", "mcdist")}
VALID_RHO = (0.9, 1.0, 0.0, 0.5)
VALID_RESPONSE = (5, 0.75, A, 256)                              # delay_steps, lag, ring, ring_envs: the valid call covers 256 envs


def name_of(entry):
    return entry[:-len("_f32")]


def call(g, entry, N, over, corr=VALID_RHO, resp=VALID_RESPONSE):
    """scoring_rejections_support.call() for a *_delayed_* entry: its disturbed sibling's call with two more arguments in front
    of the stream -- `corr`, the four rho, and `resp`, Acas2dResponse's four fields; None for a NULL pointer."""
    nat, L = g.native, g.native.lib()
    kind = SR.ENTRIES[DELAYED[entry]][0]
    fn = getattr(L, entry)
    if over is None:
        rc = fn(*([None, None, 0, None, 0, 0, None, 0, 0, 0, 0] + [None] * (len(fn.argtypes) - 11)))
        return rc, L.acas2d_last_error().decode()
    s = {"cfg": g.ACAS2DConfig(n_traffic=N).to_c(), "state": nat.CState(*([A] * 14)), "policies": nat.CPolicy(*([A] * 6), 64, 0),
         "stats": nat.CEvalStats(*([A] * 6)), "mc": nat.CMonteCarlo(*([A] * 9), 16, 2, 0.02, 0, 0),
         "dist": nat.CDisturbance(0.05, 0.1, 0.1, 0.3, 7, 5, 0)}
    top = dict({k: True for k in s}, n_envs=256, K=2, count=100, obs=A, T=2000 if kind == "mcdist" else 10, n=N, off=0,
               outcome=A, steps=A, ret=A)
    for k, val in over.items():
        if "." in k:
            setattr(s[k.split(".")[0]], k.split(".")[1], val)
        else:
            assert k in top, k
            top[k] = val
    ref = lambda k: None if top[k] is None else C.byref(s[k])  # noqa: E731
    tail = ("mc", "dist") if kind == "mcdist" else ("stats", "dist")
    outs = [] if kind == "mcdist" else [top["outcome"], top["steps"], top["ret"]]
    rc = fn(ref("cfg"), ref("state"), top["n_envs"], ref("policies"), top["K"], top["count"], top["obs"], top["T"], 13, top["off"],
            top["n"], *outs, *[ref(k) for k in tail], None if corr is None else C.byref(nat.CCorrelation(*corr)),
            None if resp is None else C.byref(nat.CResponse(*resp)), None)
    return rc, L.acas2d_last_error().decode()


def test_the_struct_and_the_exports(g):
    L = g.native.lib()
    with open(os.path.join(ROOT, "include", "acas2d.h")) as f:
        header = f.read()
    assert "typedef struct Acas2dResponse {" in header and "#define ACAS2D_ABI_VERSION 7" in header
    assert C.sizeof(g.native.CResponse) == L.acas2d_response_size() == 24
    assert [n for n, _ in g.native.CResponse._fields_] == ["delay_steps", "lag", "ring", "ring_envs"]
    assert len(DELAYED) == 4
    for entry, sibling in DELAYED.items():
        assert entry in g.native.EXPORTS and entry + "(" in header
        fn, sib = getattr(L, entry), getattr(L, sibling.replace("_disturbed", "_correlated"))
        assert fn.argtypes == sib.argtypes[:-1] + [C.POINTER(g.native.CResponse), C.c_void_p] and fn.restype == C.c_int


def test_every_rejection_of_the_siblings(g):
    """... with a VALID correlation and response: the same code, the same words up to the entry's own name."""
    golden = SR.golden()
    seen = 0
    for entry, sibling in DELAYED.items():
        kind, group, Ns, bad_n = SR.ENTRIES[sibling]
        for N in Ns:
            for vid, over in SR.violations(kind, group, bad_n):
                if N == Ns[0] or any(tag in vid for tag in SR.N_DEPENDENT):
                    rc, text = call(g, entry, N, over)
                    assert rc == SR.EINVAL, (entry, N, vid, rc, text)          # first: nothing may get through to a launch
                    assert text == golden["text"][sibling][str(N)][vid].replace("_disturbed", "_delayed"), (entry, N, vid)
                    seen += 1
    assert seen == sum(len(v) for e in DELAYED.values() for v in golden["text"][e].values()) > 300
    # ... and the correlation's, behind them and in front of the response's
    for entry in DELAYED:
        N = SR.ENTRIES[DELAYED[entry]][2][0]
        for resp in (VALID_RESPONSE, None, (-1, NAN, None, 0)):
            rc, text = call(g, entry, N, {}, None, resp)
            assert rc == SR.EINVAL and text == "%s: NULL correlation" % name_of(entry), (entry, text)
            rc, text = call(g, entry, N, {}, (0.9, NAN, 0.0, 0.5), resp)
            assert rc == SR.EINVAL and text == "%s: rho_sep = 0.9, rho_cpa = nan, rho_closing = 0, rho_action = 0.5 (each in [0, 1])" % \
                name_of(entry), (entry, text)


def test_the_responses_own_rejections(g):
    for entry, sibling in DELAYED.items():
        name = name_of(entry)
        for N in SR.ENTRIES[sibling][2]:
            cases = [(None, "%s: NULL response" % name)]
            cases += [((d, 0.75, A, 256), "%s: delay_steps = %d (0 to 32767)" % (name, d)) for d in (-1, -2 ** 31, 32768, 2 ** 31 - 1)]
            cases += [((5, lag, A, 256), "%s: lag = %g (in [0, 1])" % (name, float(f32(lag)))) for lag in (-0.5, -1e-30, 1.0000001, NAN, INF)]
            cases += [((d, 0.75, None, 256), "%s: NULL ring with delay_steps = %d (float[delay_steps][ring_envs], on the device)" % (name, d))
                      for d in (1, 32767)]
            cases += [((5, 0.75, A, envs), "%s: ring_envs = %d, the launch covers 256 envs" % (name, envs)) for envs in (255, 0, -1, 128)]
            # which wins: the delay over the lag, the lag over the ring, the ring's pointer over its size
            cases += [((-1, NAN, None, 0), "%s: delay_steps = -1 (0 to 32767)" % name), ((5, NAN, None, 0), "%s: lag = nan (in [0, 1])" % name),
                      ((5, 0.75, None, 0), "%s: NULL ring with delay_steps = 5 (float[delay_steps][ring_envs], on the device)" % name)]
            for resp, want in cases:
                rc, text = call(g, entry, N, {}, VALID_RHO, resp)
                assert rc == SR.EINVAL and text == want, (entry, N, resp, rc, text)
        # the launch's env total is n_policies x the count rounded up to 64, not the state's n_envs
        rc, text = call(g, entry, SR.ENTRIES[sibling][2][0], {"n_envs": 1024, "K": 3, "count": 65}, VALID_RHO, (5, 0.75, A, 383))
        assert rc == SR.EINVAL and text == "%s: ring_envs = 383, the launch covers 384 envs" % name, text


def test_every_shape_gets_past_the_launchers_lds_limit(g):
    """The response is checked last of all: a call that is turned away for its NULL response has passed the work shape and
    geometry_for() with the error state's and the lag's LDS -- at every traffic count the entries are built for."""
    for entry, sibling in DELAYED.items():
        group = SR.ENTRIES[sibling][1]
        for N in ((8, 16, 32, 64) if group else (1, 2, 3, 4, 8)):
            rc, text = call(g, entry, N, {"n_envs": 1024, "K": 1}, VALID_RHO, None)
            assert rc == SR.EINVAL and text == "%s: NULL response" % name_of(entry), (entry, N, text)


def test_precedence(g):
    """Everything the siblings reject wins over a bad response, down to their last checks (the group entries' alignment, the
    correlation); a NULL response and a bad one win over nothing."""
    golden = SR.golden()
    for entry, sibling in DELAYED.items():
        kind, group, Ns, bad_n = SR.ENTRIES[sibling]
        N = Ns[0]
        late = ["s_action=nan", "null-disturbance", "max-steps-1048576", "steps-0", "traffic-0", "offset-negative", "holds-255",
                "traffic-%d" % bad_n[0], "launch-limit"] + (["misaligned-w2t", "misaligned-b1"] if group else [])
        by_id = dict(SR.violations(kind, group, bad_n))
        for vid in late:
            want = golden["text"][sibling][str(N)][vid].replace("_disturbed", "_delayed")
            for resp in ((-1, NAN, None, 0), None):
                rc, text = call(g, entry, N, by_id[vid], VALID_RHO, resp)
                assert rc == SR.EINVAL and text == want, (entry, vid, resp, text)
