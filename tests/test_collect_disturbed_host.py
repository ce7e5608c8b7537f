"""Training under sensor and actuator noise, host side (no GPU): the two disturbed set-collector entries in the header, the
loader and the built library; their argument validation (every pointer below is a host address: the calls are refused
before any launch); what Python refuses before it calls them -- a bad standard deviation (the rows live on the device, where
the C entry cannot look), unequal seeds, a trainer whose collector is not the fused one; the disturbance in a trainer's
state; and the --disturbance syntax of tools/train_ppo.py."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("acas2d_collect_set_disturbed_f32", "acas2d_collect_set_disturbed_group_f32")


@pytest.fixture(scope="module")
def g():
    import gym_acas2d_amd as g
    return g


def test_symbols_header_and_loader(g):
    L = g.native.lib()
    header = open(os.path.join(ROOT, "include", "acas2d.h")).read()
    assert "#define ACAS2D_ABI_VERSION 7" in header and L.acas2d_abi_version() == 7          # additive
    for name in ENTRIES:
        assert name in g.native.EXPORTS and hasattr(L, name)
        assert ("int %s(const Acas2dConfig *cfg" % name) in header
        # the sibling's arguments, then sigmas, dist_seed and obs_read in front of the stream
        sib = getattr(L, name.replace("_disturbed", "")).argtypes
        assert list(getattr(L, name).argtypes) == list(sib[:-1]) + [C.c_void_p, C.c_uint64, C.c_void_p, sib[-1]]
    # a standard deviation on the device is the caller's to check: the header says so
    assert "the CALLER makes sure each is finite and at least 0" in header


CASES = ((ENTRIES[0], 1, 16, "no thread-per-env shape"), (ENTRIES[0], 8, 5, "no thread-per-env shape"),
         (ENTRIES[1], 16, 3, "use acas2d_collect_set_f32"), (ENTRIES[1], 64, 5, "has no packed work shape"))


@pytest.mark.parametrize("entry,N,badN,bad_msg", CASES, ids=["%s-N%d" % (c[0][7:-4], c[1]) for c in CASES])
def test_validation_needs_no_gpu(g, entry, N, badN, bad_msg):
    """Everything the sibling refuses, under the entry's own name -- but one member takes any n_envs; a NULL sigmas or obs_read;
    obs_read overlapping io->obs or obs_in; max_steps + 1 >= 2^20."""
    L = g.native.lib()
    D, T, E = 5 + 3 * N, 4, 128
    row = E * D * 4
    buf = (C.c_char * (row * (3 * T + 8) + 65536))()
    a = (C.addressof(buf) + 255) // 256 * 256
    obs_in, obs, obs_read = a + 4096, a + 4096 + row, a + 4096 + row * (T + 1)        # adjoining, none overlapping
    far = obs_read + (1 << 30)
    st = g.native.CState(*([a] * 14), None)
    fn = getattr(L, entry)
    cfg = g.ACAS2DConfig(n_traffic=N).to_c()
    name = entry[:-4]

    def io(**kw):
        f = dict(actions=a, obs=obs, reward=a, done=a, outcome=a, term_obs=None, ep_return=a, ep_steps=a)
        f.update(kw)
        return g.native.CStepIO(**f)

    def ac(hidden=64, **kw):
        pol = {n: a for n, _ in g.native.CPolicy._fields_[:6]}
        pol.update({k: v for k, v in kw.items() if k in pol})
        f = {n: a for n, _ in g.native.CActorCritic._fields_[1:10]}
        f.update({k: v for k, v in kw.items() if k in f})
        return g.native.CActorCritic(g.native.CPolicy(**pol, hidden=hidden, _pad=0), **f, noise_seed=0, noise_step=0, _pad=0)

    def call(cfg_=C.byref(cfg), state=C.byref(st), io_=None, ac_=None, K=2, keys=a, obs_in_=obs_in, T_=T, off=0, n_envs=E, n=N,
             sigmas=a, seed=7, read=obs_read, null_io=False, null_ac=False):
        return fn(cfg_, state, None if null_io else C.byref(io_ or io()), None if null_ac else C.byref(ac_ or ac()), K, keys, obs_in_,
                  T_, 13, off, n_envs, n, sigmas, seed, read, None)

    def rejects(msg, **kw):
        assert call(**kw) == -22, kw
        assert msg.encode() in L.acas2d_last_error(), (kw, L.acas2d_last_error())

    # its own
    rejects(name + ": NULL sigmas", sigmas=None)
    rejects(name + ": NULL sigmas", read=None)
    for read in (obs, obs + row * T - 4, obs - row * (T + 1) + 4,       # io->obs: its first bytes, its last, obs_read's last on its first
                 obs_in, obs_in + row - 4, obs_in - row * (T + 1) + 4):   # obs_in likewise
        rejects(name + ": obs_read overlaps io->obs or obs_in", read=read)
    for max_steps, refused in (((1 << 20) - 1, True), (1 << 20, True), (0x7FFFFFFF, True), ((1 << 20) - 2, False)):
        big = g.ACAS2DConfig(n_traffic=N, max_steps=max_steps).to_c()
        # (n = badN: the admissible max_steps passes this check and is stopped by the shape, before a launch; `far`: rows of
        #  another width do not overlap either -- no address here is ever read)
        assert call(cfg_=C.byref(big), n=badN, read=far) == -22
        assert (b"the step field of the noise counter" in L.acas2d_last_error()) == refused, (max_steps, L.acas2d_last_error())
    # one member: any n_envs (stopped by the shape, before a launch); two: the sibling's rule
    assert call(K=1, n_envs=70, n=badN, read=far) == -22 and bad_msg.encode() in L.acas2d_last_error(), L.acas2d_last_error()
    rejects("n_envs = 70 is not n_members = 2 x a multiple of 64", n_envs=70)
    rejects("n_envs = 192 is not n_members = 2 x a multiple of 64", n_envs=192)
    # the sibling's
    rejects(bad_msg, n=badN, read=far)
    rejects(name + ": NULL cfg / io / actor-critic", cfg_=None)
    rejects(name + ": NULL cfg / io / actor-critic", null_io=True)
    rejects(name + ": NULL cfg / io / actor-critic", null_ac=True)
    rejects("NULL state", state=None)
    rejects("obs_in, actions (output), obs, reward, done and outcome are required", obs_in_=None)
    for f in ("actions", "obs", "reward", "done", "outcome"):
        rejects("obs_in, actions (output), obs, reward, done and outcome are required", io_=io(**{f: None}))
    for w in ("w1t", "b1", "w2t", "b2", "w3", "b3"):
        rejects("six weight buffers", ac_=ac(**{w: None}))
    rejects("got hidden = 32", ac_=ac(32))
    for w in ("v1t", "vb1", "v2t", "vb2", "v3", "vb3", "log_std", "values", "logp"):
        rejects("the value net's stacks, log_std, values and logp are required", ac_=ac(**{w: None}))
    rejects(name + ": NULL noise_seeds", keys=None)
    rejects("n_members = 0", K=0)
    rejects("n_traffic = 0", n=0)
    rejects("n_steps = 0", T_=0)
    rejects("negative n_envs / env_offset", off=-1)
    rejects("negative n_envs / env_offset", n_envs=-128)
    if "group" in entry:
        rejects("16-byte aligned", ac_=ac(w2t=a + 4))
        rejects("16-byte aligned", ac_=ac(vb1=a + 8))
    assert call(n_envs=0) == 0                               # nothing to do, nothing launched


def test_python_refuses_bad_sigmas_and_unequal_seeds(g):
    D = g.Disturbance.normalised
    for field in ("sep", "cpa", "closing", "action"):
        for bad in (-0.5, -1e-30, float("nan"), float("inf"), -float("inf")):
            with pytest.raises(ValueError, match="finite and at least 0"):
                g.DisturbanceSet(D(**{field: bad}), 1)
            with pytest.raises(ValueError, match="member 1"):
                g.DisturbanceSet([D(), D(**{field: bad})], 2)
    with pytest.raises(ValueError, match="EQUAL seeds"):
        g.DisturbanceSet([D(sep=0.1, seed=7), D(sep=0.2, seed=8)], 2)
    with pytest.raises(ValueError, match="got 3 for 2"):
        g.DisturbanceSet([D()] * 3, 2)
    with pytest.raises(TypeError):
        g.DisturbanceSet([D(), 0.5], 2)
    # what it accepts: one for all, or one per member with equal seeds; the rows are the kernel's float32s
    one = g.DisturbanceSet(D(sep=0.05, cpa=0.04, closing=0.03, action=0.2, seed=9), 3)
    assert one.rows.shape == (3, 4) and one.rows.dtype == np.float32 and one.seed == 9 and len(one) == 3
    assert one.rows[2].tolist() == [np.float32(0.05), np.float32(0.04), np.float32(0.03), np.float32(0.2)]
    sweep = g.DisturbanceSet([D(seed=9), D(sep=0.05, seed=9), D(action=0.4, seed=9)], 3)
    assert sweep.rows[:, 0].tolist() == [0.0, np.float32(0.05), 0.0] and sweep.rows[2, 3] == np.float32(0.4)
    assert not sweep.is_zero() and g.DisturbanceSet(D(seed=3), 2).is_zero()


class _Venv:
    """What PPOTrainer.__init__ reads of an env before it refuses a collector (no GPU)."""
    device, dtype, n_traffic, obs_dim, num_envs = torch.device("cpu"), torch.float32, 1, 8, 64
    double_buffer = False

    def reset(self):
        raise AssertionError("the trainer must refuse before it touches the env")


def test_trainer_that_is_not_fused_is_refused(g):
    d = g.Disturbance.normalised(sep=0.05, action=0.2)
    for kw in ({"use_graphs": False}, {"use_graphs": False, "collector": "eager"}):
        with pytest.raises(ValueError, match="collector='fused' only: the noise is drawn inside the fused collection launch"):
            g.PPOTrainer(_Venv(), g.PPOConfig(), disturbance=d, **kw)
    for collector in ("graphs", None):                        # (use_graphs said outright: nothing is captured before the refusal)
        with pytest.raises(ValueError, match="collector='fused' only"):
            g.PPOTrainer(_Venv(), g.PPOConfig(), collector=collector, use_graphs=True, disturbance=d)


def test_state_dict_round_trip_and_refusal(g):
    """The trainers' state_dict() / load_state_dict() go through these (ppo._Trainer): the disturbance as plain numbers, an
    equal one accepted, any other -- another level, another seed, none at all -- refused."""
    D = g.Disturbance.normalised
    ds = g.DisturbanceSet([D(sep=0.05, cpa=0.04, closing=0.03, action=0.2, seed=9), D(seed=9)], 2)
    sd = ds.state_dict()
    import json
    sd = json.loads(json.dumps(sd))                           # plain numbers: survives the file beside the zips
    g.DisturbanceSet([D(sep=0.05, cpa=0.04, closing=0.03, action=0.2, seed=9), D(seed=9)], 2).load_state_dict(sd)
    for other in ([D(sep=0.05, cpa=0.04, closing=0.03, action=0.25, seed=9), D(seed=9)],
                  [D(sep=0.05, cpa=0.04, closing=0.03, action=0.2, seed=10), D(seed=10)],
                  [D(seed=9), D(sep=0.05, cpa=0.04, closing=0.03, action=0.2, seed=9)]):
        with pytest.raises(ValueError, match="goes on under the noise it was started with"):
            g.DisturbanceSet(other, 2).load_state_dict(sd)
    with pytest.raises(ValueError):
        ds.load_state_dict(None)

    class T(g.ppo._Trainer):                                  # the trainers' two methods, without an env
        pass

    t = T()
    t.venv = _Venv()
    assert t.state_dict() == {"disturbance": None}
    t.load_state_dict({"disturbance": None})
    with pytest.raises(ValueError, match="this run trains under none"):
        t.load_state_dict({"disturbance": sd})
    t._set_disturbances([D(sep=0.05, cpa=0.04, closing=0.03, action=0.2, seed=9), D(seed=9)], 2, "T")
    assert json.loads(json.dumps(t.state_dict())) == {"disturbance": sd}
    t.load_state_dict({"disturbance": sd})
    with pytest.raises(ValueError):
        t.load_state_dict({"disturbance": None})
    with pytest.raises(ValueError, match="2 disturbances for 3"):
        t._set_disturbances(ds, 3, "T")


def test_disturbance_syntax(g):
    P = g.Disturbance.parse
    c = g.ACAS2DConfig().to_c()
    d = P("sep=90,cpa=40,closing=8,action=0.1,seed=7")
    assert d == g.Disturbance(sep=90, cpa=40, closing=8, action=0.1, seed=7) and d.seed == 7
    assert math.isclose(d.s_sep, 90 / c.d_sep_max, rel_tol=1e-6) and d.s_action == float(np.float32(0.1))
    assert P("sep=0,cpa=0,closing=0,action=0").is_zero() and P("action=0.2").s_action == float(np.float32(0.2))
    assert P(" sep = 0.04 , seed = 0x10 ", normalised=True) == g.Disturbance.normalised(sep=0.04, seed=16)
    n = P("sep=0.04,cpa=0.04,closing=0.04,action=0.2", normalised=True)
    assert n.sigma == (float(np.float32(0.04)),) * 3
    for bad in ("sep", "sep=", "foo=1", "sep=1;cpa=2", "sep=abc", "sep=1,sep=2", ""):
        with pytest.raises(ValueError, match="disturbance"):
            P(bad)
    # tools/train_ppo.py hands its --disturbance texts to this parser
    tool = open(os.path.join(ROOT, "tools", "train_ppo.py")).read()
    assert '"--disturbance"' in tool and "g.Disturbance.parse(" in tool
