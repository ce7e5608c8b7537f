"""Training under time-correlated and biased errors, host side (no GPU): records.correlated_step(), the one-step specification
of the error a collector keeps between launches; policy.CorrelatedDisturbanceSet, which owns that state; what still refuses a
bare CorrelatedDisturbance; the --disturbance routing of tools/train_ppo.py; the two correlated set-collector entries in the
header, the loader and the built library, and their argument validation (every pointer below is a host address: the calls are
refused before any launch) -- everything the disturbed sibling refuses, in its words, then their own, in their order."""
import ast
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("acas2d_collect_set_correlated_f32", "acas2d_collect_set_correlated_group_f32")
f32 = np.float32


@pytest.fixture(scope="module")
def g():
    import gym_acas2d_amd as g
    return g


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


# ---- records.correlated_step() ------------------------------------------------------------------------------------------------------
def test_three_steps_by_hand(g):
    """rho = 0.9 from e_0 = z_0 = 0.37 on z = -1.21, 0.58, 1.7: each step (rho e) + (q z) with the two products and the sum
    rounded to float32 -- at the first step one bit off either fma, at the second off both fmas AND off the float64 value."""
    R = g.records
    rho, q = f32(0.9), R.correlation_gain(f32(0.9))
    assert bits(q) == bits(f32(0.43588993))
    z = [f32(0.37), f32(-1.21), f32(0.58), f32(1.7)]
    want = (3192330196, 1033856610, 1062183357)               # the bit patterns of e_1, e_2, e_3
    e, differs = z[0], []
    for t in (1, 2, 3):
        a, b = f32(rho * e), f32(q * z[t])                    # two products, each rounded
        e_t = f32(a + b)                                      # the sum, rounded
        assert int(bits(e_t)) == want[t - 1], t
        got = R.correlated_step(e, z[t], rho, False)
        assert got.dtype == np.float32 and int(bits(got)) == want[t - 1], t
        d = np.float64
        fma_a = f32(d(rho) * d(e) + d(b))                     # fma(rho, e, b): the first product unrounded
        fma_b = f32(d(a) + d(q) * d(z[t]))                    # fma(q, z, a): the second one
        f64 = f32(d(rho) * d(e) + d(q) * d(z[t]))             # float64 throughout, rounded once
        differs.append((int(bits(fma_a)) != want[t - 1], int(bits(fma_b)) != want[t - 1], int(bits(f64)) != want[t - 1]))
        e = e_t
    assert differs[0][:2] == (True, True) and differs[1] == (True, True, True)
    # first, and rho == 0: z's own bits, whatever is held (a NaN included)
    for held in (f32(5.0), f32("nan")):
        assert bits(R.correlated_step(held, z[1], rho, True)) == bits(z[1])
        assert bits(R.correlated_step(held, z[1], f32(0), False)) == bits(z[1])
    # rho == 1: the held value goes on, bit for bit (q == 0); a zero held value under first == False gives q z
    assert bits(R.correlated_step(f32(0.37), z[2], f32(1), False)) == bits(f32(0.37))
    assert bits(R.correlated_step(f32(0), z[2], rho, False)) == bits(f32(q * z[2]))


def test_iterated_it_is_correlated_errors(g):
    R = g.records
    rng = np.random.default_rng(5)
    z = rng.standard_normal((40, 6, 3, 4)).astype(np.float32)
    rho = np.asarray([0.9, 1.0, 0.0, 0.5], np.float32)        # per channel of the last axis
    want = R.correlated_errors(z, rho)
    e = np.zeros_like(z)
    held = np.full(z.shape[1:], f32(7.0))                     # (stale: the first step must not read it)
    for t in range(z.shape[0]):
        e[t] = R.correlated_step(held, z[t], rho, t == 0)
        held = e[t]
    assert np.array_equal(bits(e), bits(want))
    # `first` per element: a row that restarts in the middle restarts its scan
    first = np.zeros(z.shape[1:], bool)
    first[2] = True
    again = R.correlated_step(e[9], z[10], rho, first)
    assert np.array_equal(bits(again[2]), bits(z[10][2])) and np.array_equal(bits(again[3]), bits(want[10][3]))
    with pytest.raises(ValueError, match=r"each in \[0, 1\]"):
        R.correlated_step(held, z[0], f32(1.5), False)


# ---- the class ------------------------------------------------------------------------------------------------------------------------
class _Venv:
    """What CorrelatedDisturbanceSet.bind() and PPOTrainer.__init__ read of an env (no GPU)."""
    device, dtype, n_traffic, obs_dim, num_envs = torch.device("cpu"), torch.float32, 2, 11, 64
    double_buffer = False

    def reset(self):
        raise AssertionError("the trainer must refuse before it touches the env")


def members(g, seed=9):
    D, Cd = g.Disturbance.normalised, g.CorrelatedDisturbance.normalised
    return [D(sep=0.05, action=0.2, seed=seed),
            Cd(sep=0.05, cpa=0.04, closing=0.03, action=0.2, seed=seed, rho_sep=0.9, rho_cpa=1.0, rho_closing=0.0, rho_action=0.5)]


def test_the_set(g):
    S, D, Cd = g.CorrelatedDisturbanceSet, g.Disturbance.normalised, g.CorrelatedDisturbance.normalised
    ds = S(members(g), 2)
    assert isinstance(ds, g.DisturbanceSet) and len(ds) == 2 and ds.seed == 9 and not ds.is_zero()
    assert ds.rows.shape == (2, 4) and ds.rows.dtype == np.float32
    assert ds.rows[1].tolist() == [f32(0.05), f32(0.04), f32(0.03), f32(0.2)]
    rho = np.asarray([[0, 0, 0, 0], [0.9, 1.0, 0.0, 0.5]], np.float32)
    assert ds.corr_rows.shape == (2, 8) and ds.corr_rows.dtype == np.float32
    assert np.array_equal(bits(ds.corr_rows[:, :4]), bits(rho))
    assert np.array_equal(bits(ds.corr_rows[:, 4:]), bits(g.records.correlation_gain(rho)))
    assert ds.corr_rows[0, 4:].tolist() == [1.0] * 4 and ds.corr_rows[1, 5] == 0.0
    one = S(Cd(sep=0.1, seed=3, rho=0.99), 3)                 # one for all
    assert len(one) == 3 and (one.corr_rows[:, :4] == f32(0.99)).all() and one.held is None
    # the checks of DisturbanceSet, in its words
    with pytest.raises(ValueError, match="EQUAL seeds"):
        S([D(sep=0.1, seed=7), Cd(sep=0.2, seed=8, rho=0.5)], 2)
    for field in ("sep", "cpa", "closing", "action"):
        for bad in (-0.5, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="finite and at least 0"):
                S(Cd(**{field: bad}, rho=0.5), 1)
            with pytest.raises(ValueError, match="member 1"):
                S([D(), Cd(**{field: bad}, rho=0.5)], 2)
    with pytest.raises(ValueError, match="got 3 for 2"):
        S([Cd(rho=0.5)] * 3, 2)
    with pytest.raises(TypeError):
        S([Cd(rho=0.5), 0.5], 2)
    with pytest.raises(ValueError, match=r"must lie in \[0, 1\]"):       # the rho: checked where the member is made
        Cd(sep=0.1, rho=1.5)


def test_state_dict_round_trip_and_refusal(g):
    S, D, Cd = g.CorrelatedDisturbanceSet, g.Disturbance.normalised, g.CorrelatedDisturbance.normalised
    ds = S(members(g), 2)
    sd = json.loads(json.dumps(ds.state_dict()))              # plain numbers: survives the file beside the zips
    assert "rho_sep" not in sd["members"][0] and sd["members"][1]["rho_cpa"] == 1.0
    S(members(g), 2).load_state_dict(sd)
    a, b = members(g)
    for other in ([a, Cd(sep=0.05, cpa=0.04, closing=0.03, action=0.2, seed=9, rho_sep=0.9, rho_cpa=1.0, rho_closing=0.0,
                        rho_action=0.25)],                                        # another correlation
                  [a, D(sep=0.05, cpa=0.04, closing=0.03, action=0.2, seed=9)],    # the same sigmas, white
                  [Cd(sep=0.05, action=0.2, seed=9), b],                           # rho 0 by name is not the white member
                  members(g, seed=10), [b, a]):
        with pytest.raises(ValueError, match="goes on under the noise it was started with"):
            S(other, 2).load_state_dict(sd)
    with pytest.raises(ValueError):
        ds.load_state_dict(None)
    # a white set's state is foreign to it and the other way round
    white = g.DisturbanceSet([a, a], 2)
    with pytest.raises(ValueError, match="goes on under"):
        S([a, b], 2).load_state_dict(white.state_dict())
    with pytest.raises(ValueError, match="goes on under"):
        white.load_state_dict(sd)
    S([a, a], 2).load_state_dict(white.state_dict())          # ... but an all-white correlated set reads a white state

    class T(g.ppo._Trainer):                                  # the trainers' two methods, without an env
        pass

    t = T()
    t.venv = _Venv()
    t._set_disturbances(ds, 2, "T")
    assert t.disturbances is ds
    assert json.loads(json.dumps(t.state_dict())) == {"disturbance": sd}
    t.load_state_dict({"disturbance": sd})
    assert [d.to_dict() for d in t.disturbances.members][1]["rho_action"] == 0.5       # what the logs and the json files carry
    with pytest.raises(ValueError, match="2 disturbances for 3"):
        t._set_disturbances(ds, 3, "T")


def test_the_held_state_and_its_env(g):
    ds = g.CorrelatedDisturbanceSet(members(g), 2)
    assert ds.held is None and ds.held_numpy() is None
    env = _Venv()
    held = ds.bind(env)
    assert held is ds.held and tuple(held.shape) == (3 * 2 + 1, 64) and held.dtype == torch.float32 and not held.any()
    assert ds.bind(env) is held                               # the same env: the same tensor
    with pytest.raises(ValueError, match="another env"):
        ds.bind(_Venv())
    held[3, 5] = 0.25
    saved = ds.held_numpy()
    assert saved.shape == (7, 64) and saved[3, 5] == f32(0.25)
    ds.reset_held()
    assert not ds.held.any() and saved[3, 5] == f32(0.25)     # (a copy)
    ds.load_held(saved)
    assert ds.held[3, 5] == 0.25
    with pytest.raises(ValueError, match="load_held"):
        ds.load_held(saved[:, :32])
    # across a restart: loaded before the first collection, checked against the env at the binding
    again = g.CorrelatedDisturbanceSet(members(g), 2)
    again.load_held(saved)
    assert np.array_equal(again.held_numpy(), saved)
    assert again.bind(env)[3, 5] == 0.25
    other = g.CorrelatedDisturbanceSet(members(g), 2)
    other.load_held(saved[:4])                                # another N
    with pytest.raises(ValueError, match=r"\[3 N \+ 1, E\]"):
        other.bind(env)

    class Wider(_Venv):
        num_envs = 128

    with pytest.raises(ValueError):                           # another E is another env
        ds.bind(Wider())


def test_a_bare_correlated_disturbance_is_still_refused(g):
    bare = g.CorrelatedDisturbance.normalised(sep=0.05, action=0.2, seed=9, rho=0.5)
    msg = "the collectors are white-noise only"
    with pytest.raises(ValueError, match=msg):
        g.DisturbanceSet(bare, 1)
    with pytest.raises(ValueError, match=msg):
        g.DisturbanceSet([g.Disturbance.normalised(seed=9), bare], 2)
    with pytest.raises(ValueError, match="CorrelatedDisturbanceSet"):          # ... and says where to go
        g.DisturbanceSet(bare, 1)

    class T(g.ppo._Trainer):
        pass

    t = T()
    t.venv = _Venv()
    with pytest.raises(ValueError, match=msg):
        t._set_disturbances(bare, 1, "T")
    # the env's own path (no launch: the set is built first)
    with pytest.raises(ValueError, match=msg):
        g.ACAS2DVecEnv._disturbed_entry(_Venv(), "collect()", bare, 1, False)
    # the set in a trainer that is not fused is refused like a Disturbance
    with pytest.raises(ValueError, match="collector='fused' only"):
        g.PPOTrainer(_Venv(), g.PPOConfig(), use_graphs=False, disturbance=g.CorrelatedDisturbanceSet(bare, 1))


# ---- tools/train_ppo.py ---------------------------------------------------------------------------------------------------------------
def test_the_command_line_routing(g):
    """The tool's own function, taken out of its source (the script itself parses its arguments and trains when it is run)."""
    path = os.path.join(ROOT, "tools", "train_ppo.py")
    tool = open(path).read()
    assert '"--disturbance"' in tool and "g.Disturbance.parse(" in tool and "g.CorrelatedDisturbance.parse(" in tool
    fn = [n for n in ast.parse(tool).body if isinstance(n, ast.FunctionDef) and n.name == "training_disturbances"]
    assert len(fn) == 1 and "training_disturbances(args.disturbance" in tool
    ns = {"g": g}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
    route = ns["training_disturbances"]
    white = route(["sep=0.04,action=0.2,seed=7"], 1, True)
    assert type(white) is g.Disturbance and white == g.Disturbance.normalised(sep=0.04, action=0.2, seed=7)
    sweep = route(["sep=0.04,seed=7", "sep=0.08,seed=7"], 2, True)
    assert [type(d) for d in sweep] == [g.Disturbance] * 2
    corr = route(["sep=0.04,action=0.2,seed=7,rho=0.99"], 1, True)
    assert type(corr) is g.CorrelatedDisturbanceSet and len(corr) == 1
    assert corr.members[0] == g.CorrelatedDisturbance.normalised(sep=0.04, action=0.2, seed=7, rho=0.99)
    pop = route(["sep=0.04,seed=7,rho_sep=0.5"], 3, True)     # once for all members
    assert type(pop) is g.CorrelatedDisturbanceSet and len(pop) == 3 and (pop.corr_rows[:, 0] == f32(0.5)).all()
    mixed = route(["sep=0.04,seed=7", "sep=0.04,seed=7,rho_action=1"], 2, True)      # one per member, one of them white
    assert type(mixed) is g.CorrelatedDisturbanceSet
    assert [type(d) for d in mixed.members] == [g.Disturbance, g.CorrelatedDisturbance] and mixed.corr_rows[1, 3] == 1.0
    px = route(["sep=90,rho=0.5"], 1, False)                  # pixels
    assert px.members[0].s_sep == g.Disturbance(sep=90).s_sep
    for bad in ("sep=0.04,rho=1.5", "sep=0.04,rho=", "rho=0.5,rho=0.6", "sep=0.04,rho_foo=1"):
        with pytest.raises(ValueError):
            route([bad], 1, True)
    with pytest.raises(ValueError, match="EQUAL seeds"):
        route(["sep=0.04,seed=7", "sep=0.04,seed=8,rho=0.5"], 2, True)


# ---- the C entries --------------------------------------------------------------------------------------------------------------------
def test_symbols_header_and_loader(g):
    L = g.native.lib()
    header = open(os.path.join(ROOT, "include", "acas2d.h")).read()
    assert "#define ACAS2D_ABI_VERSION 7" in header and L.acas2d_abi_version() == 7 and g.native.ABI_VERSION == 7      # additive
    for name in ENTRIES:
        assert name in g.native.EXPORTS and hasattr(L, name)
        assert ("int %s(const Acas2dConfig *cfg" % name) in header
        # the disturbed sibling's arguments, then correlations and held in front of the stream
        sib = getattr(L, name.replace("_correlated", "_disturbed")).argtypes
        assert list(getattr(L, name).argtypes) == list(sib[:-1]) + [C.c_void_p, C.c_void_p, sib[-1]]
    # coefficients on the device are the caller's to check, and a zero held value is documented: the header says so
    assert "the CALLER makes sure each rho is in [0, 1]" in header and "gives e_t = q z_t" in header


CASES = ((ENTRIES[0], 1, 16, "no thread-per-env shape"), (ENTRIES[0], 8, 5, "no thread-per-env shape"),
         (ENTRIES[1], 16, 3, "use acas2d_collect_set_f32"), (ENTRIES[1], 64, 5, "has no packed work shape"))


@pytest.mark.parametrize("entry,N,badN,bad_msg", CASES, ids=["%s-N%d" % (c[0][7:-4], c[1]) for c in CASES])
def test_validation_needs_no_gpu(g, entry, N, badN, bad_msg):
    L = g.native.lib()
    D, T, E = 5 + 3 * N, 4, 128
    row, held_bytes = E * D * 4, E * (3 * N + 1) * 4
    buf = (C.c_char * (row * (3 * T + 8) + held_bytes + 65536))()
    a = (C.addressof(buf) + 255) // 256 * 256
    obs_in, obs, obs_read = a + 4096, a + 4096 + row, a + 4096 + row * (T + 1)        # adjoining, none overlapping
    held = obs_read + row * (T + 1)                                                    # ... and the state behind them
    far = obs_read + (1 << 30)
    far_held = far + (1 << 29)                                # (rows of another width: nothing here overlaps them)
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
             sigmas=a, seed=7, read=obs_read, corr=a, held_=held, null_io=False, null_ac=False):
        return fn(cfg_, state, None if null_io else C.byref(io_ or io()), None if null_ac else C.byref(ac_ or ac()), K, keys, obs_in_,
                  T_, 13, off, n_envs, n, sigmas, seed, read, corr, held_, None)

    def rejects(msg, **kw):
        assert call(**kw) == -22, kw
        assert msg.encode() in L.acas2d_last_error(), (kw, L.acas2d_last_error())

    # ---- everything the disturbed sibling refuses, under this entry's name
    rejects(name + ": NULL sigmas", sigmas=None)
    rejects(name + ": NULL sigmas", read=None)
    for read in (obs, obs + row * T - 4, obs - row * (T + 1) + 4, obs_in, obs_in + row - 4, obs_in - row * (T + 1) + 4):
        rejects(name + ": obs_read overlaps io->obs or obs_in", read=read, held_=far)
    for max_steps, refused in (((1 << 20) - 1, True), (1 << 20, True), (0x7FFFFFFF, True), ((1 << 20) - 2, False)):
        big = g.ACAS2DConfig(n_traffic=N, max_steps=max_steps).to_c()
        assert call(cfg_=C.byref(big), n=badN, read=far, held_=far_held) == -22
        assert (b"the step field of the noise counter" in L.acas2d_last_error()) == refused, (max_steps, L.acas2d_last_error())
    assert call(K=1, n_envs=70, n=badN, read=far, held_=far_held) == -22 and bad_msg.encode() in L.acas2d_last_error(), L.acas2d_last_error()
    rejects("n_envs = 70 is not n_members = 2 x a multiple of 64", n_envs=70)
    rejects("n_envs = 192 is not n_members = 2 x a multiple of 64", n_envs=192)
    rejects(bad_msg, n=badN, read=far, held_=far_held)
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
    # ---- its own: a NULL correlations, then a NULL held, then held overlapping obs_read, io->obs or obs_in
    rejects(name + ": NULL correlations", corr=None)
    rejects(name + ": NULL held", held_=None)
    for h in (obs_read, obs_read + row * (T + 1) - 4, obs_read - held_bytes + 4,      # obs_read: first bytes, last, held's last on its first
              obs, obs + row * T - 4, obs_in, obs_in + row - 4, obs_in - held_bytes + 4):
        rejects(name + ": held overlaps obs_read, io->obs or obs_in", held_=h)
    # the precedence: EVERYTHING the sibling rejects first, down to its last checks -- the sizes, the signs, the work shape and
    # (group) the alignment, which stand behind its own pointers -- then correlations, then held, then the overlap
    for own in (dict(corr=None, held_=None), dict(corr=None), dict(held_=None), dict(held_=obs)):
        rejects(name + ": NULL sigmas", sigmas=None, **own)
        rejects(name + ": obs_read overlaps", read=obs, **own)
        rejects("the step field of the noise counter", cfg_=C.byref(g.ACAS2DConfig(n_traffic=N, max_steps=1 << 20).to_c()), **own)
        rejects("n_members = 0", K=0, **own)
        rejects(name + ": NULL noise_seeds", keys=None, **own)
        rejects("n_traffic = 0", n=0, **own)
        rejects("n_steps = 0", T_=0, **own)
        rejects("negative n_envs / env_offset", off=-1, **own)
        rejects("negative n_envs / env_offset", n_envs=-128, **own)
        rejects(bad_msg, n=badN, read=far, **own)
        if "group" in entry:
            rejects("16-byte aligned", ac_=ac(w2t=a + 4), **own)
            rejects("16-byte aligned", ac_=ac(vb1=a + 8), **own)
        assert call(n_envs=0, **own) == 0                     # nothing to do: nothing is looked at
    rejects(name + ": NULL correlations", corr=None, held_=None)
    rejects(name + ": NULL correlations", corr=None, held_=obs)
    rejects(name + ": NULL held", held_=None)


BUILT = tuple((ENTRIES[0], N) for N in (1, 2, 3, 4, 8)) + tuple((ENTRIES[1], N) for N in (8, 16, 32, 64))


@pytest.mark.parametrize("entry,N", BUILT, ids=["%s-N%d" % (e[7:-4], N) for e, N in BUILT])
def test_every_shape_gets_past_the_launchers_lds_limit(g, entry, N):
    """The entries' own rejections stand last of all: a call that is turned away for its NULL correlations has passed the work
    shape and geometry_for() with the error state's LDS (3 C + 1 values per lane behind the tile, the reset slots and the hidden
    vectors: at most 63 232 of 65 536 bytes per workgroup, at (4,2)) -- at every traffic count the two entries are built for.
    One member, 70 envs (a partial wave) and two members x 64; host pointers only, nothing is launched."""
    L = g.native.lib()
    T, E = 4, 128
    row = E * (5 + 3 * N) * 4
    buf = (C.c_char * (row * (2 * T + 4) + E * (3 * N + 1) * 4 + 65536))()
    a = (C.addressof(buf) + 255) // 256 * 256
    obs_in, obs, obs_read = a + 4096, a + 4096 + row, a + 4096 + row * (T + 1)
    held = obs_read + row * (T + 1)
    st = g.native.CState(*([a] * 14), None)
    cfg = g.ACAS2DConfig(n_traffic=N).to_c()
    io = g.native.CStepIO(actions=a, obs=obs, reward=a, done=a, outcome=a, term_obs=None, ep_return=a, ep_steps=a)
    pol = g.native.CPolicy(**{n: a for n, _ in g.native.CPolicy._fields_[:6]}, hidden=64, _pad=0)
    ac = g.native.CActorCritic(pol, **{n: a for n, _ in g.native.CActorCritic._fields_[1:10]}, noise_seed=0, noise_step=0, _pad=0)
    for K, n_envs in ((1, 70), (2, E)):
        for corr, held_, msg in ((None, held, "NULL correlations"), (None, None, "NULL correlations"), (a, None, "NULL held")):
            rc = getattr(L, entry)(C.byref(cfg), C.byref(st), C.byref(io), C.byref(ac), K, a, obs_in, T, 13, 0, n_envs, N, a, 7,
                                   obs_read, corr, held_, None)
            assert rc == -22, (K, rc)
            assert L.acas2d_last_error().decode().startswith("%s: %s" % (entry[:-4], msg)), (K, L.acas2d_last_error())
