"""acas2d_gae_f32 (csrc/acas2d_gae.hip): the bootstrap value and GAE of a PPO iteration in one launch.

The contract is bitwise: the kernel's sweep is compute_gae()'s sequence of float32 roundings.  The referee is a float32
NumPy restatement of that sequence (`referee`), pinned to compute_gae on the CPU first; the GPU tests then hold the kernel
to the referee AND to compute_gae run on the device, bit pattern for bit pattern.  The in-kernel critic is held to the
collector: the value of an observation equals what a collection started on it stores in `values`.  The trainers' `gae=`
option and the torch-free C++ host (examples/c_abi_ppo_example.cpp) are run end to end."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers as H

torch = pytest.importorskip("torch")
DEV = "cuda:0"
ROOT, CSRC = H.ROOT, H.CSRC
FLT_MAX = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def g():
    import gym_acas2d_amd as g
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    g.native.lib()
    return g


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def referee(rew, val, done, last_value, gamma, gl):
    """The kernel's sequence in float32 NumPy: every operation one float32 rounding.  gamma / gl: float32 scalars or [E]."""
    rew, val, last_value = (np.asarray(x, np.float32) for x in (rew, val, last_value))
    gamma, gl = np.asarray(gamma, np.float32), np.asarray(gl, np.float32)
    T = rew.shape[0]
    r = np.where(np.isnan(rew), np.float32(0), np.clip(rew, -FLT_MAX, FLT_MAX)).astype(np.float32)
    adv, ret = np.zeros_like(val), np.zeros_like(val)
    last = np.zeros_like(last_value)
    for t in reversed(range(T)):
        nt = np.where(np.asarray(done[t]).astype(bool), np.float32(0), np.float32(1)).astype(np.float32)
        nv = last_value if t == T - 1 else val[t + 1]
        delta = (r[t] + ((gamma * nv) * nt)) - val[t]
        last = delta + ((gl * nt) * last)
        assert delta.dtype == np.float32 and last.dtype == np.float32
        adv[t], ret[t] = last, last + val[t]
    return adv, ret


DONE_PATTERNS = ("none", "all", "ends", "one_env", "random")


def make_inputs(T, E, pattern, seed):
    """Hand-placed edges: values of order +-50, rewards of +-1000, NaN and +-inf (one infinity of each sign, in different
    envs where there are two: two FLT_MAX of one sign in one episode would overflow to inf and meet 0 x inf = NaN at a
    done, and a generated NaN's sign bit differs between x86 and the GPU), dones by `pattern`."""
    rng = np.random.default_rng(seed)
    rew = rng.normal(0, 1, (T, E)).astype(np.float32)
    val = rng.normal(0, 50, (T, E)).astype(np.float32)
    last_value = rng.normal(0, 50, E).astype(np.float32)
    rew[rng.random((T, E)) < 0.05] = 1000.0
    rew[rng.random((T, E)) < 0.05] = -1000.0
    rew[rng.random((T, E)) < 0.04] = np.nan
    rew[T // 2, 1 % E] = np.inf
    rew[T // 3, 2 % E] = -np.inf
    rew[T - 1, 0] = np.nan
    done = np.zeros((T, E), bool)
    if pattern == "all":
        done[:] = True
    elif pattern == "ends":
        done[0], done[T - 1] = True, True
    elif pattern == "one_env":
        done[:, E // 2] = True
    elif pattern == "random":
        done = rng.random((T, E)) < 0.15
    return rew, val, done, last_value


# ---- CPU -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tensors", (False, True), ids=("floats", "tensors"))
def test_referee_equals_compute_gae_bitwise_on_the_cpu(tensors):
    """Pins the referee the GPU tests use: both semantics of gamma x lambda (Python numbers: the product in double, rounded
    once; float32 tensors: rounded, then multiplied in float32)."""
    from gym_acas2d_amd.ppo import compute_gae
    T, E = 97, 130
    for pattern in DONE_PATTERNS:
        rew, val, done, lv = make_inputs(T, E, pattern, seed=7)
        rng = np.random.default_rng(1)
        if tensors:
            gam = rng.uniform(0.9, 0.999, E).astype(np.float32)
            lam = rng.uniform(0.8, 0.99, E).astype(np.float32)
            a, r = referee(rew, val, done, lv, gam, gam * lam)
            gam_t, lam_t = torch.as_tensor(gam), torch.as_tensor(lam)
        else:
            gam_t, lam_t = 0.99, 0.95
            a, r = referee(rew, val, done, lv, np.float32(0.99), np.float32(0.99 * 0.95))
        rew_t = torch.nan_to_num(torch.as_tensor(rew), nan=0.0)
        a_t, r_t = compute_gae(rew_t, torch.as_tensor(val), torch.as_tensor(done), torch.as_tensor(lv), gam_t, lam_t)
        assert np.array_equal(bits(a), bits(a_t)) and np.array_equal(bits(r), bits(r_t)), pattern
        assert np.isfinite(a).all()                       # (the placement above generates no NaN)


def _valid_gae(native, **over):
    """A struct every check accepts (made-up addresses: nothing may be launched with it), then `over`."""
    f = dict(reward=0x1000, value=0x2000, done=0x3000, last_value=0x4000, obs_last=0x5000, v1t=0x6000, vb1=0x7000,
             v2t=0x8000, vb2=0x9000, v3=0xa000, vb3=0xb000, gamma=0xc000, gamma_lambda=0xd000, adv=0xe000, ret=0xf000,
             last_value_out=None, nan_count=None, n_envs=192, n_steps=8, n_members=1, obs_dim=8, _pad=0)
    f.update(over)
    return native.CGae(**f)


def test_gae_rejections_and_struct_size_without_a_device():
    from gym_acas2d_amd import native
    L = native.lib()
    assert L.acas2d_gae_size() == C.sizeof(native.CGae)
    assert L.acas2d_gae_pipeline_depth() >= 2
    cases = [("NULL struct", None)]
    for name in ("reward", "value", "done", "adv", "ret", "gamma", "gamma_lambda"):
        cases.append(("NULL " + name, {name: None}))
    cases += [("n_steps 0", dict(n_steps=0)), ("n_envs 0", dict(n_envs=0)), ("n_members 0", dict(n_members=0)),
              ("K = 3, EM = 65", dict(n_members=3, n_envs=195)), ("K = 2, odd split", dict(n_members=2, n_envs=193)),
              ("no last_value, no obs_last", dict(last_value=None, obs_last=None)),
              ("bootstrap, obs_dim 53", dict(last_value=None, obs_dim=53)),
              ("bootstrap, obs_dim 9", dict(last_value=None, obs_dim=9)),
              ("adv == ret", dict(ret=0xe000))]
    for name in ("v1t", "vb1", "v2t", "vb2", "v3", "vb3"):
        cases.append(("bootstrap, NULL " + name, {"last_value": None, name: None}))
    for name in ("reward", "value", "done", "last_value", "obs_last", "gamma", "gamma_lambda", "v1t", "vb3"):
        addr = _valid_gae(native).__getattribute__(name)
        cases.append(("adv == " + name, dict(adv=addr)))
        cases.append(("ret == " + name, dict(ret=addr)))
    for what, over in cases:
        rc = L.acas2d_gae_f32(None, None) if over is None else L.acas2d_gae_f32(C.byref(_valid_gae(native, **over)), None)
        assert rc == -22, (what, rc)
        assert L.acas2d_last_error().startswith(b"acas2d_gae"), what
    L.acas2d_gae_f32(C.byref(_valid_gae(native, last_value=None, obs_dim=53)), None)
    assert b"wide" in L.acas2d_last_error() and b"last_value" in L.acas2d_last_error()


@H.needs_hipcc
def test_gae_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    """The code-object metadata of csrc/acas2d_gae.hip, read the way tests/test_build_resources.py reads it: the sweep
    keeps two blocks of 16 rows in registers, and the bootstrap variants stream a critic through SGPRs on top."""
    _, kernels = H.kernel_metadata(tmp_path, "acas2d_gae.hip")
    assert len(kernels) == 6                              # last_value given + five observation widths
    for k in kernels:
        assert "gae_kernel" in k.name
        print(k.name, "vgpr", k.field("vgpr_count"), "sgpr", k.field("sgpr_count"))
        assert k.field("vgpr_spill_count") == 0 and k.field("sgpr_spill_count") == 0, k.name
        assert k.field("private_segment_fixed_size") == 0 and k.field("vgpr_count") <= 256, k.name


# ---- GPU: the sweep ---------------------------------------------------------------------------------------------------
def _depth():
    from gym_acas2d_amd import native
    return int(native.lib().acas2d_gae_pipeline_depth())


def _t_cases():
    U = 16                                                # acas2d_gae_pipeline_depth(); asserted in the test
    return sorted({1, 2, U - 1, U, U + 1, 3 * U + 5})


def _check_sweep(g, T, E, K, gam, lam, tensors):
    dev = torch.device(DEV)
    EM = E // K
    for pi, pattern in enumerate(DONE_PATTERNS):
        rew, val, done, lv = make_inputs(T, E, pattern, seed=100 * T + E + pi)
        if tensors:
            gam32, lam32 = np.asarray(gam, np.float32), np.asarray(lam, np.float32)
            gam_e, gl_e = np.repeat(gam32, EM), np.repeat(gam32 * lam32, EM)
            gam_a, lam_a = torch.as_tensor(gam32, device=dev), torch.as_tensor(lam32, device=dev)
            gam_t, lam_t = gam_a.repeat_interleave(EM), lam_a.repeat_interleave(EM)      # compute_gae: per env
        else:
            gam_e, gl_e = np.float32(gam), np.float32(gam * lam)
            gam_a, lam_a, gam_t, lam_t = gam, lam, gam, lam
        a_ref, r_ref = referee(rew, val, done, lv, gam_e, gl_e)
        d = lambda x: torch.as_tensor(x, device=dev)  # noqa: E731
        rew_d, val_d, done_d, lv_d = d(rew), d(val), d(done), d(lv)
        a_t, r_t = g.compute_gae(torch.nan_to_num(rew_d, nan=0.0), val_d, done_d, lv_d, gam_t, lam_t)
        nan_count = torch.zeros(K, dtype=torch.int32, device=dev)
        adv, ret = g.gae_fused(rew_d, val_d, done_d, lv_d, gamma=gam_a, gae_lambda=lam_a, n_members=K, nan_count=nan_count)
        torch.cuda.synchronize()
        what = (T, E, K, pattern, tensors)
        assert np.array_equal(bits(adv), bits(a_ref)) and np.array_equal(bits(ret), bits(r_ref)), what
        assert np.array_equal(bits(adv), bits(a_t)) and np.array_equal(bits(ret), bits(r_t)), what
        want = np.isnan(rew).reshape(T, K, EM).sum((0, 2))
        assert want.sum() > 0 and np.array_equal(nan_count.cpu().numpy(), want), what
        # uint8 dones (the collector's own buffer) are the same launch
        adv8, ret8 = g.gae_fused(rew_d, val_d, done_d.view(torch.uint8), lv_d, gamma=gam_a, gae_lambda=lam_a, n_members=K)
        assert torch.equal(adv8.view(torch.int32), adv.view(torch.int32)) and torch.equal(ret8.view(torch.int32),
                                                                                           ret.view(torch.int32)), what


@pytest.mark.gpu
@pytest.mark.parametrize("E", (1, 63, 64, 65, 200))
@pytest.mark.parametrize("T", _t_cases())
def test_gae_sweep_one_member_bitwise(g, T, E):
    """K = 1 at every T around the pipeline depth and env counts with tail lanes, against the NumPy referee and against
    compute_gae on the device: no dones, all dones, a done at t = 0 and T - 1, one env done at every step, random dones;
    rewards of +-1000, NaN and +-inf; values of order +-50; nan_count."""
    assert _t_cases() == sorted({1, 2, _depth() - 1, _depth(), _depth() + 1, 3 * _depth() + 5})
    _check_sweep(g, T, E, 1, 0.99, 0.95, False)


@pytest.mark.gpu
@pytest.mark.parametrize("tensors", (False, True), ids=("floats", "tensors"))
@pytest.mark.parametrize("EM", (64, 128))
@pytest.mark.parametrize("T", _t_cases())
def test_gae_sweep_three_members_bitwise(g, T, EM, tensors):
    """K = 3: distinct gamma / lambda per member as float32 tensors (the product rounded in float32), and one pair of Python
    numbers for all (the product taken in double)."""
    if tensors:
        _check_sweep(g, T, 3 * EM, 3, (0.99, 0.97, 0.999), (0.95, 0.9, 0.98), True)
    else:
        _check_sweep(g, T, 3 * EM, 3, 0.98, 0.93, False)


@pytest.mark.gpu
def test_gae_fused_says_what_it_cannot_take(g):
    z = torch.zeros(4, 192, device=DEV)
    done = torch.zeros(4, 192, dtype=torch.bool, device=DEV)
    with pytest.raises(ValueError, match="multiple of 64"):
        g.gae_fused(z[:, :190], z[:, :190], done[:, :190], z[0, :190], n_members=2)
    with pytest.raises(ValueError, match="last_value"):
        g.gae_fused(z, z, done)
    with pytest.raises(ValueError, match="pass last_value"):
        g.gae_fused(z, z, done, critic=g.ActorCritic(53), obs_last=torch.zeros(192, 53, device=DEV))
    with pytest.raises(ValueError, match="float32"):
        g.gae_fused(z.double(), z.double(), done, z[0].double())
    with pytest.raises(RuntimeError, match="adv and ret"):
        g.gae_fused(z, z, done, z[0].clone(), out={"adv": z, "ret": torch.zeros_like(z)})


# ---- GPU: the bootstrap value -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("N", (1, 2, 3, 4, 8))
def test_bootstrap_value_equals_the_next_collection_bitwise(g, N):
    """Collect 4 steps, run gae_fused with the critic inside the kernel on obs[T]; collect again from the state left with
    the same weights: the kernel's last_value is that collection's values[0], bit for bit (130 envs: a tail wave).  A
    non-finite entry of obs_last gives the bits of the same row with 0 there."""
    T, E, D = 4, 130, 5 + 3 * N
    torch.manual_seed(40 + N)
    pol = g.ActorCritic(D).to(DEV)
    with torch.no_grad():
        pol.value_net.weight.mul_(20.0)                   # values of order 10, not SB3's near-zero start
        pol.value_net.bias.fill_(0.3)
    env = g.ACAS2DVecEnv(E, N, device=DEV, dtype=torch.float32, seed=5)
    env.reset()
    out = env.collect(pol, T, noise_seed=9, noise_step=0)
    adv, ret, lv = g.gae_fused(out["reward"], out["values"], out["done"], critic=pol, obs_last=out["obs"][T],
                               gamma=0.99, gae_lambda=0.95)
    nxt = env.collect(pol, T, noise_seed=9, noise_step=T)
    torch.cuda.synchronize()
    assert float(lv.abs().max()) > 0.1
    assert np.array_equal(bits(lv), bits(nxt["values"][0]))
    # ... and the sweep used it
    a_ref, r_ref = referee(out["reward"].cpu().numpy(), out["values"].cpu().numpy(), out["done"].cpu().numpy(),
                           lv.cpu().numpy(), np.float32(0.99), np.float32(0.99 * 0.95))
    assert np.array_equal(bits(adv), bits(a_ref)) and np.array_equal(bits(ret), bits(r_ref))
    bad, zero = out["obs"][T].clone(), out["obs"][T].clone()
    for (e, i), v in (((5, 2), float("nan")), ((77, 0), float("inf")), ((129, D - 1), float("-inf"))):
        bad[e, i], zero[e, i] = v, 0.0
    lv_bad = g.gae_fused(out["reward"], out["values"], out["done"], critic=pol, obs_last=bad)[2]
    lv_zero = g.gae_fused(out["reward"], out["values"], out["done"], critic=pol, obs_last=zero)[2]
    assert np.array_equal(bits(lv_bad), bits(lv_zero)) and not np.array_equal(bits(lv_bad)[[5, 77, 129]], bits(lv)[[5, 77, 129]])


@pytest.mark.gpu
def test_bootstrap_value_of_three_members_equals_the_next_set_collection(g):
    T, N, K, EM = 4, 2, 3, 64
    D, E = 5 + 3 * N, K * EM
    members = []
    for k in range(K):
        torch.manual_seed(60 + k)
        m = g.ActorCritic(D)
        with torch.no_grad():
            m.value_net.weight.mul_(10.0 + 5 * k)
        members.append(m)
    pset = g.ActorCriticSet.from_members(members, device=DEV)
    env = g.ACAS2DVecEnv(E, N, device=DEV, dtype=torch.float32, seed=5)
    env.reset()
    seeds = [3, 4, 5]
    out = env.collect_set(pset, T, seeds, noise_step=0)
    gam = torch.tensor([0.99, 0.97, 0.999], device=DEV)
    lam = torch.tensor([0.95, 0.9, 0.98], device=DEV)
    adv, ret, lv = g.gae_fused(out["reward"], out["values"], out["done"], critic=pset, obs_last=out["obs"][T], gamma=gam,
                               gae_lambda=lam, n_members=K)
    nxt = env.collect_set(pset, T, seeds, noise_step=T)
    torch.cuda.synchronize()
    assert np.array_equal(bits(lv), bits(nxt["values"][0]))
    lv3 = lv.view(K, EM)
    assert not torch.equal(lv3[0], lv3[1])
    gam_e, gl_e = gam.repeat_interleave(EM).cpu().numpy(), (gam * lam).repeat_interleave(EM).cpu().numpy()
    a_ref, r_ref = referee(out["reward"].cpu().numpy(), out["values"].cpu().numpy(), out["done"].cpu().numpy(),
                           lv.cpu().numpy(), gam_e, gl_e)
    assert np.array_equal(bits(adv), bits(a_ref)) and np.array_equal(bits(ret), bits(r_ref))


# ---- GPU: the trainers ----------------------------------------------------------------------------------------------------
def _ppo_trainer(g, gae):
    N, E, T = 1, 256, 24
    venv = g.ACAS2DVecEnv(E, N, device=DEV, dtype=torch.float32, seed=13, config=g.ACAS2DConfig(n_traffic=N, max_steps=15))
    cfg = g.PPOConfig(n_steps=T, batch_size=1024, n_epochs=2, seed=13)
    return g.PPOTrainer(venv, cfg, collector="fused", updater="fused", gae=gae)


@pytest.mark.gpu
def test_ppo_trainer_kernel_gae_is_the_torch_run_bitwise(g):
    """Two identically seeded PPOTrainer(collector="fused", updater="fused"), with and without gae="kernel": after
    collect() the advantages and returns are bit-equal (max_steps 15 < T: dones occur)."""
    tk, tt = _ppo_trainer(g, "kernel"), _ppo_trainer(g, None)
    assert tk.gae == "kernel" and tt.gae == "torch"
    tk.collect()
    tt.collect()
    torch.cuda.synchronize()
    assert bool(tk.b_done.any()) and torch.equal(tk.b_done, tt.b_done)
    assert float(tk.b_adv.abs().max()) > 0
    assert np.array_equal(bits(tk.b_rew), bits(tt.b_rew)) and np.array_equal(bits(tk.b_val), bits(tt.b_val))
    assert np.array_equal(bits(tk.b_adv), bits(tt.b_adv)) and np.array_equal(bits(tk.b_ret), bits(tt.b_ret))


@pytest.mark.gpu
def test_ppo_trainer_learns_three_iterations_with_kernel_gae(g):
    tk = _ppo_trainer(g, "kernel")
    n = 3 * 24 * 256
    hist = tk.learn(n, log=None)
    assert tk.num_timesteps == n and len(hist) == 3
    assert all(bool(torch.isfinite(p).all()) for p in tk.policy.parameters())
    assert all(np.isfinite(h["value_loss"]) for h in hist)


@pytest.mark.gpu
def test_trainers_reject_kernel_gae_where_it_is_not_wired(g):
    venv = g.ACAS2DVecEnv(64, 1, device=DEV, dtype=torch.float32, seed=13)
    for kw in (dict(collector="graphs"), dict(use_graphs=False), dict(collector="eager", use_graphs=True)):
        with pytest.raises(ValueError, match="collector='fused'"):
            g.PPOTrainer(venv, g.PPOConfig(n_steps=4), gae="kernel", **kw)
    with pytest.raises(ValueError, match="gae must be"):
        g.PPOTrainer(venv, g.PPOConfig(n_steps=4), gae="fast")
    with pytest.raises(ValueError, match="gae must be"):
        g.PopulationTrainer(venv, [g.PPOConfig(n_steps=4)], gae="fast")


def _population(g, gae):
    K, EM, N, T = 3, 256, 8, 24
    gam, lam = (0.99, 0.97, 0.999), (0.95, 0.9, 0.98)
    cfgs = [g.PPOConfig(seed=13 + k, gamma=gam[k], gae_lambda=lam[k], n_steps=T, batch_size=2048, n_epochs=2)
            for k in range(K)]
    venv = g.ACAS2DVecEnv(K * EM, N, device=DEV, seed=13, config=g.ACAS2DConfig(n_traffic=N, max_steps=15))
    return g.PopulationTrainer(venv, cfgs, gae=gae)


@pytest.mark.gpu
def test_population_trainer_kernel_gae_is_the_torch_run_bitwise(g):
    """K = 3, EM = 256, N = 8, per-member gamma / lambda (compute_gae then takes per-env float32 vectors)."""
    pk, pt = _population(g, "kernel"), _population(g, None)
    pk.collect()
    pt.collect()
    torch.cuda.synchronize()
    assert bool(pk.b_done.any()) and torch.equal(pk.b_done, pt.b_done)
    assert np.array_equal(bits(pk.last_value), bits(pt.last_value))
    assert np.array_equal(bits(pk.b_adv), bits(pt.b_adv)) and np.array_equal(bits(pk.b_ret), bits(pt.b_ret))
    # equal gamma / lambda: Python numbers in compute_gae (the product in double)
    assert float(pk.b_adv.abs().max()) > 0


@pytest.mark.gpu
def test_population_trainer_learns_three_iterations_with_kernel_gae(g):
    pk = _population(g, "kernel")
    n = 3 * 24 * 256
    pk.learn(n, log=None)
    assert pk.num_timesteps == n
    assert all(bool(torch.isfinite(p).all()) for p in pk.policy_set.params.values())


# ---- GPU: the torch-free C++ host ---------------------------------------------------------------------------------------
class _Lcg:
    """examples/c_abi_ppo_example.cpp's generator: the weights, then the shuffles, from one 64-bit LCG."""

    def __init__(self):
        self.s = 13

    def next(self):
        self.s = (self.s * 6364136223846793005 + 1442695040888963407) % 2 ** 64
        return self.s

    def weights(self, count, scale):
        return np.asarray([((self.next() >> 40) / 2 ** 24 - 0.5) * scale for _ in range(count)], np.float32)

    def shuffle(self, n):
        perm = list(range(n))
        for i in range(n - 1, 0, -1):
            j = (self.next() >> 33) % (i + 1)
            perm[i], perm[j] = perm[j], perm[i]
        return perm


@pytest.mark.gpu
def test_cpp_host_runs_ppo_on_the_c_abi_and_matches_the_python_wrappers(g, tmp_path):
    """examples/c_abi_ppo_example.cpp: reset, collect, GAE with the bootstrap value in the kernel and minibatch updates
    from C++, no Python and no torch in the process.  Replayed here through the Python wrappers with the restated
    generators: the collection / GAE checksums are equal exactly; after the one compared update the parameters agree
    within the applied-step bound of tests/test_learner_kernels.py (1e-2 lr past one ulp: float atomics make the update
    non-bitwise) and the value loss within its 1e-5."""
    exe = os.path.join(ROOT, "examples", "c_abi_ppo_example")
    made_from = (exe + ".cpp", os.path.join(ROOT, "include", "acas2d.h"))
    if not os.path.exists(exe) or any(os.path.getmtime(exe) < os.path.getmtime(f) for f in made_from):
        subprocess.run(["make", "-C", CSRC, "example"], check=True, capture_output=True)
    E, N, T, iters = 256, 1, 16, 2
    D, lr = 5 + 3 * N, 3e-4
    dump = tmp_path / "params.bin"
    lines = subprocess.run([exe, str(E), str(N), str(T), str(iters), str(dump)], check=True, capture_output=True,
                           text=True).stdout.splitlines()
    print("\n".join(lines))
    assert [l.split()[0] for l in lines] == ["collect", "update", "final"]
    c_sums = [int(x) for x in lines[0].split()[1:]]
    c_upd = [float(x) for x in lines[1].split()[1:]]
    c_final = lines[2].split()[1:]

    lcg = _Lcg()
    counts = [64 * D, 64, 64 * 64, 64, 64, 1, 64 * D, 64, 64 * 64, 64, 64, 1, 1]
    scales = [0.5, 0, 0.25, 0, 2.0 ** -6, 0, 0.5, 0, 0.25, 0, 0.125, 0, 0]
    pol = g.ActorCritic(D).to(DEV)
    from gym_acas2d_amd.ppo import PARAM_NAMES
    with torch.no_grad():
        for name, n, s in zip(PARAM_NAMES, counts, scales):
            p = pol.get_parameter(name)
            assert p.numel() == n
            w = lcg.weights(n, s) if s else np.zeros(n, np.float32)
            p.copy_(torch.as_tensor(w).reshape(p.shape))
    env = g.ACAS2DVecEnv(E, N, device=DEV, dtype=torch.float32, seed=13)
    env.reset()
    out = env.collect(pol, T, noise_seed=13, noise_step=0)
    adv, ret, _ = g.gae_fused(out["reward"], out["values"], out["done"], critic=pol, obs_last=out["obs"][T], gamma=0.99,
                              gae_lambda=0.95)
    torch.cuda.synchronize()
    usum = lambda t: int(bits(t).astype(np.uint64).sum())  # noqa: E731
    assert c_sums == [usum(out["obs"]), usum(out["reward"]), usum(out["values"]), usum(adv), usum(ret)]

    cfg = g.PPOConfig()
    assert (cfg.clip_range, cfg.vf_coef, cfg.ent_coef, cfg.max_grad_norm, cfg.learning_rate) == (0.2, 0.5, 0.0, 0.5, lr)
    fu = g.FusedUpdate(pol, cfg, out["obs"][:T], out["actions"], out["logp"], adv, ret)
    B = min(1024, T * E)
    idx = torch.as_tensor(lcg.shuffle(T * E)[:B], dtype=torch.int64, device=DEV)
    fu.step(idx)
    torch.cuda.synchronize()
    vf = fu.last_losses()["value_loss"]
    print("value loss: C++ %.9e, Python %.9e" % (c_upd[13], vf))
    assert abs(c_upd[13] - vf) <= 1e-5 * max(1.0, vf)
    c_params = np.fromfile(dump, np.float32)
    assert c_params.size == sum(counts)
    worst, at = 0.0, 0
    for name, n, c_sum in zip(PARAM_NAMES, counts, c_upd):
        mine = pol.get_parameter(name).detach().cpu().numpy().reshape(-1).astype(np.float64)
        theirs = c_params[at:at + n].astype(np.float64)
        at += n
        assert abs(theirs.sum() - c_sum) <= 1e-9 * max(1.0, np.abs(theirs).sum()), name      # the printed sum is the dump's
        ulp = np.spacing(np.abs(mine).astype(np.float32)).astype(np.float64)
        excess = (np.abs(theirs - mine) - ulp) / lr
        worst = max(worst, float(excess.max()))
        assert excess.max() <= 1e-2, (name, float(excess.max()), int(excess.argmax()))
    print("worst parameter excess %.2e lr (bound 1e-2)" % worst)
    moved = np.abs(c_params[:64 * D].astype(np.float64) - lcg_first_layer(D)).max()
    assert moved > 0.05 * lr                                  # the step was taken
    assert np.isfinite(float(c_final[0])) and c_final[1] == "1"


def lcg_first_layer(D):
    return _Lcg().weights(64 * D, 0.5).astype(np.float64)
