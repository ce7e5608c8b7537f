"""K PPO learners at once: acas2d_collect_set_f32, acas2d_ppo_update_set_f32 and the host classes over them
(ppo.ActorCriticSet, ACAS2DVecEnv.collect_set, ppo.FusedUpdateSet, ppo.PopulationTrainer).

  CPU  the two symbols and every rejection before a launch; the register guard of csrc/acas2d_ppo_set.hip; the stack /
       member round trip and the population's config rules.
  GPU  a set collection equals K solo collections bit for bit; raw gradients and applied steps per member against the
       float64 references of tests/learner_ref.py, with the criteria and bounds of tests/learner_support.py (the set
       kernels run the solo kernels' body per member, so the same bounds apply), and against the solo update bit for bit
       where there is one wave per network; the trainer's first iteration against K solo PPOTrainer runs; a few iterations
       with the callbacks.
Every criterion prints what it observed."""
import ctypes as C
import os
import random
import re
import types

import numpy as np
import pytest

import helpers as H
import learner_ref as R
import learner_support as LS

torch = pytest.importorskip("torch")
DEV = "cuda:0"
SET_TRAFFIC = (1, 2, 3, 4, 8)          # the five float32 thread-per-env kernels


@pytest.fixture(scope="module")
def g():
    import gym_acas2d_amd as g
    g.native.lib()
    return g


@pytest.fixture(scope="module")
def gpu(g):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return g


# ---- CPU --------------------------------------------------------------------------------------------------------------
def test_set_entry_points_are_exported(g):
    L = g.native.lib()
    assert "acas2d_collect_set_f32" in g.native.EXPORTS and "acas2d_ppo_update_set_f32" in g.native.EXPORTS
    assert L.acas2d_collect_set_f32 and L.acas2d_ppo_update_set_f32
    assert C.sizeof(g.native.CPpoUpdateSet) == 19 * 8 + 4 * 4 + 6 * 8


def test_collect_set_validation_needs_no_gpu(g):
    """acas2d_collect_set_f32 rejects every bad argument with ACAS2D_EINVAL and a message, before any launch (the
    pointers are host addresses: a launch would fail otherwise)."""
    L = g.native.lib()
    buf = (C.c_double * 8192)()
    a = C.addressof(buf)
    st = g.native.CState(*([a] * 14))
    io = g.native.CStepIO(a, a, a, a, a, None, a, a)

    def ac(hidden=64, **none):
        f = {n: a for n, _ in g.native.CPolicy._fields_[:6]}
        f.update({k: v for k, v in none.items() if k in f})
        rest = {n: a for n in ("v1t", "vb1", "v2t", "vb2", "v3", "vb3", "log_std", "values", "logp")}
        rest.update({k: v for k, v in none.items() if k in rest})
        return g.native.CActorCritic(g.native.CPolicy(**f, hidden=hidden, _pad=0), **rest, noise_seed=0, noise_step=0, _pad=0)

    for N in SET_TRAFFIC:
        cfg = g.ACAS2DConfig(n_traffic=N).to_c()

        def call(cfg_=C.byref(cfg), state=C.byref(st), io_=C.byref(io), p=None, K=3, seeds=a, obs=a, T=10, off=0, E=3 * 128,
                 n=N):
            return L.acas2d_collect_set_f32(cfg_, state, io_, C.byref(p) if p is not None else C.byref(ac()), K, seeds, obs,
                                            T, 13, off, E, n, None)

        def rejects(msg, **kw):
            assert call(**kw) == -22, kw
            assert msg.encode() in L.acas2d_last_error(), (kw, L.acas2d_last_error())

        rejects("NULL cfg", cfg_=None)
        rejects("NULL state", state=None)
        rejects("are required", obs=None)
        for K in (0, -2):
            rejects("n_members = %d" % K, K=K)
        for E, K in ((3 * 128 + 64, 3), (3 * 100, 3), (64, 2), (127, 1), (192, 2)):
            rejects("not n_members = %d x a multiple of 64" % K, E=E, K=K)
        for badN in (5, 6, 7, 16, 32, 64):
            rejects("no thread-per-env shape", n=badN)
        rejects("n_traffic = 0", n=0)
        for name in ("w1t", "b1", "w2t", "b2", "w3", "b3"):
            rejects("six weight buffers", p=ac(**{name: None}))
        for name in ("v1t", "vb1", "v2t", "vb2", "v3", "vb3", "log_std", "values", "logp"):
            rejects("value net", p=ac(**{name: None}))
        rejects("NULL noise_seeds", seeds=None)
        rejects("n_steps = 0", T=0)
        rejects("negative", off=-1)
        # the scope is said where a caller meets it
        assert call(n=16) == -22 and b"float64" in L.acas2d_last_error() and b"16 / 32 / 64" in L.acas2d_last_error()
    assert L.acas2d_collect_set_f32(None, None, None, None, 0, None, None, 0, 0, 0, 0, 0, None) == -22


def test_update_set_validation_needs_no_gpu(g):
    """acas2d_ppo_update_set_f32 rejects every bad argument before its first launch."""
    L = g.native.lib()
    buf = (C.c_double * 64)()
    a = C.addressof(buf)
    names = [n for n, _ in g.native.CPpoUpdateSet._fields_]
    ints = dict(n_members=3, n_rows=64, obs_dim=8, apply=0)

    def call(**kw):
        return L.acas2d_ppo_update_set_f32(*LS.host_update_set_args(g, a, **{**ints, **kw}))

    def rejects(msg, **kw):
        assert call(**kw) == -22, kw
        assert msg.encode() in L.acas2d_last_error(), (kw, L.acas2d_last_error())

    for n in names:
        if n not in ints:
            rejects("every pointer is required", **{n: None})
    for K in (0, -1, 65536):
        rejects("n_members = %d" % K, n_members=K)
    for B in (1, 0, -5):
        rejects("n_rows = %d" % B, n_rows=B)
    for D in (0, 5, 9, 53, 101, 197):
        rejects("obs_dim = %d" % D, obs_dim=D)
    assert call(obs_dim=53) == -22 and b"16 / 32 / 64" in L.acas2d_last_error()
    assert L.acas2d_ppo_update_set_f32(None, None) == -22


@H.needs_hipcc
def test_ppo_update_set_kernels_stay_in_registers(tmp_path):
    """csrc/acas2d_ppo_set.hip: five gradient kernels and one apply kernel, no spill of either register file, no
    scratch, at most 256 VGPRs -- test_ppo_update_kernels_stay_in_registers' guard for the new unit."""
    _, kernels = H.kernel_metadata(tmp_path, "acas2d_ppo_set.hip")
    assert len([k for k in kernels if "ppo_grad_set_kernel" in k.name]) == 5
    assert len([k for k in kernels if "ppo_apply_set_kernel" in k.name]) == 1
    assert len(kernels) == 6
    for k in kernels:
        print(k.name, {f: k.field(f) for f in ("vgpr_count", "sgpr_count")})
        assert k.field("vgpr_spill_count") == 0 and k.field("sgpr_spill_count") == 0, k.name
        assert k.field("private_segment_fixed_size") == 0 and k.field("vgpr_count") <= 256, k.name


def test_set_collector_is_five_float32_kernels(g):
    """Mode::CollectSet is value 7 and is launched for one lane per env in float32 only."""
    src = open(os.path.join(H.CSRC, "acas2d_kernels.hpp")).read()
    modes = re.search(r"enum class Mode \{(.*?)\};", src, re.S).group(1)
    names = [ln.split(",")[0].strip() for ln in modes.splitlines() if ln.strip() and not ln.strip().startswith("//")]
    assert names == ["Latch", "Step", "Arena", "Rollout", "Policy", "Collect", "Eval", "CollectSet"]
    assert "launch_collect_set<float>" in open(os.path.join(H.CSRC, "acas2d_f32.hip")).read()
    assert "launch_collect_set" not in open(os.path.join(H.CSRC, "acas2d_f64.hip")).read()


def test_actor_critic_set_round_trip(g):
    torch.manual_seed(5)
    members = [g.ActorCritic(11) for _ in range(4)]
    with torch.no_grad():
        for k, m in enumerate(members):
            m.log_std.fill_(-0.1 * k)
    s = g.ActorCriticSet.from_members(members)
    assert s.n_members == 4 and s.obs_dim == 11
    for n in R.PARAM_NAMES:
        assert s.params[n].shape == (4,) + tuple(members[0].get_parameter(n).shape)
    for k, m in enumerate(members):
        back = s.member(k)
        for n in R.PARAM_NAMES:
            assert H.bits_equal(back.get_parameter(n).detach(), m.get_parameter(n).detach()), (k, n)
        for got, ref in zip(s.actor_weights()[k], m.actor_weights()):
            assert H.bits_equal(got, ref)
    # a member is a copy: writing to it does not reach the stack
    back = s.member(2)
    with torch.no_grad():
        back.log_std.fill_(7.0)
    assert float(s.params["log_std"][2]) == pytest.approx(-0.2)
    w = s.collector_weights()
    assert [tuple(t.shape) for t in w[:6]] == [(4, 11, 64), (4, 64), (4, 64, 64), (4, 64), (4, 64), (4, 1)]
    assert tuple(w[12].shape) == (4,)
    assert torch.equal(w[0][1], members[1].mlp_extractor.policy_net[0].weight.detach().t())
    assert torch.equal(w[8][3], members[3].mlp_extractor.value_net[2].weight.detach().t())
    with pytest.raises(ValueError):
        g.ActorCriticSet.from_members([])
    with pytest.raises(ValueError):
        g.ActorCriticSet.from_members([g.ActorCritic(8), g.ActorCritic(11)])


def test_population_config_rules(g):
    """What the shared launches cannot take is a ValueError at construction, before the env is touched."""
    venv = lambda **kw: types.SimpleNamespace(**{**dict(dtype=torch.float32, n_traffic=1, obs_dim=8, num_envs=3 * 64, device="cpu"), **kw})  # noqa: E731
    cfgs = lambda **kw: [g.PPOConfig(seed=13 + k, **{f: (v[k] if isinstance(v, tuple) else v) for f, v in kw.items()})  # noqa: E731
                         for k in range(3)]
    for field, vals in (("n_steps", (64, 64, 128)), ("batch_size", (256, 512, 256)), ("n_epochs", (4, 4, 5))):
        with pytest.raises(ValueError, match=field):
            g.PopulationTrainer(venv(), cfgs(**{field: vals}))
    with pytest.raises(ValueError, match="float32"):
        g.PopulationTrainer(venv(dtype=torch.float64), cfgs())
    for N in (5, 16, 32, 64):
        with pytest.raises(ValueError, match="n_traffic"):
            g.PopulationTrainer(venv(n_traffic=N, obs_dim=5 + 3 * N), cfgs())
    for E in (3 * 64 + 1, 3 * 100, 64, 200):
        with pytest.raises(ValueError, match="multiple of 64"):
            g.PopulationTrainer(venv(num_envs=E), cfgs())
    with pytest.raises(ValueError):
        g.PopulationTrainer(venv(), [])
    # the fields that MAY differ pass these checks: construction gets as far as the env (a stub without reset())
    with pytest.raises(AttributeError, match="reset"):
        g.PopulationTrainer(venv(), cfgs(learning_rate=(1e-4, 3e-4, 1e-3), clip_range=(0.1, 0.2, 0.3), ent_coef=(0.0, 0.01, 0.0),
                                         vf_coef=(0.5, 0.25, 1.0), max_grad_norm=(0.5, 1.0, 0.5), gamma=(0.99, 0.98, 0.999),
                                         gae_lambda=(0.95, 0.9, 0.95)))


# ---- GPU: the collector ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("config", ("default", "small"))
@pytest.mark.parametrize("EM", (64, 192))
@pytest.mark.parametrize("N", SET_TRAFFIC)
def test_collect_set_equals_solo_collections_bitwise(gpu, N, EM, config):
    """One acas2d_collect_set_f32 launch for K = 3 distinct actor-critics and noise keys against three solo collect()
    launches on envs of EM envs at env_offset + k EM: all nine outputs, obs[T] and the state left behind, compared as
    bit patterns (NaN != NaN).  T runs past max_steps, so every env of every member is reset inside the launch."""
    g = gpu
    K, D = 3, 5 + 3 * N
    kw = {} if config == "default" else H.NONDEFAULT_CONFIGS[config]
    cfg = g.ACAS2DConfig(n_traffic=N, **kw)
    T = cfg.max_steps + 9
    seeds = [0x243F6A8885A308D3, 11, 2 ** 63 + 5]
    pols = LS.members(g, D, K)
    pset = g.ActorCriticSet.from_members(pols)
    off = 37
    env = g.ACAS2DVecEnv(K * EM, N, device=DEV, seed=21, env_offset=off, config=cfg)
    env.reset()
    out = env.collect_set(pset, T, seeds, noise_step=7)
    torch.cuda.synchronize()
    outcomes = set()
    for k in range(K):
        solo = g.ACAS2DVecEnv(EM, N, device=DEV, seed=21, env_offset=off + k * EM, config=cfg)
        solo.reset()
        ref = solo.collect(pols[k], T, noise_seed=seeds[k], noise_step=7)
        torch.cuda.synchronize()
        cols = slice(k * EM, (k + 1) * EM)
        assert H.bits_equal(out["obs"][:, cols], ref["obs"]), (k, "obs")
        for name in LS.OUTPUTS:
            assert H.bits_equal(out[name][:, cols], ref[name]), (k, name)
        for name in LS.STATE:
            assert H.bits_equal(getattr(env, name)[cols], getattr(solo, name)), (k, name)
        assert H.bits_equal(env.outputs["obs"][cols], solo.outputs["obs"]), k
        resets = out["done"][:, cols].sum(0)
        assert int(resets.min()) >= 1, (k, "an env of this member was never reset")
        outcomes |= set(out["outcome"][:, cols][out["done"][:, cols]].unique().tolist())
        print("member %d: %d episodes ended inside the launch" % (k, int(resets.sum())))
    if config == "small" and EM == 192:
        assert outcomes >= {H.COLLISION, H.TIMEOUT}, outcomes
    # the members really differ (a launch that gave every member policy 0 would not pass above; say so directly)
    assert not H.bits_equal(out["actions"][:, :EM], out["actions"][:, EM:2 * EM])


@pytest.mark.gpu
@pytest.mark.parametrize("N", SET_TRAFFIC)
def test_collect_set_routes_each_member_to_its_own_rows(gpu, N):
    """One member whose actor saturates at +1, one at -1, one in between: the rows of each, and only they, show it."""
    g = gpu
    K, EM, D, T = 3, 128, 5 + 3 * N, 20
    pols = LS.members(g, D, K, scale=1.0)
    with torch.no_grad():
        for pol, b in zip(pols, (50.0, -50.0, 0.0)):
            pol.action_net.weight.zero_()
            pol.action_net.bias.fill_(b)
            pol.log_std.fill_(-0.7)
    env = g.ACAS2DVecEnv(K * EM, N, device=DEV, seed=3)
    env.reset()
    out = env.collect_set(g.ActorCriticSet.from_members(pols), T, [1, 2, 3])
    a = out["actions"]
    assert bool((a[:, :EM] > 40).all()) and bool((a[:, EM:2 * EM] < -40).all()) and bool((a[:, 2 * EM:].abs() < 10).all())
    # the env saw the clipped action: the saturated members turn at the limit, in opposite directions
    twin = g.ACAS2DVecEnv(K * EM, N, device=DEV, seed=3)
    twin.reset()
    psi0 = twin.own_psi.clone()
    o, _, done, _ = twin.step(a[0].clamp(-1, 1))
    assert H.bits_equal(o, out["obs"][1]) and H.bits_equal(done, out["done"][0])
    # an env whose episode ended in this very step holds a fresh episode's heading: it says nothing about the turn
    live = ~done
    print("N=%d: %d of %d envs ended their episode in the first step" % (N, int(done.sum()), K * EM))
    assert int(live[:EM].sum()) > EM // 2 and int(live[EM:2 * EM].sum()) > EM // 2
    d = (twin.own_psi - psi0 + 540) % 360 - 180
    assert bool((d[:EM][live[:EM]] > 0).all()) and bool((d[EM:2 * EM][live[EM:2 * EM]] < 0).all())


# ---- GPU: the update ---------------------------------------------------------------------------------------------------
GRAD_CASES = [(D, B) for D in R.UPDATE_WIDTHS for B in (2, 65, 2085, 4096)]


@pytest.mark.gpu
@pytest.mark.parametrize("D,B", GRAD_CASES, ids=["D%d-B%d" % c for c in GRAD_CASES])
def test_update_set_raw_gradients_per_member_vs_float64(gpu, D, B):
    """apply = 0: the gradient launch alone, K = 3 members with different parameters, clip_range 0.1 / 0.2 / 0.3 and
    vf_coef 0.5 / 0.25 / 1.0 on disjoint rows of ONE shared buffer.  Every member's 13 tensors against ppo_loss() in
    float64 autograd (learner_ref.grad64), both old_logp modes; criterion and bounds of test_learner_kernels.py (the
    observed tau is printed per member and case)."""
    g = gpu
    K = 3
    clips, vfs = (0.1, 0.2, 0.3), (0.5, 0.25, 1.0)
    n = K * B + 317
    bt = LS.RolloutBatch(g, D, K, n, seed=3000 + 7 * D + B)
    pset = bt.policy_set()
    segs = R.segments(bt.pols[0])
    worst = 0.0
    for mode, ent in (("mixed", 0.01), ("first", 0.0)):
        cfgs = [g.PPOConfig(ent_coef=ent, clip_range=clips[k], vf_coef=vfs[k], max_grad_norm=0.5) for k in range(K)]
        idx = torch.randperm(n, device=DEV)[:K * B].reshape(K, B).contiguous()       # disjoint rows
        for k in range(K):
            bt.set_old_logp(LS.theta_of(pset, k), idx[k], mode, clips[k])
        fu = g.FusedUpdateSet(pset, cfgs, bt.obs, bt.act, bt.old_logp, bt.adv, bt.ret)
        fu.step_count.copy_(torch.tensor([0, 5, 9999], dtype=torch.int32))
        before = [LS.theta_of(pset, k) for k in range(K)]
        fu.step(idx, apply=False)
        torch.cuda.synchronize()
        assert fu.step_count.cpu().tolist() == [0, 5, 9999]                          # adam_step untouched
        assert float(fu.m.abs().max()) == 0.0 and float(fu.v.abs().max()) == 0.0     # nothing applied
        for k in range(K):
            assert np.array_equal(LS.theta_of(pset, k), before[k]), k
            got = fu.grad[k].double().cpu().numpy()
            got[-1] -= ent                                # (the entropy term is added by the apply launch)
            obs, act, old, adv, ret = bt.host(idx[k])
            ref, pg, vf, ratio = R.grad64(g.ActorCritic, cfgs[k], D, before[k], obs, act, old, adv, ret)
            a = adv - adv.mean()
            if mode == "mixed" and B >= 65:               # the mix actually occurs, at this member's own clip range
                lo, hi = 1 - clips[k], 1 + clips[k]
                for lo_hi in (ratio < lo, ratio > hi):
                    assert (lo_hi & (a > 0)).sum() >= 1 and (lo_hi & (a < 0)).sum() >= 1, (k, B)
                assert ((ratio > lo) & (ratio < hi)).sum() >= 1
            if mode == "first":
                assert np.abs(ratio - 1).max() < 1e-5
            worst = max(worst, LS.assert_per_tensor("raw gradient D=%d B=%d %s member %d" % (D, B, mode, k), got, ref, segs, LS.TAU))
            st = fu.stats[k].double().cpu().numpy()
            print("  pg %.3e vs %.3e, vf %.3e vs %.3e" % (st[0], pg, st[1], vf))
            assert abs(st[0] - pg) <= 1e-5 * max(1.0, abs(pg)) and abs(st[1] - vf) <= 1e-5 * max(1.0, vf)
    print("raw gradients D=%d B=%d: worst observed tau %.2e (bound %.0e)" % (D, B, worst, LS.TAU))


# B is not an input of the apply launch: one partial wave and one many-wave minibatch per width
APPLY_CASES = [(D, B) for D in R.UPDATE_WIDTHS for B in (65, 2085)]


@pytest.mark.gpu
@pytest.mark.parametrize("D,B", APPLY_CASES, ids=["D%d-B%d" % c for c in APPLY_CASES])
def test_update_set_applied_steps_per_member_vs_float64(gpu, D, B):
    """Two applied steps of K = 4 members, each reference step (learner_ref.grad64 + adam64) started from the kernel's OWN
    parameters, moments and step count.  Member 0: clip active (max_grad_norm 0.5), ent_coef 0.01, lr 3e-4, step 0;
    member 1: clip inactive (1e6), lr 1e-3, step 5; member 2: lr 1e-4, step 9 999 with non-zero moments; member 3:
    learning_rate 0 -- it keeps every parameter bit while its moments and step count advance.  Bounds of
    test_fused_update_applied_steps_vs_float64."""
    g = gpu
    K = 4
    lrs, norms, ents, starts = (3e-4, 1e-3, 1e-4, 0.0), (0.5, 1e6, 0.5, 0.5), (0.01, 0.0, 0.0, 0.01), (0, 5, 9999, 3)
    clips, vfs = (0.2, 0.1, 0.3, 0.2), (0.5, 0.25, 1.0, 0.5)
    b1, b2, eps = 0.9, 0.999, 1e-5
    n = K * B + 317
    bt = LS.RolloutBatch(g, D, K, n, seed=4000 + 7 * D + B)
    pset = bt.policy_set()
    segs = R.segments(bt.pols[0])
    cfgs = [g.PPOConfig(ent_coef=ents[k], max_grad_norm=norms[k], learning_rate=lrs[k], clip_range=clips[k], vf_coef=vfs[k])
            for k in range(K)]
    fu = g.FusedUpdateSet(pset, cfgs, bt.obs, bt.act, bt.old_logp, bt.adv, bt.ret)
    fu.step_count.copy_(torch.tensor(starts, dtype=torch.int32))
    rng = np.random.default_rng(B)
    m_pre = rng.normal(0, 1e-2, fu.m.shape[1])                      # moments as a long run leaves them: v >= m^2
    fu.m[2].copy_(torch.as_tensor(m_pre.astype(np.float32), device=DEV))
    fu.v[2].copy_(torch.as_tensor((m_pre ** 2 * rng.uniform(1, 4, m_pre.size) + 1e-8).astype(np.float32), device=DEV))
    worst = {"param": 0.0, "m": 0.0, "v": 0.0, "norm": 0.0, "pg": 0.0, "vf": 0.0}
    for step in range(2):
        idx = torch.randperm(n, device=DEV)[:K * B].reshape(K, B).contiguous()
        for k in range(K):
            bt.set_old_logp(LS.theta_of(pset, k), idx[k], "mixed", clips[k])           # from the member's CURRENT parameters
        theta0 = [LS.theta_of(pset, k) for k in range(K)]
        m0, v0 = fu.m.double().cpu().numpy(), fu.v.double().cpu().numpy()
        s0 = fu.step_count.cpu().tolist()
        fu.step(idx)
        torch.cuda.synchronize()
        assert fu.step_count.cpu().tolist() == [s + 1 for s in s0]                   # every member advanced by one
        assert float(fu.grad.abs().max()) == 0.0
        assert float(fu.stats[:, 0:2].abs().max()) == 0.0
        m1, v1 = fu.m.double().cpu().numpy(), fu.v.double().cpu().numpy()
        for k in range(K):
            what = "D=%d B=%d member %d step %d" % (D, B, k, s0[k] + 1)
            obs, act, old, adv, ret = bt.host(idx[k])
            grad, pg, vf, _ = R.grad64(g.ActorCritic, cfgs[k], D, theta0[k], obs, act, old, adv, ret)
            theta_ref, m_ref, v_ref, norm = R.adam64(theta0[k], grad, m0[k], v0[k], s0[k], norms[k], lrs[k], b1, b2, eps)
            assert (norm > norms[k]) == (norms[k] < 1.0), (what, norm)                # active / inactive as meant
            st = fu.stats[k].double().cpu().numpy()
            for key, got_, ref_, tol in (("norm", st[2], norm, 1e-5 * norm), ("pg", st[4], pg, 1e-5 * max(1.0, abs(pg))),
                                         ("vf", st[5], vf, 1e-5 * max(1.0, vf))):
                worst[key] = max(worst[key], abs(got_ - ref_) / tol)
                assert abs(got_ - ref_) <= tol, (what, key, got_, ref_)
            worst["m"] = max(worst["m"], LS.assert_per_tensor("m " + what, m1[k], m_ref, segs, LS.TAU_M))
            worst["v"] = max(worst["v"], LS.assert_per_tensor("v " + what, v1[k], v_ref, segs, LS.TAU_V))
            theta1 = LS.theta_of(pset, k)
            if lrs[k] == 0.0:                             # isolation: a member that does not learn keeps every bit
                assert np.array_equal(theta1, theta0[k]), what
                assert np.abs(m1[k] - m0[k]).max() > 0
                continue
            ulp = np.spacing(np.abs(theta_ref).astype(np.float32)).astype(np.float64)
            excess = (np.abs(theta1 - theta_ref) - ulp) / lrs[k]
            worst["param"] = max(worst["param"], float(excess.max()))
            assert excess.max() <= 1e-2, (what, float(excess.max()), int(excess.argmax()))
            assert np.median(np.abs(theta1 - theta0[k]) / lrs[k]) > 0.05, what         # the step was taken
    print("applied steps D=%d B=%d: worst param excess %.2e lr (bound 1e-2), m tau %.2e (bound %.0e), v tau %.2e (bound "
          "%.0e), norm / pg / vf at %.2f / %.2f / %.2f of their 1e-5 bounds"
          % (D, B, worst["param"], worst["m"], LS.TAU_M, worst["v"], LS.TAU_V, worst["norm"], worst["pg"], worst["vf"]))


BITWISE_CASES = [(D, B) for D in R.UPDATE_WIDTHS for B in (2, 63, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("D,B", BITWISE_CASES, ids=["D%d-B%d" % c for c in BITWISE_CASES])
def test_update_set_single_wave_equals_solo_bitwise(gpu, D, B):
    """The set kernels and the solo kernels run ONE body (csrc/acas2d_ppo.hpp: grad_narrow, apply_body), so where the
    result does not depend on the order of the atomics it is the same bits: with B <= 64 there is one wave per network,
    every gradient entry receives exactly one atomic add onto zero, and the apply kernel's reduction order is fixed.
    K = 3 members with different weights, minibatches and hyper-rows (and Adam step counts) on one shared buffer, through
    FusedUpdateSet; the same member by member through FusedUpdate on the same buffer.  First the raw gradient (apply=False
    against the solo probe max_grad_norm < 0), then three applied steps, compared after each: grad, the 13 parameters, m,
    v, step_count, stats[2] / [4] / [5] with torch.equal.  B = 2 and 63 leave dead lanes, B = 64 fills the wave."""
    g = gpu
    K = 3
    hyper = dict(clip_range=(0.1, 0.2, 0.3), vf_coef=(0.5, 0.25, 1.0), ent_coef=(0.01, 0.0, 0.02),
                 max_grad_norm=(0.5, 1e6, 0.3), learning_rate=(3e-4, 1e-3, 1e-4))
    cfgs = [g.PPOConfig(**{f: v[k] for f, v in hyper.items()}) for k in range(K)]
    probes = [g.PPOConfig(**{**{f: v[k] for f, v in hyper.items()}, "max_grad_norm": -1.0}) for k in range(K)]
    n = K * B + 317
    bt = LS.RolloutBatch(g, D, K, n, seed=5000 + 7 * D + B)
    pset = bt.policy_set()
    idx = torch.randperm(n, device=DEV)[:K * B].reshape(K, B).contiguous()           # disjoint rows
    for k in range(K):
        bt.set_old_logp(LS.theta_of(pset, k), idx[k], "mixed", hyper["clip_range"][k])
    solo = [pset.member(k) for k in range(K)]                                     # copies, before anything is applied
    bufs = (bt.obs, bt.act, bt.old_logp, bt.adv, bt.ret)

    def same(what, a, b):
        assert a.shape == b.shape and torch.equal(a, b), (what, D, B, float((a.double() - b.double()).abs().max()))

    fs = g.FusedUpdateSet(pset, cfgs, *bufs)
    fs.step(idx, apply=False)
    for k in range(K):
        fu = g.FusedUpdate(solo[k], probes[k], *bufs)
        fu.step(idx[k].contiguous())
        assert float(fu.grad.abs().max()) > 0.0
        same("raw gradient, member %d" % k, fs.grad[k], fu.grad)
        same("raw losses, member %d" % k, fs.stats[k, 0:2], fu.stats[0:2])

    fs = g.FusedUpdateSet(pset, cfgs, *bufs)
    fus = [g.FusedUpdate(solo[k], cfgs[k], *bufs) for k in range(K)]
    starts = (0, 5, 9999)
    fs.step_count.copy_(torch.tensor(starts, dtype=torch.int32))
    for k in range(K):
        fus[k].step_count.fill_(starts[k])
    for step in range(3):
        rows = idx[:, torch.randperm(B, device=DEV)].contiguous()                   # the same rows on other lanes
        fs.step(rows)
        for k in range(K):
            fus[k].step(rows[k].contiguous())
            what = "member %d, applied step %d: " % (k, step + 1)
            same(what + "grad", fs.grad[k], fus[k].grad)
            for name in R.PARAM_NAMES:
                same(what + name, pset.params[name][k], solo[k].get_parameter(name).detach())
            same(what + "m", fs.m[k], fus[k].m)
            same(what + "v", fs.v[k], fus[k].v)
            same(what + "step_count", fs.step_count[k:k + 1], fus[k].step_count)
            for slot in (2, 4, 5):
                same(what + "stats[%d]" % slot, fs.stats[k, slot], fus[k].stats[slot])
    assert fs.step_count.cpu().tolist() == [s + 3 for s in starts]
    moved = max(float((pset.params[R.PARAM_NAMES[2]][k] - bt.pols[k].get_parameter(R.PARAM_NAMES[2]).detach()).abs().max())
                for k in range(K))
    assert moved > 0.0                                                               # the steps were taken


# ---- GPU: the trainer --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("N", (1, 8))
def test_population_first_iteration_equals_solo_trainers(gpu, N):
    """K = 3 members with different seeds and learning rates (at N = 8 also different gamma / lambda), EM = 256: the
    buffers of the first collection equal three solo PPOTrainer(collector="fused", updater="fused") on env_offset =
    k EM bit for bit, GAE equals compute_gae on the member's own columns, and the last values are the critics'."""
    g = gpu
    K, EM, D, T = 3, 256, 5 + 3 * N, 24
    gam = (0.99, 0.99, 0.99) if N == 1 else (0.99, 0.98, 0.999)
    lam = (0.95, 0.95, 0.95) if N == 1 else (0.95, 0.9, 0.97)
    cfgs = [g.PPOConfig(seed=13 + k, learning_rate=(1e-4, 3e-4, 1e-3)[k], gamma=gam[k], gae_lambda=lam[k], n_steps=T,
                        batch_size=1024, n_epochs=2) for k in range(K)]
    ecfg = g.ACAS2DConfig(n_traffic=N, max_steps=15)                  # short episodes: dones inside the first collection
    venv = g.ACAS2DVecEnv(K * EM, N, device=DEV, seed=13, config=ecfg)
    pop = g.PopulationTrainer(venv, cfgs)
    pop.collect()
    torch.cuda.synchronize()
    for k in range(K):
        solo_env = g.ACAS2DVecEnv(EM, N, device=DEV, seed=13, env_offset=k * EM, config=ecfg)
        tr = g.PPOTrainer(solo_env, cfgs[k], collector="fused", updater="fused")
        for name in R.PARAM_NAMES:                                    # the member starts from the solo trainer's weights
            assert H.bits_equal(pop.policy_set.params[name][k], tr.policy.get_parameter(name).detach()), (k, name)
        tr.collect()
        torch.cuda.synchronize()
        cols = slice(k * EM, (k + 1) * EM)
        for name in ("b_obs", "b_act", "b_logp", "b_val", "b_rew", "b_done"):
            assert H.bits_equal(getattr(pop, name)[:, cols], getattr(tr, name)), (k, name)
        assert bool(pop.b_done[:, cols].any())
        if N == 1:
            gk, lk = cfgs[k].gamma, cfgs[k].gae_lambda                # equal across members: the numbers themselves
        else:
            gk, lk = (torch.tensor(v, dtype=torch.float32, device=DEV) for v in (cfgs[k].gamma, cfgs[k].gae_lambda))
        adv, ret = g.compute_gae(pop.b_rew[:, cols], pop.b_val[:, cols], pop.b_done[:, cols], pop.last_value[cols], gk, lk)
        assert H.bits_equal(pop.b_adv[:, cols], adv) and H.bits_equal(pop.b_ret[:, cols], ret), k
        if N == 1:                                                    # ... and then the solo trainer's own, to rounding
            assert float((pop.b_adv[:, cols] - tr.b_adv).abs().max()) <= 1e-4 * max(1.0, float(tr.b_adv.abs().max()))
        _, v64 = R.forward64(R.params64(pop.member(k)), pop.obs[cols].double().cpu().numpy(), sample=True)
        got = pop.last_value[cols].double().cpu().numpy()
        rel = float((np.abs(got - v64) / np.maximum(1.0, np.abs(v64))).max())
        print("member %d: last values within %.2e of float64 (bound 5e-6)" % (k, rel))
        assert rel <= 5e-6
    assert pop.num_timesteps == T * EM


@pytest.mark.gpu
def test_population_learns_a_few_iterations_with_callbacks(gpu, tmp_path):
    g = gpu
    K, EM, N, T = 3, 256, 1, 32
    cfgs = [g.PPOConfig(seed=13 + k, learning_rate=(1e-4, 3e-4, 1e-3)[k], n_steps=T, batch_size=2048, n_epochs=2)
            for k in range(K)]
    venv = g.ACAS2DVecEnv(K * EM, N, device=DEV, seed=13, config=g.ACAS2DConfig(n_traffic=N, max_steps=40))
    pop = g.PopulationTrainer(venv, cfgs)
    start = [{n: pop.policy_set.params[n][k].clone() for n in R.PARAM_NAMES} for k in range(K)]
    per_it, iters, n_eval = T * EM, 3, 10
    hist = pop.learn(iters * per_it, log=None, eval_every=per_it, eval_episodes=n_eval, eval_seed=99, save_dir=str(tmp_path),
                     checkpoint_every=per_it)
    assert pop.num_timesteps == iters * per_it
    train = [r for r in hist if not r.get("eval")]
    evals = [r for r in hist if r.get("eval")]
    assert sorted((r["member"], r["iteration"]) for r in train) == [(k, i) for k in range(K) for i in range(1, iters + 1)]
    assert len(evals) == K * iters and hist is pop.history
    for r in train:
        assert np.isfinite([r["pg_loss"], r["value_loss"], r["std"]]).all() and r["timesteps"] == r["iteration"] * per_it
    assert pop.optimizer_state()["step"] == [iters * 2 * (per_it // 2048)] * K
    for k in range(K):
        for n in R.PARAM_NAMES:
            p = pop.policy_set.params[n][k]
            assert bool(torch.isfinite(p).all()), (k, n)
        moved = max(float((pop.policy_set.params[n][k] - start[k][n]).abs().max()) for n in R.PARAM_NAMES)
        assert moved > 1e-4, (k, moved)
    for a, b in ((0, 1), (1, 2), (0, 2)):
        assert not torch.equal(pop.policy_set.params[R.PARAM_NAMES[2]][a], pop.policy_set.params[R.PARAM_NAMES[2]][b])
    # the files, member by member
    rng = random.Random(99)
    episodes = [g.reset_parity.draw_episodes(venv.config, n_eval, rng) for _ in range(iters)]
    own, trf, goal = episodes[-1]
    final = g.evaluate_policies_fused(pop.policy_set.actor_weights(), own, trf, goal, dtype=torch.float32, device=DEV,
                                      config=venv.config)
    for k in range(K):
        d = tmp_path / ("member_%d" % k)
        ev = np.load(d / "results" / "evaluations.npz")
        assert ev["timesteps"].tolist() == [per_it * (i + 1) for i in range(iters)]
        assert ev["results"].shape == (iters, n_eval) and ev["ep_lengths"].shape == (iters, n_eval)
        # the recorded evaluation of the last iteration is row k of one evaluate_policies_fused launch on the weights left
        assert np.array_equal(ev["results"][-1], final["total_reward"][k].astype(np.float64)), k
        assert np.array_equal(ev["ep_lengths"][-1], final["steps"][k].astype(np.int64) - 1), k
        mine = [r for r in evals if r["member"] == k]
        assert [r["mean_reward"] for r in mine] == [float(row.mean()) for row in ev["results"]]
        ckpts = sorted(os.listdir(d / "checkpoints"))
        assert ckpts == sorted("model_%d_steps.zip" % (per_it * (i + 1)) for i in range(iters))
        last = g.load_sb3_policy(str(d / "checkpoints" / ("model_%d_steps.zip" % (iters * per_it))))
        for got, ref in zip(last.actor_weights(), pop.member(k).actor_weights()):
            assert H.bits_equal(got.cpu(), ref.cpu()), k
        best_t = [r["timesteps"] for r in mine if r["new_best"]][-1]
        best = g.load_sb3_policy(str(d / "best_model.zip"))
        at_best = g.load_sb3_policy(str(d / "checkpoints" / ("model_%d_steps.zip" % best_t)))
        for got, ref in zip(best.actor_weights(), at_best.actor_weights()):
            assert H.bits_equal(got, ref), k
