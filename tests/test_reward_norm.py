"""acas2d_reward_normalize_f32 (csrc/acas2d_rewnorm.hip), ppo.RewardNormalizer and the trainers' reward_norm= option: SB3's
VecNormalize(norm_obs=False, norm_reward=True) on the device.

The referee is tests/rewnorm_ref.py, a float64 NumPy restatement of the contract in include/acas2d.h with the order of the
two sums over a member's envs as a parameter.  The bounds between kernel and referee are those between the referee's two
summation orders, and the CPU part holds the referee to them first:
  out      every entry within 1 float32 ulp, at most 0.1 % of the entries different at all;
  stats, returns   within 4 T (EM + 8) 2^-53 relative (the worst-case growth of a float64 sum of EM terms, re-ordered,
           through T merges); count exactly.
Reproducibility, chunk invariance, member independence and in place = out of place are held bit for bit."""
import ctypes as C
import dataclasses
import os
import types

import numpy as np
import pytest

import helpers as H
import rewnorm_ref as R

torch = pytest.importorskip("torch")
DEV = "cuda:0"

# (T, E, K): the smallest call, a lone env, tail lanes, more than one wave with a tail, members of one and two waves, a row
# of 16 columns per lane; then T on each side of the sweep's block depth (16) and of twice it
SHAPES = [(1, 1, 1), (17, 1, 1), (33, 63, 1), (97, 130, 1), (33, 192, 3), (48, 256, 2), (40, 1024, 1),
          (15, 65, 1), (16, 65, 1), (31, 128, 2), (32, 65, 1)]
DONE_PATTERNS = ("none", "all", "ends", "one_env", "random")
GAMMAS = (0.99, 0.97, 0.999)


def make_inputs(T, E, pattern, seed, infinities=False):
    """N(0, 1) rewards with +-1000 spikes and NaN; `infinities`: one -inf and one +inf as well, in different envs (where
    there are two) of the last three rows -- an infinity drives var to ~1e76 and flattens everything after it.  Dones by
    `pattern`, as tests/test_gae_kernel.py's."""
    rng = np.random.default_rng(seed)
    rew = rng.normal(0, 1, (T, E)).astype(np.float32)
    rew[rng.random((T, E)) < 0.05] = 1000.0
    rew[rng.random((T, E)) < 0.05] = -1000.0
    rew[rng.random((T, E)) < 0.04] = np.nan
    rew[T // 2, 0] = np.nan                               # (one for certain)
    if infinities:
        rew[max(T - 3, 0), 2 % E] = -np.inf
        rew[T - 1, 1 % E] = np.inf
    done = np.zeros((T, E), bool)
    if pattern == "all":
        done[:] = True
    elif pattern == "ends":
        done[0], done[T - 1] = True, True
    elif pattern == "one_env":
        done[:, E // 2] = True
    elif pattern == "random":
        done = rng.random((T, E)) < 0.15
    return rew, done


def cases(T, E):
    """(what, reward, done, clip) for every done pattern: the finite family at clip 10 and 2, the infinities at clip 10."""
    for pi, pattern in enumerate(DONE_PATTERNS):
        seed = 100 * T + E + pi
        rew, done = make_inputs(T, E, pattern, seed)
        yield (pattern, "finite", 10.0), rew, done, 10.0
        yield (pattern, "finite", 2.0), rew, done, 2.0
        rew, done = make_inputs(T, E, pattern, seed, infinities=True)
        yield (pattern, "infinities", 10.0), rew, done, 10.0


def ordered(a):
    """float32 bit patterns as integers in the order of the values: the difference of two is their distance in ulps."""
    u = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(u < 0, -(u & 0x7fffffff), u)


def check_within_bounds(what, got, ref, T, EM):
    """(out, returns, stats) against the referee's, by the bounds of the module docstring; every figure is printed."""
    (out, ret, st), (out_r, ret_r, st_r) = got, ref
    assert np.isfinite(out).all() and np.isfinite(out_r).all(), what
    ulps = np.abs(ordered(out) - ordered(out_r))
    bound = 4.0 * T * (EM + 8) * 2.0 ** -53
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.where(b == 0, 1.0, np.abs(b)), initial=0.0))  # noqa: E731
    zeros_agree = np.array_equal(ret == 0, ret_r == 0) and np.array_equal(st == 0, st_r == 0)
    figures = dict(max_ulp=int(ulps.max()), differing=int((ulps != 0).sum()), of=out.size, rel_returns=rel(ret, ret_r),
                   rel_mean=rel(st[:, 0], st_r[:, 0]), rel_var=rel(st[:, 1], st_r[:, 1]), bound=bound)
    print(what, figures)
    assert ulps.max() <= 1 and (ulps != 0).sum() <= 0.001 * out.size, (what, figures)
    assert zeros_agree, what
    assert figures["rel_returns"] <= bound and figures["rel_mean"] <= bound and figures["rel_var"] <= bound, (what, figures)
    assert np.array_equal(st[:, 2], st_r[:, 2]), (what, st[:, 2], st_r[:, 2])


def same_bits(a, b):
    a, b = (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x) for x in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- CPU -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,E,K", SHAPES)
def test_restatement_orders_agree_within_the_bounds_and_chunks_bitwise(T, E, K):
    """NumPy's summation order against the sequential one: the bounds the kernel is held to are not fitted to the kernel.
    And the restatement over T rows equals itself over T1 rows and the rest with the carried state, bit for bit."""
    for what, rew, done, clip in cases(T, E):
        ret0, st0 = R.fresh_state(E, K)
        a = R.normalize(rew, done, ret0, st0, GAMMAS[:K], clip=clip, n_members=K, order="numpy")
        b = R.normalize(rew, done, ret0, st0, GAMMAS[:K], clip=clip, n_members=K, order="sequential")
        check_within_bounds((T, E, K) + what, a, b, T, E // K)
        assert (np.isnan(rew).any() or T * E == 1) and (what[1] != "infinities" or np.isinf(rew).any())
        if clip == 2.0 and T * E > 17:
            assert (np.abs(a[0]) == 2.0).any()            # the clip is hit (wherever there is room for a spike)
        for T1 in sorted({1, T // 2, T - 1} - {0, T}):
            for order, whole in (("numpy", a), ("sequential", b)):
                o1, r1, s1 = R.normalize(rew[:T1], done[:T1], ret0, st0, GAMMAS[:K], clip=clip, n_members=K, order=order)
                o2, r2, s2 = R.normalize(rew[T1:], done[T1:], r1, s1, GAMMAS[:K], clip=clip, n_members=K, order=order)
                assert same_bits(np.concatenate((o1, o2)), whole[0]) and same_bits(r2, whole[1]) and same_bits(s2, whole[2])


@pytest.mark.parametrize("T,E,K", SHAPES)
def test_torch_reference_equals_the_restatement_within_the_bounds(T, E, K):
    """ppo.normalize_rewards_reference, the documented slow path, on the CPU; in place as well."""
    from gym_acas2d_amd.ppo import normalize_rewards_reference
    for what, rew, done, clip in cases(T, E):
        ret0, st0 = R.fresh_state(E, K)
        ref = R.normalize(rew, done, ret0, st0, GAMMAS[:K], clip=clip, n_members=K)
        ret, st = torch.as_tensor(ret0.copy()), torch.as_tensor(st0.copy())
        buf = torch.as_tensor(rew.copy())
        out = normalize_rewards_reference(buf, torch.as_tensor(done), ret, st, GAMMAS[:K], clip_reward=clip, n_members=K,
                                          out=buf)
        assert out is buf
        check_within_bounds((T, E, K) + what, (out.numpy(), ret.numpy(), st.numpy()), ref, T, E // K)


def _valid(native, **over):
    """A struct every check accepts (made-up addresses: nothing may be launched with it), then `over`."""
    f = dict(reward=0x1000, done=0x2000, out=0x3000, returns=0x4000, stats=0x5000, gamma=0x6000, workspace=0x7000,
             epsilon=1e-8, clip=10.0, n_envs=192, n_steps=8, n_members=1)
    f.update(over)
    return native.CRewardNorm(**f)


def test_reward_norm_rejections_and_struct_size_without_a_device():
    from gym_acas2d_amd import native
    L = native.lib()
    assert L.acas2d_reward_norm_size() == C.sizeof(native.CRewardNorm)
    assert L.acas2d_reward_norm_pipeline_depth() == 16
    assert L.acas2d_reward_norm_workspace_bytes(192, 8, 3) >= 8 * (8 * 192 + 3 * 8 * 3)
    assert L.acas2d_reward_norm_workspace_bytes(0, 8, 1) == 0 and L.acas2d_reward_norm_workspace_bytes(2 ** 31, 8, 1) == 0
    names = ("reward", "done", "out", "returns", "stats", "gamma", "workspace")
    cases = [("NULL struct", None)] + [("NULL " + n, {n: None}) for n in names]
    cases += [("n_steps 0", dict(n_steps=0)), ("n_envs 0", dict(n_envs=0)), ("n_members 0", dict(n_members=0)),
              ("n_envs 2^31", dict(n_envs=2 ** 31)), ("K = 3, EM = 65", dict(n_members=3, n_envs=195)),
              ("K = 2, odd split", dict(n_members=2, n_envs=193)), ("K = 2, EM = 32", dict(n_members=2, n_envs=64))]
    for field in ("epsilon", "clip"):
        for v in (0.0, -1.0, float("inf"), float("nan")):
            cases.append(("%s = %r" % (field, v), {field: v}))
    base = _valid(native)
    for w in ("out", "returns", "stats", "workspace"):
        for other in names:
            if other != w and (w, other) != ("out", "reward"):
                cases.append(("%s == %s" % (w, other), {w: getattr(base, other)}))
                cases.append(("%s == %s" % (other, w), {other: getattr(base, w)}))
    for n in ("returns", "stats", "gamma", "workspace"):
        cases.append(("misaligned " + n, {n: getattr(base, n) + 4}))
    for what, over in cases:
        rc = (L.acas2d_reward_normalize_f32(None, None) if over is None
              else L.acas2d_reward_normalize_f32(C.byref(_valid(native, **over)), None))
        assert rc == -22, (what, rc)
        assert L.acas2d_last_error().startswith(b"acas2d_reward_normalize"), what
    # python's own checks, before anything is launched
    from gym_acas2d_amd.ppo import RewardNormalizer
    for kw in (dict(n_envs=190, n_members=2), dict(n_envs=0), dict(n_envs=64, epsilon=0.0), dict(n_envs=64, clip_reward=-1.0),
               dict(n_envs=128, n_members=2, gamma=[0.9, 0.9, 0.9])):
        with pytest.raises(ValueError):
            RewardNormalizer(device="cpu", **kw)
    n = RewardNormalizer(128, 2, gamma=[0.9, 0.99], device="cpu")
    assert n.stats.tolist() == [[0.0, 1.0, 1e-4]] * 2 and n.gamma.tolist() == [0.9, 0.99] and not bool(n.returns.any())
    with pytest.raises(ValueError, match="GPU"):
        n.normalize(torch.zeros(2, 128), torch.zeros(2, 128, dtype=torch.bool))


def test_reward_norm_is_a_trainer_argument_and_never_a_config_field():
    """Nothing is launched: the rules are checked before the env is touched (a stub env: an accepted construction gets as
    far as its missing reset())."""
    import gym_acas2d_amd as g
    fields = [f.name for f in dataclasses.fields(g.PPOConfig)]
    assert not [f for f in fields + list(g.ppo.MEMBER_FIELDS) + list(g.ppo.HYPER_SLOTS) if "norm" in f and f != "max_grad_norm"]
    venv = types.SimpleNamespace(dtype=torch.float32, n_traffic=1, obs_dim=8, num_envs=128, device="cpu")
    for kw in (dict(use_graphs=False), dict(use_graphs=True), dict(use_graphs=True, collector="graphs", updater="fused"),
               dict(use_graphs=True, collector="eager")):
        with pytest.raises(ValueError, match="collector='fused'"):
            g.PPOTrainer(venv, g.PPOConfig(), reward_norm=True, **kw)
    cfg = g.PPOConfig()
    with pytest.raises(AttributeError, match="reset"):       # the fused collector takes it
        g.PPOTrainer(venv, cfg, use_graphs=True, collector="fused", updater="fused", reward_norm=True)
    assert [f.name for f in dataclasses.fields(cfg)] == fields and not hasattr(cfg, "reward_norm")
    cfgs = [g.PPOConfig(seed=k) for k in range(2)]
    for bad in ("yes", 1.5):
        with pytest.raises(TypeError, match="reward_norm"):
            g.PopulationTrainer(venv, cfgs, reward_norm=bad)
    with pytest.raises(AttributeError, match="reset"):
        g.PopulationTrainer(venv, cfgs, reward_norm=True)
    with pytest.raises(AttributeError, match="reset"):
        g.PBTTrainer(venv, cfgs, g.PBTConfig(ready_every=1), reward_norm=True)


@H.needs_hipcc
def test_reward_norm_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    """The code-object metadata of csrc/acas2d_rewnorm.hip, read the way tests/test_gae_kernel.py reads its unit."""
    _, kernels = H.kernel_metadata(tmp_path, "acas2d_rewnorm.hip")
    assert sorted(k.name.split("rewnorm_")[1].split("_kernel")[0] for k in kernels) == ["merge", "moments", "scale", "sweep"]
    for k in kernels:
        print(k.name, "vgpr", k.field("vgpr_count"), "sgpr", k.field("sgpr_count"))
        assert k.field("vgpr_spill_count") == 0 and k.field("sgpr_spill_count") == 0, k.name
        assert k.field("private_segment_fixed_size") == 0 and k.field("vgpr_count") <= 256, k.name


# ---- GPU: the entry ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g():
    import gym_acas2d_amd as g
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    g.native.lib()
    return g


def _run(g, rew_d, done_d, K, gamma, clip, pieces=None, in_place=False):
    """A fresh RewardNormalizer over the rows of rew_d, whole or in `pieces` (row ranges); (out, returns, stats) as NumPy."""
    T, E = rew_d.shape
    n = g.RewardNormalizer(E, K, gamma=gamma, clip_reward=clip, device=DEV)
    buf = rew_d.clone() if in_place else rew_d
    outs = []
    for lo, hi in pieces or [(0, T)]:
        o = n.normalize(buf[lo:hi], done_d[lo:hi], out=buf[lo:hi] if in_place else None)
        assert not in_place or o.data_ptr() == buf[lo:hi].data_ptr()
        outs.append(o)
    torch.cuda.synchronize()
    return torch.cat(outs).cpu().numpy(), n.returns.cpu().numpy(), n.stats.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("T,E,K", SHAPES)
def test_reward_normalize_against_the_restatement_and_its_bitwise_properties(g, T, E, K):
    assert int(g.native.lib().acas2d_reward_norm_pipeline_depth()) == 16            # SHAPES straddles it
    EM, gam = E // K, GAMMAS[:K]
    for what, rew, done, clip in cases(T, E):
        what = (T, E, K) + what
        ref = R.normalize(rew, done, *R.fresh_state(E, K), gam, clip=clip, n_members=K)
        rew_d, done_d = torch.as_tensor(rew, device=DEV), torch.as_tensor(done, device=DEV)
        got = _run(g, rew_d, done_d, K, gam, clip)
        check_within_bounds(what, got, ref, T, EM)
        assert not got[1][done[T - 1]].any(), what        # returns: 0 exactly where the last row is done
        if clip == 2.0:
            assert T * E <= 17 or (np.abs(got[0]) == 2.0).any(), what
            continue                                      # (the clip touches `out` alone: the properties below at 10)
        same = lambda other: all(same_bits(a, b) for a, b in zip(got, other))  # noqa: E731
        assert same(_run(g, rew_d, done_d, K, gam, clip)), ("two runs",) + what
        assert same(_run(g, rew_d, done_d.view(torch.uint8), K, gam, clip, in_place=True)), ("in place",) + what
        for T1 in sorted({1, T // 2, T - 1} - {0, T}):
            assert same(_run(g, rew_d, done_d, K, gam, clip, pieces=[(0, T1), (T1, T)])), ("chunked", T1) + what
        if K > 1:
            solo = [_run(g, rew_d[:, k * EM:(k + 1) * EM].contiguous(), done_d[:, k * EM:(k + 1) * EM].contiguous(), 1,
                         gam[k], clip) for k in range(K)]
            joined = [np.concatenate([s[i] for s in solo], axis=-1 if i < 2 else 0) for i in range(3)]
            assert same(joined), ("members",) + what


@pytest.mark.gpu
def test_reward_normalizer_says_what_it_cannot_take(g):
    n = g.RewardNormalizer(128, device=DEV)
    z, d = torch.zeros(4, 128, device=DEV), torch.zeros(4, 128, dtype=torch.bool, device=DEV)
    with pytest.raises(ValueError, match="one shape"):
        n.normalize(z[:, :64], d[:, :64])
    with pytest.raises(ValueError, match="float32"):
        n.normalize(z.double(), d)
    with pytest.raises(ValueError, match="contiguous"):
        n.normalize(z.t().contiguous().t(), d)
    with pytest.raises(ValueError, match="out must be"):
        n.normalize(z, d, out=torch.zeros(2, 128, device=DEV))
    assert n.stats.cpu().tolist() == [[0.0, 1.0, 1e-4]]    # nothing ran


# ---- GPU: the trainers ---------------------------------------------------------------------------------------------------
def _solo(g, reward_norm=True, seed=13, **kw):
    venv = g.ACAS2DVecEnv(128, 1, device=DEV, dtype=torch.float32, seed=13, config=g.ACAS2DConfig(n_traffic=1, max_steps=12))
    cfg = g.PPOConfig(n_steps=16, batch_size=512, n_epochs=1, seed=seed, gamma=0.98)
    return g.PPOTrainer(venv, cfg, collector="fused", updater="fused", gae="kernel", reward_norm=reward_norm, **kw)


@pytest.mark.gpu
def test_ppo_trainer_normalises_the_rollout_rewards_before_gae(g):
    """Two collect() calls: b_rew is the restatement over both iterations' RAW rewards (the collector's output dict) with
    the carried state; GAE ran on it (compute_gae's bits); the episode returns stay raw; update() reports reward_std."""
    tr = _solo(g)
    T, E = 16, 128
    raw, dones, normed = [], [], []
    for _ in range(2):
        tr.collect()
        raw.append(tr._fused_out["reward"].float().cpu().numpy().copy())
        dones.append(tr.b_done.cpu().numpy().copy())
        normed.append(tr.b_rew.cpu().numpy().copy())
    torch.cuda.synchronize()
    raw, dones = np.concatenate(raw), np.concatenate(dones)
    assert dones.any() and np.abs(raw).max() > 0
    ref = R.normalize(raw, dones, *R.fresh_state(E), 0.98)
    n = tr.reward_norm
    check_within_bounds("PPOTrainer", (np.concatenate(normed), n.returns.cpu().numpy(), n.stats.cpu().numpy()), ref, 2 * T, E)
    assert not same_bits(normed[1], raw[T:])
    with torch.no_grad():
        _, last_value = tr.policy.forward(tr.obs)
    adv, ret = g.compute_gae(tr.b_rew, tr.b_val, tr.b_done, last_value, tr.cfg.gamma, tr.cfg.gae_lambda)
    assert same_bits(tr.b_adv, adv) and same_bits(tr.b_ret, ret)
    st = tr.update()
    assert abs(st["reward_std"] / np.sqrt(ref[2][0, 1] + 1e-8) - 1) <= 4.0 * 2 * T * (E + 8) * 2.0 ** -53
    # raw episode returns: what an identically seeded trainer without the option sees in its first collection
    plain, again = _solo(g, reward_norm=None), _solo(g)
    plain.collect()
    again.collect()
    assert plain.reward_norm is None and "reward_std" not in plain.update()
    assert same_bits(plain.b_epret, again.b_epret) and same_bits(plain.b_done, again.b_done)
    assert same_bits(again.b_rew, normed[0]) and not same_bits(plain.b_rew, again.b_rew)


@pytest.mark.gpu
def test_reward_norm_off_issues_no_call(g, monkeypatch):
    import learner_support as S
    calls = S.count_calls(g, monkeypatch, "acas2d_reward_normalize_f32")
    tr = _solo(g, reward_norm=None)
    S.iterate(tr)
    assert calls == []
    tr = _solo(g)
    S.iterate(tr)
    assert len(calls) == 1


def _population(g, K, pbt=None, reward_norm=True, T=16, gammas=None):
    cfgs = [g.PPOConfig(seed=13 + k, n_steps=T, batch_size=256, n_epochs=1, learning_rate=3e-4 * (1 + k),
                        gamma=(gammas or [0.98] * K)[k]) for k in range(K)]
    venv = g.ACAS2DVecEnv(K * 64, 1, device=DEV, dtype=torch.float32, seed=13, config=g.ACAS2DConfig(n_traffic=1, max_steps=12))
    if pbt is None:
        return g.PopulationTrainer(venv, cfgs, gae="kernel", reward_norm=reward_norm)
    return g.PBTTrainer(venv, cfgs, pbt, gae="kernel", reward_norm=reward_norm)


@pytest.mark.gpu
def test_population_members_keep_their_own_statistics(g):
    """K = 2 x 64 envs, each member with its own gamma: after two iterations member k's statistics, returns and rewards
    are those of a solo normaliser run on its columns of the raw rewards, bit for bit."""
    K, EM, gam = 2, 64, [0.98, 0.9]
    t = _population(g, K, gammas=gam)
    solo = [g.RewardNormalizer(EM, gamma=gam[k], device=DEV) for k in range(K)]
    for _ in range(2):
        t.collect()
        raw = torch.nan_to_num(t._fused_out["reward"].float(), nan=0.0)
        for k in range(K):
            cols = slice(k * EM, (k + 1) * EM)
            o = solo[k].normalize(raw[:, cols].contiguous(), t.b_done[:, cols].contiguous())
            assert same_bits(o, t.b_rew[:, cols])
        st = t.update()
    torch.cuda.synchronize()
    for k in range(K):
        assert same_bits(solo[k].stats[0], t.reward_norm.stats[k])
        assert same_bits(solo[k].returns, t.reward_norm.returns[k * EM:(k + 1) * EM])
        assert st[k]["reward_std"] == float(solo[k].reward_std()[0])
    assert not same_bits(t.reward_norm.stats[0], t.reward_norm.stats[1])


@pytest.mark.gpu
def test_pbt_recipient_inherits_the_donors_statistics(g):
    """K = 4, fraction 0.25: after exploit() stats[k] == stats[donor[k]] for every k, bit for bit, the returns untouched;
    the score of the exchange is the raw mean episode return."""
    t = _population(g, 4, pbt=g.PBTConfig(ready_every=1, fraction=0.25, seed=77))
    plain = _population(g, 4, pbt=g.PBTConfig(ready_every=1, fraction=0.25, seed=77), reward_norm=None)
    t.collect()
    plain.collect()
    assert same_bits(t.window["score"], plain.window["score"]) and same_bits(t.b_epret, plain.b_epret)
    g.PopulationTrainer.update(t)                         # the parent's update alone: no exploit yet
    torch.cuda.synchronize()
    stats0, returns0 = t.reward_norm.stats.clone(), t.reward_norm.returns.clone()
    assert len({bytes(stats0[k].cpu().numpy().tobytes()) for k in range(4)}) == 4
    recs = t.exploit()
    torch.cuda.synchronize()
    donor = [k if r["exploit"] is None else r["exploit"] for k, r in enumerate(recs)]
    assert sum(d != k for k, d in enumerate(donor)) == 1
    for k in range(4):
        assert same_bits(t.reward_norm.stats[k], stats0[donor[k]]), k
    assert same_bits(t.reward_norm.returns, returns0)
    t.collect()                                           # the next iteration runs on the inherited scale
    st = t.update()
    assert all(np.isfinite(s["reward_std"]) and np.isfinite(s["value_loss"]) for s in st)


@pytest.mark.gpu
def test_checkpoints_carry_the_normaliser_state(g, tmp_path):
    """learn() over two iterations with a checkpoint after each: the state saved after the first, loaded into a fresh
    normaliser, turns the second iteration's raw rewards into the trainer's b_rew and ends in the trainer's state, bit for
    bit -- which is the second checkpoint.  The zips are written as before."""
    tr = _solo(g)
    T, E = 16, 128
    tr.learn(2 * T * E, log=None, save_dir=str(tmp_path), checkpoint_every=T * E, eval_every=T * E, eval_episodes=4)
    torch.cuda.synchronize()
    ck = os.path.join(str(tmp_path), "checkpoints")
    assert sorted(os.listdir(ck)) == sorted(["model_%d_steps.zip" % n for n in (T * E, 2 * T * E)] +
                                            ["reward_norm_%d_steps.pt" % n for n in (T * E, 2 * T * E)])
    assert os.path.exists(os.path.join(str(tmp_path), "best_model.zip"))
    assert os.path.exists(os.path.join(str(tmp_path), "best_model_reward_norm.pt"))
    first, second = (torch.load(os.path.join(ck, "reward_norm_%d_steps.pt" % n)) for n in (T * E, 2 * T * E))
    assert abs(first["stats"][0, 2].item() - T * E) < 1e-3 and abs(second["stats"][0, 2].item() - 2 * T * E) < 1e-3
    fresh = g.RewardNormalizer(E, device=DEV)
    fresh.load_state_dict(first)
    out = fresh.normalize(torch.nan_to_num(tr._fused_out["reward"].float(), nan=0.0), tr.b_done)
    torch.cuda.synchronize()
    assert same_bits(out, tr.b_rew)
    now = fresh.state_dict()
    for name in ("returns", "stats", "gamma"):
        assert same_bits(now[name], second[name]) and same_bits(now[name], getattr(tr.reward_norm, name)), name
    assert (now["epsilon"], now["clip_reward"], now["n_envs"], now["n_members"]) == (1e-8, 10.0, E, 1)
    with pytest.raises(ValueError, match="load_state_dict"):
        g.RewardNormalizer(64, device=DEV).load_state_dict(first)
