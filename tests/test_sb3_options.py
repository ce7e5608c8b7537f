"""SB3's clip_range_vf and its learning-rate / clip-range schedules inside the fused update:
acas2d_ppo_update_sb3_set_f32 (csrc/acas2d_ppo_sb3.hip) and the host code over it (ppo.PPOConfig's four option fields,
ppo.linear_schedule, ppo_loss(old_val=), FusedUpdate / FusedUpdateSet's `options` entry, the three trainers), against the
float64 restatement of tests/sb3_options_ref.py.

  CPU  the two symbols and the struct's size; every rejection before a HIP call, naming its field; ppo_loss with
       clip_range_vf against NumPy and its closed-form gradient, rows exactly at +-c included; the config rules; the
       op-by-op update under a schedule; the register guard of the new unit.
  GPU  neutral options == the guarded entry bit for bit; value clipping against float64; the factors; the stop with options
       on; the footprint of the three new pointers; the three trainers.
The bounds are the project's own (tests/test_kl_guard.py): TAU, TAU0, TAU_M, TAU_V per tensor, stats[5] and diag[2] within
1e-5 max(1, ref).  Every criterion prints what it observed.

Observed (MI355X), worst fractions of the bounds over the value-clipping, factor and stop cases: stats[5] 0.019, stats[4]
0.565 (D = 101, K = 1, B = 2, the unclipped second call), the gradient norm 0.061, diag[2] 0.004 with every clipped count
exact; m 0.027 of TAU_M, v 0.265 of TAU_V (D = 8, K = 1, B = 130), the parameters below TAU0 per tensor, the parameter
excess 7.4e-4 lr of the 1e-2 lr allowed (D = 101, K = 1, B = 65).  The neutral, footprint (B = 64) and stopped-member
identities held bit for bit.  The 146 GPU tests of this file take 12.9 s.  DESIGN.md 4.2j has the same figures."""
import ctypes as C
import dataclasses
import os
import re
import types

import numpy as np
import pytest

import helpers as H
import kl_guard_ref as KR
import learner_ref as R
import learner_support as LS
import sb3_options_ref as S

torch = pytest.importorskip("torch")
DEV = "cuda:0"
NARROW, WIDE = (8, 11, 14, 17, 29), (53, 101, 197)
WIDTHS = NARROW + WIDE
ENTRY, GUARDED = "acas2d_ppo_update_sb3_set_f32", "acas2d_ppo_update_guarded_set_f32"
B1, B2, EPS = 0.9, 0.999, 1e-5


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
def test_sb3_entry_is_exported_and_declared(g):
    L = g.native.lib()
    for name in (ENTRY, "acas2d_ppo_options_size"):
        assert name in g.native.EXPORTS and getattr(L, name)
    assert C.sizeof(g.native.CPpoOptions) == L.acas2d_ppo_options_size() == 3 * 8
    assert [n for n, _ in g.native.CPpoOptions._fields_] == ["old_val", "clip_range_vf", "scale"]
    header = re.sub(r"\s+", " ", open(os.path.join(H.ROOT, "include", "acas2d.h")).read())
    assert ("int %s(const Acas2dPpoUpdateSet *u, const Acas2dPpoGuard *g, const Acas2dPpoOptions *o, void *stream);"
            % ENTRY) in header
    assert "size_t acas2d_ppo_options_size(void);" in header
    assert L.acas2d_abi_version() == g.native.ABI_VERSION == 7
    print("CPpoOptions: %d bytes" % C.sizeof(g.native.CPpoOptions))


def test_sb3_update_validation_needs_no_gpu(g):
    """acas2d_ppo_update_sb3_set_f32 rejects everything the guarded entry rejects, a NULL `o` and a NULL pointer in `o`
    with ACAS2D_EINVAL before any HIP call (the pointers are host addresses: a launch would fail otherwise); the message
    names the field."""
    L = g.native.lib()
    buf = (C.c_double * 64)()
    a = C.addressof(buf)
    names = [n for n, _ in g.native.CPpoUpdateSet._fields_]
    ints = dict(n_members=3, n_rows=64, obs_dim=8, apply=1)

    def call(guard=(a, a, a), opts=(a, a, a), **kw):
        return L.acas2d_ppo_update_sb3_set_f32(*LS.host_update_set_args(g, a, guard=guard, opts=opts, **{**ints, **kw}))

    def rejects(msg, **kw):
        assert call(**kw) == -22, kw
        err = L.acas2d_last_error()
        print("  %-40s %s" % (kw, err.decode()[:120]))
        assert msg.encode() in err and b"acas2d_ppo_update_sb3_set" in err, (kw, err)

    for n in names:
        if n not in ints:
            rejects("every pointer is required", **{n: None})
    for B in (1, 0, -5):
        rejects("n_rows = %d" % B, n_rows=B)
    assert L.acas2d_ppo_update_sb3_set_f32(None, None, None, None) == -22 and b"NULL argument" in L.acas2d_last_error()
    rejects("target_kl, stopped, diag", guard=None)
    for hole in range(3):
        rejects("target_kl, stopped, diag", guard=tuple(None if i == hole else a for i in range(3)))
    rejects("NULL `o`", opts=None)
    for hole, field in enumerate(("old_val", "clip_range_vf", "scale")):
        rejects("field %s is NULL" % field, opts=tuple(None if i == hole else a for i in range(3)))
    for K in (0, -1, 65536):
        rejects("n_members = %d" % K, n_members=K)
    for D in (0, 7, 9, 30, 52, 54, 100, 198):
        rejects("obs_dim = %d" % D, obs_dim=D)
        assert b"8, 11, 14, 17, 29, 53, 101, 197" in L.acas2d_last_error()
    for D in WIDTHS:
        rejects("apply = 0", obs_dim=D, apply=0)


def _fake_policy(mean, value, log_std):
    return types.SimpleNamespace(forward=lambda obs: (mean, value), log_std=log_std)


def test_ppo_loss_clip_range_vf_against_numpy_and_its_closed_form_gradient(g):
    rng = np.random.default_rng(11)
    n, c, vf_coef = 97, 0.5, 0.71
    t = lambda x: torch.as_tensor(np.asarray(x, np.float64))  # noqa: E731
    old_val = np.round(rng.normal(1.0, 2.0, n) * 64) / 64      # dyadic: old +- c is exact
    value = old_val + rng.normal(0, 0.6, n)
    value[:4] = old_val[:4] + np.array([c, -c, c, -c])         # rows exactly AT the edges: the gradient passes
    value[4:6] = old_val[4:6] + np.array([c + 1e-9, -c - 1e-9])                        # just outside: it does not
    ret = rng.normal(2, 3, n)
    d = value - old_val
    assert (d[:4] == [c, -c, c, -c]).all() and (np.abs(d[4:6]) > c).all()
    assert (np.abs(d) > c).sum() > 10 and (np.abs(d) < c).sum() > 10
    mean, act = t(rng.normal(0, 1, (n, 1))), t(rng.normal(0, 1, (n, 1)))
    old_logp, adv = t(rng.normal(-1, 0.3, n)), t(rng.normal(0, 2, n))
    ls = torch.zeros(1, dtype=torch.float64, requires_grad=True)
    v = t(value).requires_grad_(True)
    cfg = g.PPOConfig(clip_range_vf=c, vf_coef=vf_coef, ent_coef=0.01)
    loss, pg, vf = g.ppo.ppo_loss(_fake_policy(mean, v, ls), cfg, None, act, old_logp, adv, t(ret), t(old_val))
    vf64, _ = S.value_loss64(value, old_val, ret, c)
    plain64, _ = S.value_loss64(value, old_val, ret, None)
    ent = -(0.5 + S.LOG_SQRT_2PI)
    logp = (-((act - mean) ** 2) / 2.0 - S.LOG_SQRT_2PI).numpy()[:, 0]                  # log_std = 0
    an = adv.numpy()
    an = (an - an.mean()) / (an.std(ddof=1) + 1e-8)
    ratio = np.exp(logp - old_logp.numpy())
    pg64 = -np.mean(np.minimum(an * ratio, an * np.clip(ratio, 1 - cfg.clip_range, 1 + cfg.clip_range)))
    loss64 = pg64 + 0.01 * ent + vf_coef * vf64
    print("value loss %.15g vs NumPy %.15g (unclipped %.15g), loss %.15g vs %.15g" % (float(vf.detach()), vf64, plain64, float(loss.detach()), loss64))
    assert abs(float(vf.detach()) - vf64) <= 1e-12 * abs(vf64) and abs(float(loss.detach()) - loss64) <= 1e-12 * abs(loss64)
    assert abs(vf64 - plain64) > 1e-3                          # (the clipping does something on this minibatch)
    loss.backward()
    want = S.dvalue64(value, old_val, ret, c, vf_coef)
    got = v.grad.numpy()
    print("d loss / d value: max |autograd - closed form| %.3e; at the edges %s, just outside %s" % (np.abs(got - want).max(), got[:4], got[4:6]))
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert (got[:4] != 0).all() and (got[4:6] == 0).all() and (got[np.abs(d) > c] == 0).all()
    with pytest.raises(ValueError, match="old_val"):
        g.ppo.ppo_loss(_fake_policy(mean, v, ls), cfg, None, act, old_logp, adv, t(ret))
    # clip_range_vf = None: the expression it always was, bit for bit, whether or not old_val is given
    plain = g.PPOConfig(vf_coef=vf_coef, ent_coef=0.01)
    a = g.ppo.ppo_loss(_fake_policy(mean, v, ls), plain, None, act, old_logp, adv, t(ret))
    b = g.ppo.ppo_loss(_fake_policy(mean, v, ls), plain, None, act, old_logp, adv, t(ret), old_val=t(old_val))
    want_vf = torch.nn.functional.mse_loss(v, t(ret))
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and torch.equal(a[2], want_vf)
    assert abs(float(a[2]) - plain64) <= 1e-12 * plain64


def test_option_config_rules(g):
    P = g.PPOConfig
    for bad in (0.0, -0.3, float("nan")):
        with pytest.raises(ValueError, match="clip_range_vf"):
            P(clip_range_vf=bad)
    c = P(clip_range_vf=0.3, learning_rate_schedule=g.ppo.linear_schedule())
    assert c.clip_range_vf == 0.3 and c.clip_range_schedule is None and c.clip_range_vf_schedule is None
    r = dataclasses.replace(c, seed=5)
    assert r.clip_range_vf == 0.3 and r.learning_rate_schedule is c.learning_rate_schedule and r.seed == 5
    # the four are attributes, not dataclass fields (tests/test_ppo_host.py's rule on fields stays): pinned here, so that
    # nobody relies on ==, asdict() or repr() to compare or serialise them
    assert g.ppo.OPTION_FIELDS == ("clip_range_vf",) + g.ppo.SCHEDULE_FIELDS
    assert not set(g.ppo.OPTION_FIELDS) & {f.name for f in dataclasses.fields(c)} and not set(g.ppo.OPTION_FIELDS) & set(dataclasses.asdict(c))
    assert c == P() and "clip_range_vf" not in repr(c)
    dropped = P(**dataclasses.asdict(c))
    assert all(getattr(dropped, n) is None for n in g.ppo.OPTION_FIELDS)
    assert all(getattr(r, n) == getattr(c, n) for n in g.ppo.OPTION_FIELDS)          # replace() does carry them
    d = P()
    assert (d.clip_range_vf, d.learning_rate_schedule, d.clip_range_schedule, d.clip_range_vf_schedule) == (None,) * 4
    s = P.sb3()
    assert (s.clip_range_vf, s.learning_rate_schedule, s.clip_range_schedule, s.clip_range_vf_schedule) == (None,) * 4
    assert P.sb3(clip_range_vf=0.2).clip_range_vf == 0.2
    assert not g.ppo.has_options(d) and g.ppo.has_options(c) and g.ppo.has_options(P(clip_range_schedule=lambda p: 1.0))
    # linear_schedule: the end points and `final`
    f0, f1 = g.ppo.linear_schedule(), g.ppo.linear_schedule(0.1)
    assert (f0(1.0), f0(0.0), f0(0.25)) == (1.0, 0.0, 0.25)
    assert f1(1.0) == 1.0 and f1(0.0) == 0.1 and abs(f1(0.5) - 0.55) <= 1e-15
    assert g.ppo.schedule_factors(c, 0.25) == [0.25, 1.0, 1.0] and g.ppo.schedule_factors(d, 0.3) == [1.0, 1.0, 1.0]
    # a factor that is negative or not finite raises where it is evaluated
    for name in g.ppo.SCHEDULE_FIELDS:
        for bad in (-0.1, float("nan"), float("inf")):
            cfg = P(**{name: lambda p, bad=bad: bad})          # (construction does not evaluate)
            with pytest.raises(ValueError, match=name):
                g.ppo.schedule_factors(cfg, 0.5)
            with pytest.raises(ValueError, match=name):
                g.ppo.effective_config(cfg, 0.5)
    e = g.ppo.effective_config(P(clip_range_vf=0.4, learning_rate_schedule=f0, clip_range_schedule=f1, clip_range_vf_schedule=f0), 0.5)
    assert (e.learning_rate, e.clip_range, e.clip_range_vf) == (1.5e-4, 0.2 * f1(0.5), 0.2) and not g.ppo.has_options(dataclasses.replace(e, clip_range_vf=None))
    # member fields outside the hyper row, like target_kl
    for name in ("clip_range_vf",) + g.ppo.SCHEDULE_FIELDS:
        assert name in g.ppo.MEMBER_FIELDS and name not in g.ppo.HYPER_SLOTS
    assert len(g.ppo.HYPER_SLOTS) == 8
    # the captured torch-op updater raises, as it does for target_kl; the fused one and the op-by-op one take them
    venv = types.SimpleNamespace(dtype=torch.float32, n_traffic=1, obs_dim=8, num_envs=3 * 64, device="cpu")
    for cfg in (P(clip_range_vf=0.3), P(learning_rate_schedule=f0), P(clip_range_schedule=f0), P(clip_range_vf_schedule=f0)):
        for kw in (dict(use_graphs=True), dict(use_graphs=True, updater="graphs", collector="graphs")):
            with pytest.raises(ValueError, match="updater='fused'"):
                g.PPOTrainer(venv, cfg, **kw)
        with pytest.raises(AttributeError, match="reset"):     # accepted: construction gets as far as the env (a stub)
            g.PPOTrainer(venv, cfg, use_graphs=True, collector="fused", updater="fused")
        with pytest.raises(AttributeError, match="reset"):
            g.PPOTrainer(venv, cfg, use_graphs=False)
    cfgs = [P(seed=13, clip_range_vf=v, learning_rate_schedule=s_) for v, s_ in ((None, None), (0.3, None), (None, f0))]
    with pytest.raises(AttributeError, match="reset"):
        g.PopulationTrainer(venv, cfgs)
    with pytest.raises(AttributeError, match="reset"):
        g.PBTTrainer(venv, cfgs, g.PBTConfig(ready_every=2, fraction=0.0))


def _eager_trainer(g, n=256, D=8, **cfg_kw):
    rng = np.random.default_rng(3)
    venv = types.SimpleNamespace(dtype=torch.float32, n_traffic=1, obs_dim=D, num_envs=64, device="cpu",
                                 reset=lambda: torch.zeros(64, D))
    obs = torch.as_tensor(rng.uniform(-1, 1, (n, D)), dtype=torch.float32)
    act = torch.as_tensor(rng.normal(0, 0.7, (n, 1)), dtype=torch.float32)
    adv, ret = (torch.as_tensor(rng.normal(m, 2, n), dtype=torch.float32) for m in (0, 2))
    val = torch.as_tensor(rng.normal(0.5, 1, n), dtype=torch.float32)
    tr = g.PPOTrainer(venv, g.PPOConfig(seed=7, batch_size=64, n_epochs=3, **cfg_kw), use_graphs=False)
    with torch.no_grad():
        mean, _ = tr.policy.forward(obs)
        old = g.ppo._normal_logp(mean, tr.policy.log_std, act)
    return tr, (obs, act, old, adv, ret, val)


def test_eager_update_honours_the_schedules_and_clip_range_vf(g):
    """The op-by-op PPOTrainer.update(): a learning-rate factor of 0 leaves every parameter bit for bit while Adam's step
    count and moments advance; linear_schedule() at progress 0.25 sets the optimizer's lr to 0.25 x learning_rate and the
    effective clip range; clip_range_vf changes the critic's step and needs old_val."""
    tr, batch = _eager_trainer(g, learning_rate_schedule=lambda p: 0.0)
    before = R.flat_params(tr.policy)
    torch.manual_seed(11)
    st = tr.update(*batch)
    steps = {int(s["step"]) for s in tr.opt.state_dict()["state"].values()}
    moments = max(float(s["exp_avg"].abs().max()) for s in tr.opt.state_dict()["state"].values())
    print("factor 0:", st, "optimizer steps", steps, "max |exp_avg| %.3e" % moments)
    assert np.array_equal(R.flat_params(tr.policy), before) and steps == {12} and moments > 0
    assert st["learning_rate"] == 0.0 and st["clip_range"] == 0.2 and "clip_range_vf" not in st

    lin = g.ppo.linear_schedule()
    tr, batch = _eager_trainer(g, learning_rate_schedule=lin, clip_range_schedule=g.ppo.linear_schedule(0.5))
    tr.total_timesteps, tr.num_timesteps = 1000, 750          # as inside learn(): progress_remaining 0.25
    torch.manual_seed(11)
    st = tr.update(*batch)
    lrs = {grp["lr"] for grp in tr.opt.param_groups}
    print("progress 0.25:", st, "optimizer lr", lrs)
    assert lrs == {0.25 * tr.cfg.learning_rate} and st["learning_rate"] == 0.25 * 3e-4 and st["clip_range"] == 0.2 * 0.625
    tr.total_timesteps = None                                 # outside learn(): 1.0
    tr.update(*batch)
    assert {grp["lr"] for grp in tr.opt.param_groups} == {tr.cfg.learning_rate}
    tr.total_timesteps, tr.num_timesteps = 1000, 1300         # an overshooting last iteration: clamped at 0
    assert tr._progress_remaining() == 0.0

    out = {}
    for name, kw in (("plain", {}), ("clipped", dict(clip_range_vf=0.05))):
        tr, batch = _eager_trainer(g, **kw)
        torch.manual_seed(11)
        st = tr.update(*batch)
        out[name] = (st, R.flat_params(tr.policy))
    segs = R.segments(tr.policy)
    a, b = out["plain"][1], out["clipped"][1]
    critic_moved = max(float(np.abs(a[s:e] - b[s:e]).max()) for n, s, e in segs if "value_net" in n)
    print("clip_range_vf=0.05:", out["clipped"][0], "critic differs from the plain run by %.3e" % critic_moved)
    assert out["clipped"][0]["clip_range_vf"] == 0.05 and "clip_range_vf" not in out["plain"][0] and critic_moved > 0
    with pytest.raises(ValueError, match="old_val"):
        tr.update(*batch[:5])


@H.needs_hipcc
def test_sb3_update_kernels_stay_in_registers_and_lds(g, tmp_path):
    """csrc/acas2d_ppo_sb3.hip: five narrow gradient kernels, three wide ones and the apply kernel, held to what
    test_guarded_update_kernels_stay_in_registers_and_lds holds the guarded unit to: no spill of either register file, no
    scratch, at most 256 VGPRs, 64 / 256 / 1 024 threads, the wide kernels' dynamic plus static LDS within 160 KB.
    Observed: narrow 144 VGPRs / 87 SGPRs (90 at D = 29); wide 94 / 96 / 98 VGPRs, 104 / 104 / 105 SGPRs; apply 30 / 46."""
    _, kernels = H.kernel_metadata(tmp_path, "acas2d_ppo_sb3.hip")
    assert len(kernels) == 9
    L = g.native.lib()
    seen = {"narrow": [], "wide": [], "apply": 0}
    for k in kernels:
        name = k.name
        print(name[:70], "vgpr", k.field("vgpr_count"), "sgpr", k.field("sgpr_count"), "static LDS",
              k.field("group_segment_fixed_size"))
        assert k.field("vgpr_spill_count") == 0 and k.field("sgpr_spill_count") == 0, name
        assert k.field("private_segment_fixed_size") == 0 and k.field("vgpr_count") <= 256, name
        if "ppo_apply_sb3_set_kernel" in name:
            seen["apply"] += 1
            assert k.field("max_flat_workgroup_size") == 1024, name
            continue
        D = int(re.search(r"kernelILi(\d+)E", name).group(1))
        if "ppo_grad_wide_sb3_set_kernel" in name:
            seen["wide"].append(D)
            assert k.field("max_flat_workgroup_size") == 256, name
            lds = L.acas2d_ppo_wide_lds_bytes(D)
            assert lds + k.field("group_segment_fixed_size") <= 160 * 1024, (D, lds)
        else:
            assert "ppo_grad_sb3_set_kernel" in name
            seen["narrow"].append(D)
            assert k.field("max_flat_workgroup_size") == 64, name
    assert sorted(seen["narrow"]) == list(NARROW) and sorted(seen["wide"]) == list(WIDE) and seen["apply"] == 1


# ---- GPU: the kernels -------------------------------------------------------------------------------------------------
CLIP_VF = (0.3, None, 1.0)             # members 0 and 2 clip, member 1 is off, in the same launch
_ONE = lambda p: 1.0  # noqa: E731     (a schedule that turns the options entry on and changes nothing)


WORST = {}


def _note(key, frac):
    WORST[key] = max(WORST.get(key, 0.0), frac)


def _pre_state(fu):
    return fu.m.double().cpu().numpy(), fu.v.double().cpu().numpy(), fu.step_count.cpu().tolist()


def _check_member(g, what, bt, pset, fu, k, cfg, idx_k, theta0, pre, old_val, clip_range, clip_vf, lr, segs):
    """Member k after ONE call against float64 from the kernel's own pre-step state: the gradient norm, the two logged
    losses (1e-5 max(1, ref)), m and v per tensor (TAU_M, TAU_V), the parameters per tensor (TAU) and within 1e-2 lr of
    the float64 step beyond one float32 ulp (tests/test_kl_guard.py's rule)."""
    m0, v0, s0 = pre
    obs, act, old, adv, ret = bt.host(idx_k)
    ov = old_val.double().cpu().numpy()[idx_k.cpu().numpy()]
    grad, pg, vf, _, _ = S.grad64(g.ActorCritic, cfg, bt.D, theta0, obs, act, old, adv, ret, ov, clip_range, clip_vf)
    theta_ref, m_ref, v_ref, norm = R.adam64(theta0, grad, m0[k], v0[k], s0[k], cfg.max_grad_norm, lr, B1, B2, EPS)
    stats = fu.stats.double().cpu().numpy()
    for key, got_, ref_, tol in (("norm", stats[k, 2], norm, 1e-5 * norm), ("pg", stats[k, 4], pg, 1e-5 * max(1.0, abs(pg))),
                                 ("vf", stats[k, 5], vf, 1e-5 * max(1.0, vf))):
        print("  %s %s: %.8g vs %.8g (%.3f of the bound)" % (what, key, got_, ref_, abs(got_ - ref_) / tol))
        assert abs(got_ - ref_) <= tol, (what, key, got_, ref_)
        _note("stats " + key, abs(got_ - ref_) / tol)
    assert fu.step_count[k].item() == s0[k] + 1 and float(fu.grad[k].abs().max()) == 0.0, what
    _note("m", LS.assert_per_tensor("m " + what, fu.m[k].double().cpu().numpy(), m_ref, segs, LS.TAU_M) / LS.TAU_M)
    _note("v", LS.assert_per_tensor("v " + what, fu.v[k].double().cpu().numpy(), v_ref, segs, LS.TAU_V) / LS.TAU_V)
    theta1 = LS.theta_of(pset, k)
    _note("theta", LS.assert_per_tensor("theta " + what, theta1, theta_ref, segs, LS.TAU) / LS.TAU)
    if lr > 0:
        ulp = np.spacing(np.abs(theta_ref).astype(np.float32)).astype(np.float64)
        excess = (np.abs(theta1 - theta_ref) - ulp) / lr
        print("  %s: parameter excess %.2e lr (bound 1e-2)" % (what, float(excess.max())))
        assert excess.max() <= 1e-2, (what, float(excess.max()), int(excess.argmax()))
        _note("theta excess", float(excess.max()) / 1e-2)
        # the step was taken wherever float64 takes one (at B = 2 both rows of a network may be clipped: gradient exactly 0)
        moved_ref, moved = np.abs(theta_ref - theta0) / lr > 0.05, np.abs(theta1 - theta0) / lr > 0.025
        assert moved[moved_ref].all() and moved_ref.any(), (what, int(moved_ref.sum()), int(moved.sum()))
    else:
        assert np.array_equal(theta1, theta0), what
    return vf


IDENTITY_CASES = [(D, K, B) for D in WIDTHS for K in (1, 3) for B in (2, 63, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("D,K,B", IDENTITY_CASES, ids=["D%d-K%d-B%d" % c for c in IDENTITY_CASES])
def test_neutral_options_equal_the_guarded_entry_bitwise(gpu, D, K, B):
    """scale rows of ones, clip_range_vf all 0: two calls leave the parameters, adam_m, adam_v, adam_step, stats and diag
    of acas2d_ppo_update_guarded_set_f32 on twin state, bit for bit (x * 1.0f is exact; B <= 64: one workgroup adds each
    gradient entry).  old_val is NaN everywhere: it is not read."""
    g = gpu
    bt = LS.RolloutBatch(g, D, K, K * B + 317, seed=8500 + 7 * D + 31 * K + B)
    plain_cfgs = LS.member_cfgs(g, K)
    opt_cfgs = LS.member_cfgs(g, K, per_member=[dict(learning_rate_schedule=_ONE)] + [{}] * (K - 1))
    twins = {"guarded": bt.policy_set(), "sb3": bt.policy_set()}
    nan = torch.full((bt.n,), float("nan"), dtype=torch.float32, device=DEV)
    fus = {"guarded": g.FusedUpdateSet(twins["guarded"], plain_cfgs, *bt.bufs, diagnostics=True),
           "sb3": g.FusedUpdateSet(twins["sb3"], opt_cfgs, *bt.bufs, old_val=nan)}
    a, b = fus["guarded"], fus["sb3"]
    assert a.guarded and not a.options and b.guarded and b.options
    for fu in fus.values():
        fu.begin_update()
    torch.cuda.synchronize()
    assert torch.equal(b.scale, torch.ones(K, 4, device=DEV)) and float(b.clip_range_vf.abs().max()) == 0.0

    def same(what, x, y):
        assert x.shape == y.shape and H.bits_equal(x, y), (what, D, K, B)

    for call in (1, 2):
        idx = LS.draw(bt, twins["guarded"], [c.clip_range for c in plain_cfgs], B, rows=LS.host_rows)
        for fu in fus.values():
            fu.step(idx)
        torch.cuda.synchronize()
        for n in R.PARAM_NAMES:
            same("call %d %s" % (call, n), twins["guarded"].params[n], twins["sb3"].params[n])
        for what, x, y in (("m", a.m, b.m), ("v", a.v, b.v), ("step_count", a.step_count, b.step_count), ("grad", a.grad, b.grad),
                           ("stats", a.stats, b.stats), ("diag", a.diag, b.diag), ("stopped", a.stopped, b.stopped)):
            same("call %d %s" % (call, what), x, y)
        assert b.step_count.cpu().tolist() == [call] * K and b.diag[:, 7].cpu().tolist() == [float(call)] * K
        assert bool(torch.isfinite(b.stats).all())
    name = R.PARAM_NAMES[8]
    moved = float((twins["sb3"].params[name] - torch.stack([p.get_parameter(name).detach() for p in bt.pols])).abs().max())
    print("D=%d K=%d B=%d: neutral options == guarded bit for bit after two steps (critic moved by %.2e)" % (D, K, B, moved))
    assert moved > 0.0


def _cpu_value32(pset, k, obs_rows):
    """The critic of member k in torch float32 on the CPU."""
    pol = pset.member(k).cpu()
    with torch.no_grad():
        return pol.forward(obs_rows.cpu())[1].numpy()


def _place_old_val(g, bt, pset, k, idx_k, c_eff, old_val, want_sides):
    """old_val on member k's rows: its float64 value plus N(0, 0.8), admitted as the issue sets it (asserted here, on
    float64, before any launch): every row at least 1e-4 off +-c, both clipped sides and the unclipped middle present
    (want_sides), and torch float32 on the CPU on float64's side of +-c for every row."""
    theta = LS.theta_of(pset, k)
    obs_rows = bt.obs[idx_k]
    v64 = S.value64(g.ActorCritic, bt.D, theta, obs_rows.cpu().numpy())
    old = S.place_old_val(bt.rng, v64, c_eff)
    old_val[idx_k] = torch.as_tensor(old.astype(np.float32), device=old_val.device)
    if c_eff is None or not c_eff > 0:
        return
    d64 = v64 - old
    dist = float(np.abs(np.abs(d64) - c_eff).min())
    assert dist >= S.EDGE, (k, dist)
    above, below, inside = int((d64 > c_eff).sum()), int((d64 < -c_eff).sum()), int((np.abs(d64) < c_eff).sum())
    print("  member %d: c = %.8g, %d rows clipped above, %d below, %d unclipped, nearest row %.2e off an edge" % (k, c_eff, above, below, inside, dist))
    if want_sides:
        assert above >= 1 and below >= 1 and inside >= 1, (k, above, below, inside)
    d32 = _cpu_value32(pset, k, obs_rows).astype(np.float64) - old
    assert np.array_equal(d32 > c_eff, d64 > c_eff) and np.array_equal(d32 < -c_eff, d64 < -c_eff), k


CLIP_CASES = [(D, K, B) for D in WIDTHS for K in (1, 3) for B in (2, 63, 64, 65, 130)]


@pytest.mark.gpu
@pytest.mark.parametrize("D,K,B", CLIP_CASES, ids=["D%d-K%d-B%d" % c for c in CLIP_CASES])
def test_value_clipping_vs_float64(gpu, D, K, B):
    """Members with clip_range_vf (0.3, off, 1.0) in one launch, old_val = the member's float64 value + N(0, 0.8).  One
    call: parameters, m, v per tensor and stats[5] at the project's bounds against the float64 restatement with SB3's value
    clipping (the off member against the plain-MSE reference).  A second call with old_val = the critic's own float32
    output: nothing is clipped, and the result matches the plain-MSE float64 reference at the same bounds.  B = 2 and 63
    leave dead lanes, 64 fills one workgroup, 65 and 130 add a second and a third."""
    g = gpu
    bt = LS.RolloutBatch(g, D, K, K * B + 317, seed=12000 + 7 * D + 31 * K + B)
    cfgs = LS.member_cfgs(g, K, per_member=[dict(clip_range_vf=CLIP_VF[k]) for k in range(K)])
    pset = bt.policy_set()
    segs = R.segments(bt.pols[0])
    old_val = torch.full((bt.n,), float("nan"), dtype=torch.float32, device=DEV)
    fu = g.FusedUpdateSet(pset, cfgs, *bt.bufs, old_val=old_val)
    assert fu.options and fu.guarded and fu.clip_range_vf.cpu().tolist() == [np.float32(c or 0.0) for c in CLIP_VF[:K]]
    fu.begin_update()
    c_eff = [None if CLIP_VF[k] is None else S.product32(CLIP_VF[k], 1.0) for k in range(K)]
    # ---- call 1: clipped
    idx = LS.draw(bt, pset, [c.clip_range for c in cfgs], B, rows=LS.host_rows)
    theta0 = [LS.theta_of(pset, k) for k in range(K)]
    for k in range(K):
        _place_old_val(g, bt, pset, k, idx[k], c_eff[k], old_val, want_sides=B >= 63)
    pre = _pre_state(fu)
    fu.step(idx)
    torch.cuda.synchronize()
    assert fu.stopped.cpu().tolist() == [0] * K
    for k in range(K):
        what = "D=%d K=%d B=%d call 1 member %d (c %s)" % (D, K, B, k, c_eff[k])
        vf = _check_member(g, what, bt, pset, fu, k, cfgs[k], idx[k], theta0[k], pre, old_val, cfgs[k].clip_range, c_eff[k],
                           cfgs[k].learning_rate, segs)
        if c_eff[k] is not None and B >= 63:                   # (for the record: what clipping does to the logged loss)
            obs, act, old, adv, ret = bt.host(idx[k])
            plain = R.grad64(g.ActorCritic, dataclasses.replace(cfgs[k], clip_range_vf=None), D, theta0[k], obs, act, old, adv, ret)[2]
            print("  %s: value loss %.8g, the unclipped one would be %.8g" % (what, vf, plain))
    # ---- call 2: old_val = the critic's own float32 output, nothing clipped
    idx = LS.draw(bt, pset, [c.clip_range for c in cfgs], B, rows=LS.host_rows)
    theta0 = [LS.theta_of(pset, k) for k in range(K)]
    for k in range(K):
        with torch.no_grad():
            own = pset.member(k).forward(bt.obs[idx[k]])[1]
        old_val[idx[k]] = own
        v64 = S.value64(g.ActorCritic, D, theta0[k], bt.obs[idx[k]].cpu().numpy())
        assert np.abs(v64 - own.double().cpu().numpy()).max() < 1e-4
    pre = _pre_state(fu)
    fu.step(idx)
    torch.cuda.synchronize()
    for k in range(K):
        what = "D=%d K=%d B=%d call 2 member %d (unclipped)" % (D, K, B, k)
        _check_member(g, what, bt, pset, fu, k, cfgs[k], idx[k], theta0[k], pre, old_val, cfgs[k].clip_range, None,
                      cfgs[k].learning_rate, segs)
    print("D=%d K=%d B=%d: worst fractions of the bounds so far %s" % (D, K, B, {k: round(v, 3) for k, v in WORST.items()}))


FACTOR_CASES = [(D, B) for D in (8, 29, 53, 197) for B in (63, 130)]
FACTORS = ((0.5, 0.5, 2.0), (1.0, 0.25, 1.0), (0.0, 1.0, 1.0))      # on learning_rate, clip_range, clip_range_vf


def _const(x):
    return lambda p: x


def _factor_cfgs(g):
    return LS.member_cfgs(g, 3, per_member=[dict(clip_range_vf=CLIP_VF[k], learning_rate_schedule=_const(FACTORS[k][0]),
                                        clip_range_schedule=_const(FACTORS[k][1]),
                                        clip_range_vf_schedule=_const(FACTORS[k][2])) for k in range(3)])


def _effective(cfg, factors):
    """(learning rate, clip range, value clip or None) as the kernels form them: float32(hyper) * float32(scale)."""
    return (S.product32(cfg.learning_rate, factors[0]), S.product32(cfg.clip_range, factors[1]),
            None if cfg.clip_range_vf is None else S.product32(cfg.clip_range_vf, factors[2]))


@pytest.mark.gpu
@pytest.mark.parametrize("D,B", FACTOR_CASES, ids=["D%d-B%d" % c for c in FACTOR_CASES])
def test_factors_scale_the_rate_and_both_clips(gpu, D, B):
    """scale rows (0.5, 0.5, 2.0), (1, 0.25, 1), (0, 1, 1), written by begin_update() from the members' schedules.  The
    references use float32(hyper) * float32(scale), then float64: diag[3] is the float64 count at the EFFECTIVE clip range
    exactly, the applied step float64 Adam at the effective rate, the value clip the effective one.  The member with rate
    factor 0 keeps every parameter bit while adam_m, adam_v, adam_step and diag[7] advance."""
    g = gpu
    K = 3
    bt = LS.RolloutBatch(g, D, K, K * B + 317, seed=13000 + 7 * D + B)
    cfgs = _factor_cfgs(g)
    pset = bt.policy_set()
    segs = R.segments(bt.pols[0])
    old_val = torch.full((bt.n,), float("nan"), dtype=torch.float32, device=DEV)
    fu = g.FusedUpdateSet(pset, cfgs, *bt.bufs, old_val=old_val)
    fu.begin_update(0.5)
    torch.cuda.synchronize()
    want = torch.tensor([list(f) + [1.0] for f in FACTORS], dtype=torch.float32)
    assert torch.equal(fu.scale.cpu(), want) and fu.factors == [list(f) for f in FACTORS]
    eff = [_effective(cfgs[k], FACTORS[k]) for k in range(K)]
    assert [e["learning_rate"] for e in fu.effective()] == [cfgs[k].learning_rate * FACTORS[k][0] for k in range(K)]
    idx = LS.draw(bt, pset, [e[1] for e in eff], B, rows=LS.host_rows)
    theta0 = [LS.theta_of(pset, k) for k in range(K)]
    params0 = [[p[k].clone() for p in fu._params] for k in range(K)]
    for k in range(K):
        _place_old_val(g, bt, pset, k, idx[k], eff[k][2], old_val, want_sides=True)
    pre = _pre_state(fu)
    fu.step(idx)
    torch.cuda.synchronize()
    diag = fu.diag.cpu().numpy()
    for k in range(K):
        lr, clip, c_vf = eff[k]
        what = "D=%d B=%d member %d (lr %.4g, clip %.4g, value clip %s)" % (D, B, k, lr, clip, c_vf)
        log_ratio = bt.log_ratio(theta0[k], idx[k])
        assert KR.edge_distance(log_ratio, clip) >= 1e-4, (what, KR.edge_distance(log_ratio, clip))
        count, _ = KR.clip_fraction64(log_ratio, clip)
        count_cfg, _ = KR.clip_fraction64(log_ratio, cfgs[k].clip_range)
        kl64 = KR.approx_kl64(log_ratio)
        print("  %s: clipped %d of %d at the effective range (%d at the config's) -> diag[3] %.8g; approx_kl %.8g vs %.8g"
              % (what, count, B, count_cfg, diag[k, 3], diag[k, 2], kl64))
        assert diag[k, 3] == np.float32(count) / np.float32(B), (what, diag[k, 3], count)
        if FACTORS[k][1] != 1.0:
            assert count != count_cfg, what                    # (the factor is visible in the count)
        assert abs(float(diag[k, 2]) - kl64) <= 1e-5 * max(1.0, kl64), what
        _note("diag[2]", abs(float(diag[k, 2]) - kl64) / (1e-5 * max(1.0, kl64)))
        assert diag[k, 6] == 1.0 and diag[k, 7] == 1.0
        _check_member(g, what, bt, pset, fu, k, cfgs[k], idx[k], theta0[k], pre, old_val, clip, c_vf, lr, segs)
    k = 2                                                      # rate factor 0: nothing moves, Adam's state does
    assert eff[k][0] == 0.0
    for name, p, q in zip(R.PARAM_NAMES, fu._params, params0[k]):
        assert H.bits_equal(p[k], q), name
    assert float(fu.m[k].abs().max()) > 0 and float(fu.v[k].abs().max()) > 0 and fu.step_count[k].item() == 1
    print("D=%d B=%d: worst fractions of the bounds so far %s" % (D, B, {k: round(v, 3) for k, v in WORST.items()}))


@pytest.mark.gpu
@pytest.mark.parametrize("D", (8, 197))
def test_stop_with_options_on(gpu, D):
    """K = 3, three calls of one update with value clipping and factors on.  Member 0 has a target_kl that its first
    minibatch (ratio ~ 1) stays under and its second exceeds: it stops there, and its rows are bit for bit where they were,
    on the third call -- with different factors -- too.  Members 1 and 2 apply every call at the float64 bounds."""
    g = gpu
    K, B = 3, 65
    bt = LS.RolloutBatch(g, D, K, K * B + 317, seed=14000 + D)
    cfgs = _factor_cfgs(g)
    cfgs[0] = dataclasses.replace(cfgs[0], target_kl=1e-3)
    pset = bt.policy_set()
    segs = R.segments(bt.pols[0])
    old_val = torch.full((bt.n,), float("nan"), dtype=torch.float32, device=DEV)
    fu = g.FusedUpdateSet(pset, cfgs, *bt.bufs, old_val=old_val)
    fu.begin_update()
    factors = [list(f) for f in FACTORS]
    factors[2][0] = 1.0                                        # (member 2 steps too)
    frozen = None
    for call in (1, 2, 3):
        if call == 3:
            factors = [[0.7, 0.8, 0.5], [0.3, 1.0, 1.0], [2.0, 0.5, 0.25]]
        fu.scale.copy_(torch.tensor([f + [1.0] for f in factors], dtype=torch.float32))
        eff = [_effective(cfgs[k], factors[k]) for k in range(K)]
        idx = LS.host_rows(bt, K, B)
        for k in range(K):
            bt.set_old_logp(LS.theta_of(pset, k), idx[k], "first" if (k == 0 and call == 1) else "mixed", eff[k][1])
        theta0 = [LS.theta_of(pset, k) for k in range(K)]
        kl64 = [KR.approx_kl64(bt.log_ratio(theta0[k], idx[k])) for k in range(K)]
        if call == 1:
            assert not KR.stops(kl64[0], 1e-3) and kl64[0] < 1e-5
        if call == 2:
            assert KR.stops(kl64[0], 1e-3) and kl64[0] > 1e-2
            frozen = dict(theta=theta0[0], m=fu.m[0].clone(), v=fu.v[0].clone(), params=[p[0].clone() for p in fu._params])
        for k in range(K):
            _place_old_val(g, bt, pset, k, idx[k], eff[k][2], old_val, want_sides=False)
        pre = _pre_state(fu)
        fu.step(idx)
        torch.cuda.synchronize()
        stopped, diag = fu.stopped.cpu().tolist(), fu.diag.cpu().numpy()
        print("D=%d call %d: approx_kl64 %s, stopped %s, diag[:, 6] %s, diag[:, 7] %s, adam_step %s"
              % (D, call, ["%.4g" % x for x in kl64], stopped, diag[:, 6], diag[:, 7], fu.step_count.cpu().tolist()))
        assert stopped == ([0, 0, 0] if call == 1 else [1, 0, 0])
        for k in range(K):
            if k == 0 and call >= 2:
                continue
            what = "D=%d call %d member %d" % (D, call, k)
            assert diag[k, 6] == call and diag[k, 7] == call
            _check_member(g, what, bt, pset, fu, k, cfgs[k], idx[k], theta0[k], pre, old_val, eff[k][1], eff[k][2], eff[k][0], segs)
        if call >= 2:
            for name, p, q in zip(R.PARAM_NAMES, fu._params, frozen["params"]):
                assert H.bits_equal(p[0], q), (call, name)
            assert H.bits_equal(fu.m[0], frozen["m"]) and H.bits_equal(fu.v[0], frozen["v"]), call
            assert fu.step_count[0].item() == 1 and float(fu.grad[0].abs().max()) == 0.0
            assert diag[0, 6] == 2.0 and diag[0, 7] == 1.0
    d = fu.diagnostics()
    assert [x["early_stop"] for x in d] == [True, False, False] and [x["n_applied"] for x in d] == [1, 3, 3]
    print("D=%d: worst fractions of the bounds so far %s" % (D, {k: round(v, 3) for k, v in WORST.items()}))


FOOT_CASES = [(D, B) for D in (8, 53) for B in (64, 65)]


@pytest.mark.gpu
@pytest.mark.parametrize("D,B", FOOT_CASES, ids=["D%d-B%d" % c for c in FOOT_CASES])
def test_footprint_of_the_option_pointers(gpu, D, B):
    """old_val holds NaN on every row outside the clipping members' minibatches and on ALL of the off member's rows;
    sentinels surround clip_range_vf, scale and old_val.  The results are finite, at B <= 64 bit-equal to the run on a
    clean buffer (at 65 equal to the atomics' rounding), and the sentinels are intact."""
    g = gpu
    K, PAD, SENT = 3, 64, -12345.5
    bt = LS.RolloutBatch(g, D, K, K * B + 317, seed=15000 + 7 * D + B)
    cfgs = _factor_cfgs(g)
    eff = [_effective(cfgs[k], FACTORS[k]) for k in range(K)]
    idx = LS.draw(bt, bt.policy_set(), [e[1] for e in eff], B, rows=LS.host_rows)
    clean = torch.zeros(bt.n, dtype=torch.float32, device=DEV)
    for k in (0, 2):
        _place_old_val(g, bt, bt.policy_set(), k, idx[k], eff[k][2], clean, want_sides=False)
    results = {}
    for name in ("clean", "hostile"):
        pset = bt.policy_set()
        big_old = torch.full((bt.n + 2 * PAD,), SENT, dtype=torch.float32, device=DEV)
        old_val = big_old[PAD:PAD + bt.n]
        old_val.copy_(clean)
        if name == "hostile":
            keep = torch.zeros(bt.n, dtype=torch.bool, device=DEV)
            keep[idx[0]] = True
            keep[idx[2]] = True
            old_val[~keep] = float("nan")
            assert int(torch.isnan(old_val).sum()) == bt.n - 2 * B and bool(torch.isnan(old_val[idx[1]]).all())
        fu = g.FusedUpdateSet(pset, cfgs, *bt.bufs, old_val=old_val)
        big_vf = torch.full((K + 2 * PAD,), SENT, dtype=torch.float32, device=DEV)
        big_sc = torch.full((K * 4 + 2 * PAD,), SENT, dtype=torch.float32, device=DEV)
        big_vf[PAD:PAD + K] = fu.clip_range_vf
        fu.clip_range_vf, fu.scale = big_vf[PAD:PAD + K], big_sc[PAD:PAD + 4 * K].view(K, 4)
        fu._opts = g.native.CPpoOptions(old_val.data_ptr(), fu.clip_range_vf.data_ptr(), fu.scale.data_ptr())
        fu.begin_update(0.5)
        fu.step(idx)
        torch.cuda.synchronize()
        for what, big, n in (("old_val", big_old, bt.n), ("clip_range_vf", big_vf, K), ("scale", big_sc, 4 * K)):
            assert bool((big[:PAD] == SENT).all()) and bool((big[PAD + n:] == SENT).all()), (name, what)
        assert torch.equal(fu.scale.cpu(), torch.tensor([list(f) + [1.0] for f in FACTORS], dtype=torch.float32))
        theta = np.stack([LS.theta_of(pset, k) for k in range(K)])
        assert np.isfinite(theta).all() and bool(torch.isfinite(fu.m).all()) and bool(torch.isfinite(fu.v).all()), name
        assert bool(torch.isfinite(fu.stats).all()) and bool(torch.isfinite(fu.diag).all()), name
        assert fu.step_count.cpu().tolist() == [1, 1, 1]
        results[name] = (theta, fu.m.clone(), fu.stats.clone())
    a, b = results["clean"], results["hostile"]
    diff = float(np.abs(a[0] - b[0]).max())
    print("D=%d B=%d: NaN outside the rows read, sentinels intact; clean vs hostile parameters differ by %.3e" % (D, B, diff))
    if B <= 64:
        assert np.array_equal(a[0], b[0]) and H.bits_equal(a[1], b[1]) and H.bits_equal(a[2], b[2])
    else:
        assert diff <= 1e-2 * max(c.learning_rate for c in cfgs)


# ---- GPU: the trainers ------------------------------------------------------------------------------------------------
T_STEPS, T_BATCH, T_EPOCHS = 8, 64, 2                      # 64 envs x 8 steps = 512 rows: 8 minibatches x 2 epochs
T_UPDATES = 16


def _solo_trainer(g, **cfg_kw):
    return LS.solo_trainer(g, g.PPOConfig(seed=13, n_steps=T_STEPS, batch_size=T_BATCH, n_epochs=T_EPOCHS, **cfg_kw))


@pytest.mark.gpu
def test_trainer_takes_the_new_entry_only_with_options(gpu, monkeypatch):
    """PPOTrainer with none of the four fields: not one call of the new symbol, and the statistics it always returned.
    With clip_range_vf: one call per minibatch, the guarded statistics, and the effective numbers in the log."""
    g = gpu
    calls = LS.count_calls(g, monkeypatch, ENTRY)
    a = _solo_trainer(g)
    sa = LS.iterate(a)
    assert calls == [] and not a._fused_update.guarded and not a._fused_update.options
    assert sorted(sa) == ["pg_loss", "std", "value_loss"]
    b = _solo_trainer(g, clip_range_vf=0.01)
    sb = LS.iterate(b)
    print("no options: %s\nclip_range_vf=0.01: %s (%d calls of the new entry)" % (sa, sb, len(calls)))
    assert len(calls) == T_UPDATES and b._fused_update.options and b._fused_update.guarded
    assert sb["n_applied"] == T_UPDATES and sb["early_stop"] is False
    assert (sb["learning_rate"], sb["clip_range"], sb["clip_range_vf"]) == (3e-4, 0.2, 0.01)
    assert np.isfinite([sb["pg_loss"], sb["value_loss"], sb["approx_kl"], sb["clip_fraction"]]).all()
    assert int(b._fused_update.step_count.item()) == T_UPDATES
    name = R.PARAM_NAMES[8]                                 # the critic took other steps than the unclipped twin's
    assert not H.bits_equal(a.policy.get_parameter(name).detach(), b.policy.get_parameter(name).detach())


@pytest.mark.gpu
def test_learn_applies_the_linear_schedule_and_clamps_the_overshoot(gpu):
    """learn() with linear_schedule(): the logged learning_rate is cfg.learning_rate x max(0, 1 - timesteps / total) per
    iteration, and the last, overshooting iteration (factor 0) changes no parameter."""
    g = gpu
    tr = _solo_trainer(g, learning_rate_schedule=g.ppo.linear_schedule())
    per_iter = T_STEPS * 64
    total = int(2.5 * per_iter)
    snaps = []
    hist = tr.learn(total, log=lambda rec: snaps.append(R.flat_params(tr.policy)))
    assert [r["timesteps"] for r in hist] == [per_iter, 2 * per_iter, 3 * per_iter] and tr.total_timesteps is None
    for r in hist:
        want = tr.cfg.learning_rate * max(0.0, 1.0 - r["timesteps"] / total)
        print("iteration %d at %d of %d timesteps: learning_rate %.8g (want %.8g), n_applied %d" % (r["iteration"], r["timesteps"], total, r["learning_rate"], want, r["n_applied"]))
        assert r["learning_rate"] == want and r["clip_range"] == tr.cfg.clip_range and r["n_applied"] == T_UPDATES
    assert hist[-1]["learning_rate"] == 0.0
    assert not np.array_equal(snaps[0], snaps[1]) and np.array_equal(snaps[1], snaps[2])
    assert int(tr._fused_update.step_count.item()) == 3 * T_UPDATES          # (Adam's count went on)
    assert tr._progress_remaining() == 1.0                                   # outside learn()


@pytest.mark.gpu
def test_population_member_without_options_equals_its_guarded_twin(gpu, monkeypatch):
    """PopulationTrainer, K = 2, options on member 0 only: member 1 equals its twin in a population that has
    diagnostics=True and no options, bit for bit (minibatches of 64 rows: one atomic add per gradient entry)."""
    g = gpu
    K, EM = 2, 64

    def population(options, **kw):
        venv = g.ACAS2DVecEnv(K * EM, 1, device=DEV, seed=13)
        cfgs = [g.PPOConfig(seed=13 + k, n_steps=T_STEPS, batch_size=T_BATCH, n_epochs=T_EPOCHS, **(options if k == 0 else {}))
                for k in range(K)]
        return g.PopulationTrainer(venv, cfgs, gae="kernel", **kw)

    calls = LS.count_calls(g, monkeypatch, ENTRY)
    twin = population({}, diagnostics=True)
    twin.collect()
    s_twin = twin.update()
    torch.cuda.synchronize()
    assert calls == [] and twin._fused_update.guarded and not twin._fused_update.options
    pop = population(dict(clip_range_vf=0.2, learning_rate_schedule=_const(0.5)))
    pop.collect()
    st = pop.update()
    torch.cuda.synchronize()
    fu = pop._fused_update
    print("population (options, none):", st, "calls of the new entry", len(calls))
    assert len(calls) == T_UPDATES and fu.options
    for n in R.PARAM_NAMES:
        assert H.bits_equal(pop.policy_set.params[n][1], twin.policy_set.params[n][1]), n
        if "value_net" in n and n.endswith("weight"):
            assert not H.bits_equal(pop.policy_set.params[n][0], twin.policy_set.params[n][0]), n
    assert H.bits_equal(fu.m[1], twin._fused_update.m[1]) and H.bits_equal(fu.v[1], twin._fused_update.v[1])
    assert H.bits_equal(fu.diag[1], twin._fused_update.diag[1]) and H.bits_equal(fu.stats[1], twin._fused_update.stats[1])
    assert {k: v for k, v in st[1].items() if k not in ("learning_rate", "clip_range")} == s_twin[1]
    assert (st[0]["learning_rate"], st[0]["clip_range"], st[0]["clip_range_vf"]) == (1.5e-4, 0.2, 0.2)
    assert (st[1]["learning_rate"], st[1]["clip_range"]) == (3e-4, 0.2) and "clip_range_vf" not in st[1]


@pytest.mark.gpu
def test_pbt_exploit_leaves_the_options_with_their_slot(gpu):
    """PBTTrainer: an exploit step copies and perturbs the hyper ROW; clip_range_vf and the schedules of each slot stay,
    and the logged learning_rate is the perturbed row's rate times the slot's factor."""
    g = gpu
    K, EM = 4, 64
    venv = g.ACAS2DVecEnv(K * EM, 1, device=DEV, seed=13)
    scheds = [_const(0.5), None, _const(0.25), _const(2.0)]
    vfs = [0.2, None, 0.4, 0.1]
    cfgs = [g.PPOConfig(seed=13 + k, n_steps=T_STEPS, batch_size=T_BATCH, n_epochs=T_EPOCHS, clip_range_vf=vfs[k],
                        learning_rate_schedule=scheds[k]) for k in range(K)]
    pbt = g.PBTTrainer(venv, cfgs, g.PBTConfig(ready_every=1000, fraction=0.25, seed=3), gae="kernel")
    fu = pbt._fused_update
    assert fu.options
    vf_before = fu.clip_range_vf.clone()
    pbt.collect()
    s0 = pbt.update()
    assert [s["learning_rate"] for s in s0] == [3e-4 * f for f in (0.5, 1.0, 0.25, 2.0)]
    pbt.window["score"].copy_(torch.tensor([5.0, 7.0, 6.0, 1.0]))          # member 3 is the worst, member 1 the best
    recs = pbt.exploit()
    torch.cuda.synchronize()
    assert recs[3]["exploit"] == 1 and [r["exploit"] for r in recs[:3]] == [None] * 3
    row = recs[3]["hyper"]
    assert any(abs(row[4] / float(np.float32(3e-4)) - f) < 1e-6 for f in (0.8, 1.2)), row          # perturbed
    assert H.bits_equal(fu.clip_range_vf, vf_before)
    assert [c.clip_range_vf for c in pbt.configs] == vfs and [c.learning_rate_schedule for c in pbt.configs] == scheds
    pbt.collect()
    s1 = pbt.update()
    torch.cuda.synchronize()
    print("after the exploit: member 3's row", row, "logged", s1[3])
    assert s1[3]["learning_rate"] == row[4] * 2.0 and s1[3]["clip_range"] == row[0] * 1.0 and s1[3]["clip_range_vf"] == 0.1
    assert s1[0]["learning_rate"] == recs[0]["hyper"][4] * 0.5 and s1[0]["clip_range_vf"] == 0.2
    assert torch.equal(fu.scale.cpu()[:, 0], torch.tensor([0.5, 1.0, 0.25, 2.0]))
