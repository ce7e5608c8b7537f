"""SB3's target_kl early stop and its train/approx_kl, train/clip_fraction on the device:
acas2d_ppo_update_guarded_set_f32 (csrc/acas2d_ppo_guard.hip) and the host code over it (ppo.PPOConfig.target_kl,
FusedUpdate / FusedUpdateSet's guarded entry, the three trainers, ppo.approx_kl_and_clip_fraction,
ppo.explained_variance), against the float64 restatement of tests/kl_guard_ref.py.

  CPU  the two symbols and the struct's size; every rejection before a launch; the two torch helpers against NumPy; the
       config rules; SB3's break in the op-by-op update; the register guard of the new unit.
  GPU  the statistics of one guarded call (approx_kl within 1e-5 max(1, kl64) -- the bound stats[4] / stats[5] are held to:
       a float32 log-prob error of ~1e-6 enters (r - 1) - log r times |r - 1| -- and the clipped fraction exactly); the
       decision over three calls of K = 3 members; guard off == the unguarded entries bit for bit where one workgroup
       adds each gradient entry; begin_update(); the three trainers.
The statistics, the bitwise identity and the decision over three calls run at every compiled width (8, 11, 14, 17, 29, 53,
101, 197: all eight guarded instantiations are launched); tests/test_kl_guard_edges.py takes the same entry to the
hand-placed edge minibatches, to B = 8 193, to the float32 boundary of the decision and through sentinels.
Every criterion prints what it observed.

Observed (MI355X): approx_kl at most 0.081 of its bound over the 80 statistics cases (8.1e-7 absolute, D = 17, K = 3,
B = 2; 0.055 at D = 17, K = 1, B = 2; 0.020 at D = 53, K = 3, B = 2; at most 0.006 elsewhere); the clipped fraction exact
in every case.  The 141 GPU tests of this file take 9.7 s."""
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

torch = pytest.importorskip("torch")
DEV = "cuda:0"
NARROW, WIDE = (8, 11, 14, 17, 29), (53, 101, 197)
WIDTHS = NARROW + WIDE                 # every compiled guarded instantiation: what n_traffic 1, 2, 3, 4, 8, 16, 32, 64 take
GUARDED = "acas2d_ppo_update_guarded_set_f32"


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
def test_guarded_entry_is_exported_and_declared(g):
    L = g.native.lib()
    for name in (GUARDED, "acas2d_ppo_guard_size"):
        assert name in g.native.EXPORTS and getattr(L, name)
    assert C.sizeof(g.native.CPpoGuard) == L.acas2d_ppo_guard_size() == 3 * 8
    header = re.sub(r"\s+", " ", open(os.path.join(H.ROOT, "include", "acas2d.h")).read())
    assert ("int %s(const Acas2dPpoUpdateSet *u, const Acas2dPpoGuard *g, void *stream);" % GUARDED) in header
    assert L.acas2d_abi_version() == g.native.ABI_VERSION == 7
    print("CPpoGuard: %d bytes" % C.sizeof(g.native.CPpoGuard))


def test_guarded_update_validation_needs_no_gpu(g):
    """acas2d_ppo_update_guarded_set_f32 rejects every bad argument with ACAS2D_EINVAL and a message before any HIP call
    (the pointers are host addresses: a launch would fail otherwise)."""
    L = g.native.lib()
    buf = (C.c_double * 64)()
    a = C.addressof(buf)
    names = [n for n, _ in g.native.CPpoUpdateSet._fields_]
    ints = dict(n_members=3, n_rows=64, obs_dim=8, apply=1)

    def call(guard=(a, a, a), **kw):
        return L.acas2d_ppo_update_guarded_set_f32(*LS.host_update_set_args(g, a, guard=guard, **{**ints, **kw}))

    def rejects(msg, **kw):
        assert call(**kw) == -22, kw
        err = L.acas2d_last_error()
        print("  %-40s %s" % (kw, err.decode()[:110]))
        assert msg.encode() in err and b"acas2d_ppo_update_guarded_set" in err, (kw, err)

    for n in names:                                        # check_update's rejections
        if n not in ints:
            rejects("every pointer is required", **{n: None})
    for B in (1, 0, -5):
        rejects("n_rows = %d" % B, n_rows=B)
    assert L.acas2d_ppo_update_guarded_set_f32(None, None, None) == -22 and b"NULL argument" in L.acas2d_last_error()
    rejects("target_kl, stopped, diag", guard=None)        # the guard's own
    for hole in range(3):
        rejects("target_kl, stopped, diag", guard=tuple(None if i == hole else a for i in range(3)))
    for K in (0, -1, 65536):
        rejects("n_members = %d" % K, n_members=K)
    for D in (0, 7, 9, 30, 52, 54, 100, 198):
        rejects("obs_dim = %d" % D, obs_dim=D)
        assert b"8, 11, 14, 17, 29, 53, 101, 197" in L.acas2d_last_error()
    for D in NARROW + WIDE:                                # the probe mode, at every width: sent to the unguarded entries
        rejects("apply = 0", obs_dim=D, apply=0)
        err = L.acas2d_last_error()
        assert b"acas2d_ppo_update_set_f32" in err and b"acas2d_ppo_update_wide_set_f32" in err and b"no stop to decide" in err


def test_approx_kl_clip_fraction_and_explained_variance_against_numpy(g):
    rng = np.random.default_rng(5)
    n, D = 257, 11
    torch.manual_seed(5)
    pol = g.ActorCritic(D).double()
    with torch.no_grad():
        pol.action_net.weight.mul_(40.0)
        pol.log_std.fill_(-0.7)
    obs, act = rng.uniform(-1, 1, (n, D)), rng.normal(0, 0.7, n)
    theta = R.flat_params(pol)
    lp = R.logp64(g.ActorCritic, D, theta, obs, act)          # (rounds the observations to float32 first)
    old = lp + rng.normal(0, 0.5, n)
    cfg = g.PPOConfig(clip_range=0.2)
    t = lambda x: torch.as_tensor(np.asarray(x, np.float64))  # noqa: E731
    kl, cf = g.ppo.approx_kl_and_clip_fraction(pol, cfg, t(R.obs32(obs)), t(act).reshape(-1, 1), t(old))
    assert not kl.requires_grad and not cf.requires_grad
    lr = lp - old
    kl64, (count, cf64) = KR.approx_kl64(lr), KR.clip_fraction64(lr, 0.2)
    print("approx_kl %.12g vs %.12g, clip_fraction %.6f vs %.6f (%d of %d rows)" % (float(kl), kl64, float(cf), cf64, count, n))
    assert abs(float(kl) - kl64) <= 1e-12 * max(1.0, kl64) and float(cf) == cf64 and 0 < count < n
    # explained_variance: flat, per member, and constant returns
    val, ret = rng.normal(0, 1, (3, 50)), rng.normal(2, 3, (3, 50))
    ret[1] = 4.25
    ev = g.ppo.explained_variance(t(val), t(ret)).numpy()
    ref = np.array([np.nan if np.var(ret[k]) == 0 else 1 - np.var(ret[k] - val[k]) / np.var(ret[k]) for k in range(3)])
    print("explained_variance", ev, "vs", ref)
    assert np.isnan(ev[1]) and np.isnan(ref[1]) and np.allclose(ev[[0, 2]], ref[[0, 2]], rtol=1e-12, atol=0)
    flat = g.ppo.explained_variance(t(val[0]), t(ret[0]))
    assert flat.dim() == 0 and abs(float(flat) - ref[0]) <= 1e-12
    assert np.isnan(float(g.ppo.explained_variance(t(val[1]), t(ret[1]))))
    assert float(g.ppo.explained_variance(t(ret[0]), t(ret[0]))) == 1.0


def test_target_kl_config_rules(g):
    c = g.PPOConfig(target_kl=0.03)
    assert c.target_kl == 0.03 and dataclasses.replace(c, seed=5).target_kl == 0.03
    assert g.PPOConfig(**dataclasses.asdict(c)) == c
    assert g.PPOConfig().target_kl is None and g.PPOConfig.sb3().target_kl is None
    assert g.PPOConfig.sb3(target_kl=0.01).target_kl == 0.01
    assert "target_kl" in g.ppo.MEMBER_FIELDS and "target_kl" not in g.ppo.HYPER_SLOTS and len(g.ppo.HYPER_SLOTS) == 8
    venv = types.SimpleNamespace(dtype=torch.float32, n_traffic=1, obs_dim=8, num_envs=3 * 64, device="cpu")
    cfgs = [g.PPOConfig(seed=13, target_kl=t) for t in (None, 0.01, 0.05)]       # differ ONLY in target_kl
    with pytest.raises(AttributeError, match="reset"):       # accepted: construction gets as far as the env (a stub)
        g.PopulationTrainer(venv, cfgs)
    with pytest.raises(AttributeError, match="reset"):
        g.PBTTrainer(venv, cfgs, g.PBTConfig(ready_every=2, fraction=0.0))
    for kw in (dict(use_graphs=True), dict(use_graphs=True, updater="graphs", collector="graphs")):
        with pytest.raises(ValueError, match="updater='fused'"):                 # the captured torch-op updater cannot stop
            g.PPOTrainer(venv, g.PPOConfig(target_kl=0.01), **kw)
    with pytest.raises(ValueError, match="updater='fused'"):
        g.PPOTrainer(venv, g.PPOConfig(), use_graphs=False, diagnostics=True)
    with pytest.raises(AttributeError, match="reset"):       # the fused updater takes it
        g.PPOTrainer(venv, g.PPOConfig(target_kl=0.01), use_graphs=True, collector="fused", updater="fused")


def test_eager_update_breaks_before_the_optimizer_step(g):
    """The op-by-op PPOTrainer.update() with target_kl: SB3's rule.  A huge limit changes nothing; a tiny one stops at
    the first minibatch whose approx_kl exceeds it, before its optimizer step."""
    n, D = 256, 8
    rng = np.random.default_rng(3)
    venv = types.SimpleNamespace(dtype=torch.float32, n_traffic=1, obs_dim=D, num_envs=64, device="cpu",
                                 reset=lambda: torch.zeros(64, D))
    obs = torch.as_tensor(rng.uniform(-1, 1, (n, D)), dtype=torch.float32)
    act = torch.as_tensor(rng.normal(0, 0.7, (n, 1)), dtype=torch.float32)
    adv, ret = (torch.as_tensor(rng.normal(m, 2, n), dtype=torch.float32) for m in (0, 2))
    val = torch.as_tensor(rng.normal(2, 1, n), dtype=torch.float32)
    out = {}
    for name, tk in (("none", None), ("huge", 1e9), ("tiny", 1e-12)):
        tr = g.PPOTrainer(venv, g.PPOConfig(seed=7, batch_size=64, n_epochs=3, target_kl=tk), use_graphs=False)
        with torch.no_grad():
            mean, _ = tr.policy.forward(obs)
            old = g.ppo._normal_logp(mean, tr.policy.log_std, act)
        torch.manual_seed(11)
        st = tr.update(obs, act, old, adv, ret, val)
        steps = {int(s["step"]) for s in tr.opt.state_dict()["state"].values()}
        out[name] = (st, R.flat_params(tr.policy), steps)
        print(name, st, "optimizer steps", steps)
    assert np.array_equal(out["none"][1], out["huge"][1]) and out["none"][2] == out["huge"][2] == {12}
    assert "approx_kl" not in out["none"][0]
    st = out["huge"][0]
    assert st["n_applied"] == 12 and not st["early_stop"]
    assert np.isfinite([st["approx_kl"], st["clip_fraction"], st["explained_variance"]]).all() and st["approx_kl"] > 0
    st, _, steps = out["tiny"]
    assert st["early_stop"] and st["n_applied"] < 12 and steps == ({st["n_applied"]} if st["n_applied"] else set())


@H.needs_hipcc
def test_guarded_update_kernels_stay_in_registers_and_lds(g, tmp_path):
    """csrc/acas2d_ppo_guard.hip: five narrow gradient kernels, three wide ones and the apply kernel.  None spills either
    register file or uses scratch; the narrow ones use at most 256 VGPRs (test_ppo_update_set_kernels_stay_in_registers'
    rule); the wide ones are held to what tests/test_wide_update.py and tests/test_population_wide.py hold the unguarded
    kernel of the same width to: at most 256 VGPRs, 256 threads, acas2d_ppo_wide_lds_bytes of dynamic LDS plus the static
    LDS within gfx950's 160 KB."""
    _, kernels = H.kernel_metadata(tmp_path, "acas2d_ppo_guard.hip")
    assert len(kernels) == 9
    L = g.native.lib()
    seen = {"narrow": [], "wide": [], "apply": 0}
    for k in kernels:
        name = k.name
        print(name[:70], "vgpr", k.field("vgpr_count"), "sgpr", k.field("sgpr_count"), "static LDS",
              k.field("group_segment_fixed_size"))
        assert k.field("vgpr_spill_count") == 0 and k.field("sgpr_spill_count") == 0, name
        assert k.field("private_segment_fixed_size") == 0 and k.field("vgpr_count") <= 256, name
        if "ppo_apply_guarded_set_kernel" in name:
            seen["apply"] += 1
            assert k.field("max_flat_workgroup_size") == 1024, name
            continue
        D = int(re.search(r"kernelILi(\d+)E", name).group(1))
        if "ppo_grad_wide_guarded_set_kernel" in name:
            seen["wide"].append(D)
            assert k.field("max_flat_workgroup_size") == 256, name
            lds = L.acas2d_ppo_wide_lds_bytes(D)
            assert lds + k.field("group_segment_fixed_size") <= 160 * 1024, (D, lds)
        else:
            assert "ppo_grad_guarded_set_kernel" in name
            seen["narrow"].append(D)
            assert k.field("max_flat_workgroup_size") == 64, name
    assert sorted(seen["narrow"]) == list(NARROW) and sorted(seen["wide"]) == list(WIDE) and seen["apply"] == 1


# ---- GPU: the kernels -------------------------------------------------------------------------------------------------
STAT_CASES = [(D, K, B) for D in WIDTHS for K in (1, 3) for B in (2, 63, 64, 65, 130)]


@pytest.mark.gpu
@pytest.mark.parametrize("D,K,B", STAT_CASES, ids=["D%d-K%d-B%d" % c for c in STAT_CASES])
def test_guarded_statistics_vs_float64(gpu, D, K, B):
    """One guarded call with the limit off: diag[k][2] against approx_kl64 within 1e-5 max(1, kl64), diag[k][3] ==
    float32(count64) / float32(B) exactly (no row within 1e-4 of its clip range, asserted first), the accumulators
    closed, the step applied.  Then a first-epoch minibatch (ratio ~ 1): approx_kl < 1e-6, clip_fraction == 0.
    B = 2 and 63 leave dead lanes, 64 fills one workgroup, 65 and 130 add a second (and third) whose atomics land in the
    same accumulator.
    Observed on an MI355X: approx_kl at most 0.081 of the bound (8.1e-7 absolute; D = 17, K = 3, B = 2), 0.055 and 0.020 at
    D = 17, K = 1 and D = 53, K = 3 (both B = 2), at most 0.006 in the other 77 cases."""
    g = gpu
    bt = LS.RolloutBatch(g, D, K, K * B + 317, seed=6000 + 7 * D + 31 * K + B)
    cfgs = LS.member_cfgs(g, K)
    clips = [c.clip_range for c in cfgs]
    pset = bt.policy_set()
    fu = g.FusedUpdateSet(pset, cfgs, *bt.bufs, diagnostics=True)
    assert fu.guarded and float(fu.target_kl.abs().max()) == 0.0
    worst = 0.0
    for call, mode in enumerate(("mixed", "first"), 1):
        idx = LS.draw(bt, pset, clips, B, mode)
        theta = [LS.theta_of(pset, k) for k in range(K)]
        fu.begin_update()
        fu.step(idx)
        torch.cuda.synchronize()
        diag = fu.diag.cpu().numpy()
        assert fu.stopped.cpu().tolist() == [0] * K and fu.step_count.cpu().tolist() == [call] * K
        for k in range(K):
            lr = bt.log_ratio(theta[k], idx[k])
            clip = cfgs[k].clip_range
            assert KR.edge_distance(lr, clip) >= 1e-4, (k, KR.edge_distance(lr, clip))
            kl64, (count, _) = KR.approx_kl64(lr), KR.clip_fraction64(lr, clip)
            frac = abs(float(diag[k, 2]) - kl64) / (1e-5 * max(1.0, kl64))
            worst = max(worst, frac)
            print("D=%d K=%d B=%d %s member %d: approx_kl %.8g vs %.8g (%.3f of the bound), clipped %d of %d -> %.8g"
                  % (D, K, B, mode, k, diag[k, 2], kl64, frac, count, B, diag[k, 3]))
            assert frac <= 1.0, (k, diag[k, 2], kl64)
            assert diag[k, 3] == np.float32(count) / np.float32(B), (k, diag[k, 3], count, B)
            assert diag[k, 0] == 0.0 and diag[k, 1] == 0.0
            assert diag[k, 4] == diag[k, 2] and diag[k, 5] == diag[k, 3] and diag[k, 6] == 1.0 and diag[k, 7] == 1.0
            if mode == "mixed" and B >= 63:
                assert 0 < count < B and kl64 > 1e-2
            if mode == "first":
                assert np.abs(np.exp(lr) - 1).max() < 1e-5
                assert diag[k, 2] < 1e-6 and diag[k, 3] == 0.0 and count == 0
        d = fu.diagnostics()
        assert [x["n_minibatches"] for x in d] == [1] * K and [x["n_applied"] for x in d] == [1] * K
        assert not any(x["early_stop"] for x in d)
    print("D=%d K=%d B=%d: worst approx_kl error %.3f of the 1e-5 bound" % (D, K, B, worst))


def _decision_run(g, D, B, seed):
    """Three guarded calls of K = 3 members on fresh minibatches.  None where member 1's limit does not clear its three
    minibatches by the margin the test wants (the caller re-draws the seed)."""
    K = 3
    b1, b2, eps = 0.9, 0.999, 1e-5
    bt = LS.RolloutBatch(g, D, K, K * B + 317, seed=seed)
    cfgs = LS.member_cfgs(g, K)
    clips = [c.clip_range for c in cfgs]
    pset = bt.policy_set()
    segs = R.segments(bt.pols[0])
    fu = g.FusedUpdateSet(pset, cfgs, *bt.bufs, diagnostics=True)
    frozen = None
    for call in (1, 2, 3):
        idx = LS.draw(bt, pset, clips, B)
        theta0 = [LS.theta_of(pset, k) for k in range(K)]
        kl64 = [KR.approx_kl64(bt.log_ratio(theta0[k], idx[k])) for k in range(K)]
        if call == 1:
            target = [kl64[0] / 3.0, kl64[1] * 2.0, 0.0]
            fu.target_kl.copy_(torch.tensor(target, dtype=torch.float32))
            fu.begin_update()
            torch.cuda.synchronize()
            frozen = dict(theta=theta0[0], m=fu.m[0].clone(), v=fu.v[0].clone(), params=[p[0].clone() for p in fu._params])
            assert KR.stops(kl64[0], target[0]) and not KR.stops(kl64[1], target[1]) and not KR.stops(kl64[2], target[2])
        if not 1.5 * target[1] >= 1.5 * kl64[1]:           # member 1 must clear each of ITS minibatches by 1.5 x
            print("seed %d: member 1's minibatch %d has approx_kl %.4g against the limit %.4g -- re-draw" % (seed, call, kl64[1], target[1]))
            return None
        m0, v0 = fu.m.double().cpu().numpy(), fu.v.double().cpu().numpy()
        s0 = fu.step_count.cpu().tolist()
        fu.step(idx)
        torch.cuda.synchronize()
        diag, stats, stopped = fu.diag.cpu().numpy(), fu.stats.double().cpu().numpy(), fu.stopped.cpu().tolist()
        print("D=%d B=%d call %d: approx_kl64 %s, limits %s, stopped %s, diag[:, 6] %s, diag[:, 7] %s, adam_step %s"
              % (D, B, call, ["%.4g" % x for x in kl64], ["%.4g" % x for x in target], stopped, diag[:, 6], diag[:, 7],
                 fu.step_count.cpu().tolist()))
        # ---- member 0: stopped on call 1, and nothing of it moves afterwards
        assert stopped[0] == 1 and fu.step_count[0].item() == 0
        for name, p, q in zip(R.PARAM_NAMES, fu._params, frozen["params"]):
            assert torch.equal(p[0], q), (call, name)
        assert torch.equal(fu.m[0], frozen["m"]) and torch.equal(fu.v[0], frozen["v"]), call
        assert float(fu.grad[0].abs().max()) == 0.0, call
        assert diag[0, 6] == 1.0 and diag[0, 7] == 0.0 and diag[0, 0] == 0.0 and diag[0, 1] == 0.0
        if call == 1:
            obs, act, old, adv, ret = bt.host(idx[0])
            _, pg0, vf0, _ = R.grad64(g.ActorCritic, cfgs[0], D, theta0[0], obs, act, old, adv, ret)
            frozen.update(kl=diag[0, 2].copy(), pg=pg0, vf=vf0)
            assert abs(float(diag[0, 2]) - kl64[0]) <= 1e-5 * max(1.0, kl64[0])
        assert diag[0, 2] == frozen["kl"], (call, diag[0, 2], frozen["kl"])            # still call 1's
        assert stats[0, 0] == 0.0 and stats[0, 1] == 0.0 and stats[0, 2] == 0.0         # no norm was ever taken
        assert abs(stats[0, 4] - frozen["pg"]) <= 1e-5 * max(1.0, abs(frozen["pg"])), (call, stats[0, 4], frozen["pg"])
        assert abs(stats[0, 5] - frozen["vf"]) <= 1e-5 * max(1.0, frozen["vf"]), (call, stats[0, 5], frozen["vf"])
        # ---- members 1 and 2: every step applied, each against float64 from the kernel's own pre-step state
        m1, v1 = fu.m.double().cpu().numpy(), fu.v.double().cpu().numpy()
        for k in (1, 2):
            what = "D=%d B=%d member %d step %d" % (D, B, k, call)
            assert stopped[k] == 0 and diag[k, 6] == call and diag[k, 7] == call and fu.step_count[k].item() == call == s0[k] + 1
            assert abs(float(diag[k, 2]) - kl64[k]) <= 1e-5 * max(1.0, kl64[k]), what
            assert float(fu.grad[k].abs().max()) == 0.0 and stats[k, 0] == 0.0 and stats[k, 1] == 0.0, what
            c = cfgs[k]
            obs, act, old, adv, ret = bt.host(idx[k])
            grad, pg, vf, _ = R.grad64(g.ActorCritic, c, D, theta0[k], obs, act, old, adv, ret)
            theta_ref, m_ref, v_ref, norm = R.adam64(theta0[k], grad, m0[k], v0[k], s0[k], c.max_grad_norm, c.learning_rate,
                                                     b1, b2, eps)
            for key, got_, ref_, tol in (("norm", stats[k, 2], norm, 1e-5 * norm), ("pg", stats[k, 4], pg, 1e-5 * max(1.0, abs(pg))),
                                         ("vf", stats[k, 5], vf, 1e-5 * max(1.0, vf))):
                assert abs(got_ - ref_) <= tol, (what, key, got_, ref_)
            LS.assert_per_tensor("m " + what, m1[k], m_ref, segs, LS.TAU_M)
            LS.assert_per_tensor("v " + what, v1[k], v_ref, segs, LS.TAU_V)
            theta1 = LS.theta_of(pset, k)
            ulp = np.spacing(np.abs(theta_ref).astype(np.float32)).astype(np.float64)
            excess = (np.abs(theta1 - theta_ref) - ulp) / c.learning_rate
            print("  %s: parameter excess %.2e lr (bound 1e-2)" % (what, float(excess.max())))
            assert excess.max() <= 1e-2, (what, float(excess.max()), int(excess.argmax()))
            assert np.median(np.abs(theta1 - theta0[k]) / c.learning_rate) > 0.05, what    # the step was taken
    d = fu.diagnostics()
    assert [x["early_stop"] for x in d] == [True, False, False] and [x["n_applied"] for x in d] == [0, 3, 3]
    assert [x["n_minibatches"] for x in d] == [1, 3, 3]
    return True


@pytest.mark.gpu
@pytest.mark.parametrize("D", WIDTHS)
def test_guarded_decision_over_three_calls(gpu, D):
    """K = 3, three calls on fresh minibatches of 65 rows (two workgroups per network, one of them a single live lane).
    Member 0: target_kl = kl64 / 3, stops on call 1 and stays as it was before it -- parameters, moments and step count bit
    for bit, its gradient block zero, diag[0][6] == 1, diag[0][7] == 0, diag[0][2] and the logged losses call 1's.
    Member 1: target_kl = 2 kl64 (never reached: asserted per minibatch in float64, else the seed is re-drawn); member 2:
    no limit.  Both apply all three steps, each matching adam64(grad64(...)) at learner_support.py's bounds."""
    for seed in range(7000 + D, 7000 + D + 5000, 1000):
        if _decision_run(gpu, D, 65, seed):
            return
    raise AssertionError("no seed out of five gave member 1 a limit that clears its three minibatches")


IDENTITY_CASES = [(D, K, B) for D in WIDTHS for K in (1, 3) for B in (2, 63, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("D,K,B", IDENTITY_CASES, ids=["D%d-K%d-B%d" % c for c in IDENTITY_CASES])
def test_guard_off_equals_the_unguarded_entries_bitwise(gpu, D, K, B):
    """B <= 64: every gradient entry receives one atomic add, so the result does not depend on their order.  With every
    target_kl zero, two guarded calls leave the parameters, moments, step counts and logged statistics of
    acas2d_ppo_update_set_f32 (D <= 29) / acas2d_ppo_update_wide_set_f32 (D >= 53) on a twin, bit for bit; at K = 1
    also those of the solo entries (FusedUpdate as it always was), through FusedUpdateSet's and FusedUpdate's guarded
    paths alike.  A difference here means the guard changed the shared arithmetic."""
    g = gpu
    # (seeds from 8500: with the earlier 8000 the two minibatches of D = 101, K = 1, B = 2 hold four rows that the surrogate
    # clips on the side where its gradient is exactly 0 -- float64 autograd gives no actor gradient either, and the
    # `moved > 0` below, which looks at an actor matrix, cannot hold for any correct kernel; about 1 draw in 70 at B = 2)
    bt = LS.RolloutBatch(g, D, K, K * B + 317, seed=8500 + 7 * D + 31 * K + B)
    cfgs = LS.member_cfgs(g, K)
    clips = [c.clip_range for c in cfgs]
    twins = {"plain": bt.policy_set(), "guarded": bt.policy_set()}
    fus = {"plain": g.FusedUpdateSet(twins["plain"], cfgs, *bt.bufs),
           "guarded": g.FusedUpdateSet(twins["guarded"], cfgs, *bt.bufs, diagnostics=True)}
    assert not fus["plain"].guarded and fus["guarded"].guarded
    assert fus["plain"].entry == ("acas2d_ppo_update_set_f32" if D <= 29 else "acas2d_ppo_update_wide_set_f32")
    solo = {}
    if K == 1:
        for name, kw in (("solo", {}), ("solo guarded", dict(diagnostics=True))):
            pol = twins["plain"].member(0)
            solo[name] = (pol, g.FusedUpdate(pol, cfgs[0], *bt.bufs, **kw))
        assert not solo["solo"][1].guarded and solo["solo guarded"][1].guarded

    def same(what, a, b):
        assert a.shape == b.shape and torch.equal(a, b), (what, D, K, B, float((a.double() - b.double()).abs().max()))

    fus["guarded"].begin_update()
    if K == 1:
        solo["solo guarded"][1].begin_update()
    for call in (1, 2):
        idx = LS.draw(bt, twins["plain"], clips, B)
        for fu in fus.values():
            fu.step(idx)
        for _, fu in solo.values():
            fu.step(idx[0].contiguous())
        torch.cuda.synchronize()
        a, b = fus["plain"], fus["guarded"]
        for n in R.PARAM_NAMES:
            same("call %d %s" % (call, n), twins["plain"].params[n], twins["guarded"].params[n])
        for what, x, y in (("m", a.m, b.m), ("v", a.v, b.v), ("step_count", a.step_count, b.step_count), ("grad", a.grad, b.grad),
                           ("stats", a.stats, b.stats)):
            same("call %d %s" % (call, what), x, y)
        assert a.step_count.cpu().tolist() == [call] * K and b.diag[:, 7].cpu().tolist() == [float(call)] * K
        for name, (pol, fu) in solo.items():
            for n in R.PARAM_NAMES:
                same("call %d %s %s" % (call, name, n), twins["plain"].params[n][0], pol.get_parameter(n).detach())
            same("call %d %s m" % (call, name), a.m[0], fu.m)
            same("call %d %s v" % (call, name), a.v[0], fu.v)
            same("call %d %s step_count" % (call, name), a.step_count, fu.step_count)
            same("call %d %s stats" % (call, name), a.stats[0], fu.stats)
    moved = float((twins["guarded"].params[R.PARAM_NAMES[2]] - torch.stack([p.get_parameter(R.PARAM_NAMES[2]).detach()
                                                                            for p in bt.pols])).abs().max())
    print("D=%d K=%d B=%d: guarded == unguarded%s bit for bit after two steps (parameters moved by %.2e)"
          % (D, K, B, " == solo" if K == 1 else "", moved))
    assert moved > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("D", (8, 53))
def test_begin_update_lets_a_stopped_member_run_again(gpu, D):
    """The three calls again with begin_update() between them: member 0 (a limit it always exceeds) runs again each time
    -- its statistics are this call's, it stops afresh -- and every member without a limit applies every call.  Lifting
    member 0's limit then lets it apply too."""
    g = gpu
    K, B = 3, 65
    bt = LS.RolloutBatch(g, D, K, K * B + 317, seed=9000 + D)
    cfgs = LS.member_cfgs(g, K)
    clips = [c.clip_range for c in cfgs]
    cfgs[0] = dataclasses.replace(cfgs[0], target_kl=1e-6)
    pset = bt.policy_set()
    fu = g.FusedUpdateSet(pset, cfgs, *bt.bufs)
    assert fu.guarded and fu.target_kl.cpu().tolist() == [np.float32(1e-6), 0.0, 0.0]
    theta_0 = LS.theta_of(pset, 0)
    for call in (1, 2, 3):
        idx = LS.draw(bt, pset, clips, B)
        kl64 = KR.approx_kl64(bt.log_ratio(LS.theta_of(pset, 0), idx[0]))
        fu.begin_update()
        torch.cuda.synchronize()
        assert fu.stopped.cpu().tolist() == [0, 0, 0] and float(fu.diag.abs().max()) == 0.0
        fu.step(idx)
        fu.step(idx)                                       # a second minibatch of the same update: member 0 sits it out
        torch.cuda.synchronize()
        diag = fu.diag.cpu().numpy()
        print("D=%d call %d: stopped %s, member 0 approx_kl %.6g vs %.6g, diag[:, 6] %s, diag[:, 7] %s, adam_step %s"
              % (D, call, fu.stopped.cpu().tolist(), diag[0, 2], kl64, diag[:, 6], diag[:, 7], fu.step_count.cpu().tolist()))
        assert fu.stopped.cpu().tolist() == [1, 0, 0]
        assert abs(float(diag[0, 2]) - kl64) <= 1e-5 * max(1.0, kl64) and kl64 > 1.5e-6        # this call's, not an earlier one's
        assert diag[:, 6].tolist() == [1.0, 2.0, 2.0] and diag[:, 7].tolist() == [0.0, 2.0, 2.0]
        assert fu.step_count.cpu().tolist() == [0, 2 * call, 2 * call]
        assert np.array_equal(LS.theta_of(pset, 0), theta_0)
    fu.target_kl[0] = 0.0
    fu.begin_update()
    fu.step(LS.draw(bt, pset, clips, B))
    torch.cuda.synchronize()
    assert fu.stopped.cpu().tolist() == [0, 0, 0] and fu.step_count.cpu().tolist() == [1, 7, 7]
    assert not np.array_equal(LS.theta_of(pset, 0), theta_0)


# ---- GPU: the trainers ------------------------------------------------------------------------------------------------
T_STEPS, T_BATCH, T_EPOCHS, T_UPDATES = 4, 64, 3, 12       # 64 envs x 4 steps = 256 rows: 4 minibatches x 3 epochs


def _solo_trainer(g, target_kl, seed=13, **kw):
    cfg = g.PPOConfig(seed=seed, n_steps=T_STEPS, batch_size=T_BATCH, n_epochs=T_EPOCHS, target_kl=target_kl)
    return LS.solo_trainer(g, cfg, **kw)


def _same_learner(a, b):
    for n in R.PARAM_NAMES:
        assert H.bits_equal(a.policy.get_parameter(n).detach(), b.policy.get_parameter(n).detach()), n
    fa, fb = a._fused_update, b._fused_update
    assert H.bits_equal(fa.m, fb.m) and H.bits_equal(fa.v, fb.v) and H.bits_equal(fa.step_count, fb.step_count)


@pytest.mark.gpu
def test_trainer_without_target_kl_never_takes_the_guarded_entry(gpu, monkeypatch):
    """PPOTrainer(target_kl=None): not one call of the guarded symbol, the statistics it always returned, and the same bits
    as a second such trainer.  target_kl = 1e9 (never reached; B = 64: one atomic add per gradient entry) equals it bit
    for bit, through the guarded entry, and reports all 12 minibatches applied."""
    g = gpu
    calls = LS.count_calls(g, monkeypatch, GUARDED)
    a = _solo_trainer(g, None)                             # (one after the other: the minibatch permutations come from
    sa = LS.iterate(a)                                       # torch's global generator, seeded at construction)
    b = _solo_trainer(g, None)
    sb = LS.iterate(b)
    assert calls == [] and not a._fused_update.guarded
    assert sorted(sa) == ["pg_loss", "std", "value_loss"] and sa == sb
    _same_learner(a, b)
    c = _solo_trainer(g, 1e9)
    sc = LS.iterate(c)
    print("target_kl=None: %s\ntarget_kl=1e9:  %s (%d guarded calls)" % (sa, sc, len(calls)))
    assert len(calls) == T_UPDATES and c._fused_update.guarded
    _same_learner(a, c)
    assert sc["n_applied"] == T_UPDATES and sc["early_stop"] is False and (sc["pg_loss"], sc["value_loss"]) == (sa["pg_loss"], sa["value_loss"])
    assert np.isfinite([sc["approx_kl"], sc["clip_fraction"], sc["explained_variance"]]).all()
    assert sc["approx_kl"] > 0.0 and 0.0 <= sc["clip_fraction"] <= 1.0
    assert int(c._fused_update.step_count.item()) == T_UPDATES
    d = _solo_trainer(g, None, diagnostics=True)           # diagnostics alone: the same again
    sd = LS.iterate(d)
    _same_learner(a, d)
    assert sd["n_applied"] == T_UPDATES and sd["approx_kl"] == sc["approx_kl"]


@pytest.mark.gpu
def test_trainer_stops_early_on_a_tiny_target_kl(gpu):
    """target_kl = 1e-12: some minibatch exceeds it.  Which one is the device's business; the invariants are read from it."""
    g = gpu
    tr = _solo_trainer(g, 1e-12)
    st = LS.iterate(tr)
    fu = tr._fused_update
    d = fu.diagnostics()
    print("target_kl=1e-12:", st, d, "adam_step", int(fu.step_count.item()))
    assert st["early_stop"] is True and d["early_stop"] is True and st["n_applied"] < T_UPDATES
    assert int(fu.step_count.item()) == st["n_applied"] == d["n_applied"]
    assert d["n_minibatches"] == d["n_applied"] + 1
    assert d["last_approx_kl"] > 1.5e-12 and float(fu.diag[0, 2]) == d["last_approx_kl"]
    assert float(fu.grad.abs().max()) == 0.0
    assert np.isfinite([st["approx_kl"], st["clip_fraction"], st["explained_variance"], st["pg_loss"], st["value_loss"]]).all()
    st2 = LS.iterate(tr)                                     # the next update starts afresh (begin_update)
    assert int(fu.step_count.item()) == st["n_applied"] + st2["n_applied"]


@pytest.mark.gpu
def test_population_stops_one_member_and_leaves_the_other_alone(gpu, monkeypatch):
    """PopulationTrainer, K = 2 on 128 envs, target_kl (None, 1e-12).  Member 0 starts from the solo
    PPOTrainer(target_kl=None) of its seed and collects its buffers bit for bit (what tests/test_population.py
    establishes for the unguarded path), and after the update equals member 0 of the unguarded population bit for bit (B =
    64); member 1 stops."""
    g = gpu
    K, EM = 2, 64

    def population(targets, **kw):
        venv = g.ACAS2DVecEnv(K * EM, 1, device=DEV, seed=13)
        cfgs = [g.PPOConfig(seed=13 + k, n_steps=T_STEPS, batch_size=T_BATCH, n_epochs=T_EPOCHS, target_kl=targets[k])
                for k in range(K)]
        return g.PopulationTrainer(venv, cfgs, gae="kernel", **kw)

    calls = LS.count_calls(g, monkeypatch, GUARDED)
    plain = population((None, None))
    plain.collect()
    s_plain = plain.update()
    torch.cuda.synchronize()
    assert calls == [] and sorted(s_plain[0]) == ["pg_loss", "std", "value_loss"]
    pop = population((None, 1e-12))
    solo = _solo_trainer(g, None, seed=13, envs=EM, offset=0)
    for n in R.PARAM_NAMES:
        assert H.bits_equal(pop.policy_set.params[n][0], solo.policy.get_parameter(n).detach()), n
    pop.collect()
    solo.collect()
    torch.cuda.synchronize()
    for name in ("b_obs", "b_act", "b_logp", "b_val", "b_rew", "b_done"):
        assert H.bits_equal(getattr(pop, name)[:, :EM], getattr(solo, name)), name
    st = pop.update()
    torch.cuda.synchronize()
    fu = pop._fused_update
    print("population (None, 1e-12):", st, "adam_step", fu.step_count.cpu().tolist(), "guarded calls", len(calls))
    assert len(calls) == T_UPDATES
    for n in R.PARAM_NAMES:
        assert H.bits_equal(pop.policy_set.params[n][0], plain.policy_set.params[n][0]), n
    assert H.bits_equal(fu.m[0], plain._fused_update.m[0]) and H.bits_equal(fu.v[0], plain._fused_update.v[0])
    assert st[0]["n_applied"] == T_UPDATES and st[0]["early_stop"] is False
    assert (st[0]["pg_loss"], st[0]["value_loss"]) == (s_plain[0]["pg_loss"], s_plain[0]["value_loss"])
    assert st[1]["early_stop"] is True and st[1]["n_applied"] < T_UPDATES
    assert fu.step_count.cpu().tolist() == [T_UPDATES, st[1]["n_applied"]] and fu.stopped.cpu().tolist() == [0, 1]
    for k in range(K):
        assert np.isfinite([st[k]["approx_kl"], st[k]["clip_fraction"], st[k]["explained_variance"]]).all(), k
    vals, rets = pop.b_val[:, :EM].reshape(-1).double().cpu().numpy(), pop.b_ret[:, :EM].reshape(-1).double().cpu().numpy()
    ev64 = 1.0 - np.var(rets - vals) / np.var(rets)
    print("member 0 explained_variance %.8g vs float64 %.8g" % (st[0]["explained_variance"], ev64))
    assert abs(st[0]["explained_variance"] - ev64) <= 1e-4 * max(1.0, abs(ev64))
