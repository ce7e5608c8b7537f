"""acas2d_ppo_update_wide_f32 (csrc/acas2d_ppo_wide.hip): the fused PPO minibatch update at obs_dim 53, 101, 197 (16, 32,
64 traffic aircraft).

CPU: the export, its argument validation, FusedUpdate's choice of entry, and the code object's registers and LDS.
GPU: the recipe of tests/test_learner_kernels.py (learner_support.SoloBatch, its seeds, its criteria) at the new widths --
the raw gradient tensor by tensor against float64 autograd and applied steps each started from the kernel's own state;
the torch path the trainer otherwise runs (the shape of test_ppo.py's test, its bounds); sentinels around the workspace;
PPOTrainer(collector="fused", updater="fused") at 16 and 64 traffic aircraft.

Observed on an MI355X (every case prints its own figure).  Raw gradient: every tensor of every case within the 1e-6
max |ref| term alone -- the per-tensor tau comes out negative, worst -5.7e-7 (D = 53, B = 3, first-epoch minibatch; bound
2e-5); against torch's float32 autograd max |diff| / max |g| 4.8e-7 - 5.5e-7.  Applied steps: parameter excess at most
1.4e-3 lr (D = 197, B = 63; bound 1e-2), m within the tau0 term, v 1.2e-5 (bound 5e-5 -- the float32 beta2, as for the
narrow kernel), norm / pg / vf at most 0.04 / 0.06 / 0.03 of their 1e-5 bounds."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import helpers as H
import learner_ref as R
import learner_support as LS

torch = pytest.importorskip("torch")
DEV = "cuda:0"
WIDE = (53, 101, 197)
ENTRY = "acas2d_ppo_update_wide_f32"


@pytest.fixture(scope="module")
def g():
    import gym_acas2d_amd as g
    return g


@pytest.fixture(scope="module")
def gpu(g):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    g.native.lib()
    return g


# ---- CPU ----------------------------------------------------------------------------------------------------------
def test_library_exports_the_wide_update(g):
    L = g.native.lib()
    assert ENTRY in g.native.EXPORTS and hasattr(L, ENTRY)
    header = open(os.path.join(H.ROOT, "include", "acas2d.h")).read()
    assert re.search(r"int %s\(const Acas2dPpoUpdate \*u, void \*stream\);" % ENTRY, header)
    assert L.acas2d_abi_version() == 7                                  # additive


def _struct(g, **over):
    return LS.host_update(g, **{"obs_dim": 53, **over})


def test_wide_update_validation_needs_no_gpu(g):
    L = g.native.lib()
    f = getattr(L, ENTRY)
    assert f(None, None) == -22 and b"NULL argument" in L.acas2d_last_error()
    pointers = [n for n, t in g.native.CPpoUpdate._fields_ if t is C.c_void_p]
    assert len(pointers) == 24
    for name in pointers:
        u, _keep = _struct(g, **{name: None})
        assert f(C.byref(u), None) == -22, name
        assert b"every pointer is required" in L.acas2d_last_error(), name
    for n_rows in (1, 0, -5):
        u, _keep = _struct(g, n_rows=n_rows)
        assert f(C.byref(u), None) == -22
        assert (b"n_rows = %d" % n_rows) in L.acas2d_last_error()
    for D in (0, 8, 29, 52, 54, 100, 198, -53):
        u, _keep = _struct(g, obs_dim=D)
        assert f(C.byref(u), None) == -22
        assert (b"obs_dim = %d" % D) in L.acas2d_last_error()


def test_fused_update_picks_the_wide_entry_on_host_tensors(g):
    """Nothing is launched: the workspace is the 13 parameter tensors in learner_ref.PARAM_NAMES order, the entry is the
    wide one at the three widths and the narrow one below, any other width raises at construction."""
    L = g.native.lib()
    z = lambda *s: torch.zeros(*s)  # noqa: E731
    for D in WIDE:
        pol = g.ActorCritic(D)
        fu = g.FusedUpdate(pol, g.PPOConfig(), z(4, D), z(4), z(4), z(4), z(4))
        assert len(fu._params) == 13 and all(p is pol.get_parameter(n) for p, n in zip(fu._params, R.PARAM_NAMES))
        total = sum(p.numel() for p in fu._params)
        assert L.acas2d_ppo_workspace_floats(D) == total == fu.grad.numel() == fu.m.numel() == fu.v.numel() == R.segments(pol)[-1][2]
        assert fu.entry == ENTRY and fu.D == D
    fu = g.FusedUpdate(g.ActorCritic(29), g.PPOConfig(), z(4, 29), z(4), z(4), z(4), z(4))
    assert fu.entry == "acas2d_ppo_update_f32"
    with pytest.raises(ValueError, match=r"8, 11, 14, 17, 29.*53, 101, 197.*got 30"):
        g.FusedUpdate(g.ActorCritic(30), g.PPOConfig(), z(4, 30), z(4), z(4), z(4), z(4))


@H.needs_hipcc
def test_wide_update_kernels_stay_in_registers_and_lds(g, tmp_path):
    """csrc/acas2d_ppo_wide.hip: three gradient kernels (the apply kernel is acas2d_ppo.hip's), no VGPR or SGPR spill, no
    scratch, and the LDS the launcher asks for -- acas2d_ppo_wide_lds_bytes, the one figure the launch uses -- plus the
    kernel's static LDS within gfx950's 160 KB per workgroup."""
    _, kernels = H.kernel_metadata(tmp_path, "acas2d_ppo_wide.hip")
    assert len(kernels) == 3
    L = g.native.lib()
    static = {}
    for k in kernels:
        name = k.name
        assert "ppo_grad_wide_kernel" in name
        assert k.field("vgpr_spill_count") == 0 and k.field("sgpr_spill_count") == 0, name
        assert k.field("private_segment_fixed_size") == 0 and k.field("vgpr_count") <= 256, name
        assert k.field("max_flat_workgroup_size") == 256, name                # four waves per workgroup
        static[int(re.search(r"kernelILi(\d+)E", name).group(1))] = k.field("group_segment_fixed_size")
        print(name, "vgpr", k.field("vgpr_count"), "sgpr", k.field("sgpr_count"))
    assert sorted(static) == list(WIDE)
    for D in WIDE:
        lds = L.acas2d_ppo_wide_lds_bytes(D)
        # at least what the kernel's own layout holds: four [64][65] vectors and a 64 x D observation tile
        assert (4 * 64 * 65 + 64 * D) * 4 <= lds and lds + static[D] <= 160 * 1024, (D, lds, static[D])
        print("D = %d: %d bytes of dynamic LDS + %d static" % (D, lds, static[D]))
    assert L.acas2d_ppo_wide_lds_bytes(29) == -22 and b"obs_dim = 29" in L.acas2d_last_error()


# ---- GPU ----------------------------------------------------------------------------------------------------------
_B_ALL = (2, 3, 63, 64, 65, 127, 129, 2085, 4096)
CASES = [(D, B) for D in WIDE for B in (_B_ALL if D in (53, 197) else (2, 65, 2085))]
_IDS = ["D%d-B%d" % c for c in CASES]


@pytest.mark.gpu
@pytest.mark.parametrize("D,B", CASES, ids=_IDS)
def test_wide_update_raw_gradient_per_tensor_vs_float64(g, gpu, D, B):
    """test_fused_update_raw_gradient_per_tensor_vs_float64 at the wide widths: max_grad_norm < 0, each of the 13 tensors
    against ppo_loss() in float64 autograd, a "mixed" and a "first-epoch" minibatch; max |got - ref| <= 2e-5 max |ref
    tensor| + 1e-6 max |ref|, stats[0] / stats[1] to 1e-5."""
    n = max(2 * B, 300) + 17
    bt = LS.SoloBatch(g, D, n, seed=1000 + 7 * D + B)
    segs = R.segments(bt.pol)
    for mode, ent in (("mixed", 0.01), ("first", 0.0)):
        cfg = g.PPOConfig(ent_coef=ent, max_grad_norm=-1.0, clip_range=0.2)
        bt.set_old_logp(mode, cfg.clip_range)
        idx = torch.randperm(n, device=DEV)[:B].contiguous()
        fu = g.FusedUpdate(bt.pol, cfg, bt.obs, bt.act, bt.old_logp, bt.adv, bt.ret)
        assert fu.entry == ENTRY
        theta = R.flat_params(bt.pol)
        fu.step(idx)
        torch.cuda.synchronize()
        got = fu.grad.double().cpu().numpy()
        got[-1] -= ent                                    # (the entropy term is added by the apply launch)
        obs, act, old, adv, ret = bt.host(idx)
        ref, pg, vf, ratio = R.grad64(bt.ac_cls, cfg, D, theta, obs, act, old, adv, ret)
        a = adv - adv.mean()
        if mode == "mixed" and B >= 63:                   # the mix actually occurs
            for lo_hi in (ratio < 0.8, ratio > 1.2):
                assert (lo_hi & (a > 0)).sum() >= 1 and (lo_hi & (a < 0)).sum() >= 1, (B, ratio.min(), ratio.max())
            assert ((ratio > 0.8) & (ratio < 1.2)).sum() >= 1
        if mode == "first":
            assert np.abs(ratio - 1).max() < 1e-5
        assert np.array_equal(fu.step_count.cpu().numpy(), [0])      # nothing applied
        assert np.array_equal(R.flat_params(bt.pol), theta)
        LS.assert_per_tensor("wide raw gradient D=%d B=%d %s" % (D, B, mode), got, ref, segs, LS.TAU)
        st = fu.stats.double().cpu().numpy()
        print("  pg %.3e vs %.3e, vf %.3e vs %.3e" % (st[0], pg, st[1], vf))
        assert abs(st[0] - pg) <= 1e-5 * max(1.0, abs(pg)) and abs(st[1] - vf) <= 1e-5 * max(1.0, vf)


@pytest.mark.gpu
@pytest.mark.parametrize("D,B", CASES, ids=_IDS)
def test_wide_update_applied_steps_vs_float64(g, gpu, D, B):
    """test_fused_update_applied_steps_vs_float64 at the wide widths: the clip active (0.5) and inactive (1e6), a step
    count of 9 999 with non-zero moments, two steps each, every reference step from the kernel's own state.  Bounds: m
    2e-5, v 5e-5, parameters one float32 ulp + 1e-2 lr, norm / pg / vf 1e-5, `grad` exactly zero, step count + 1.
    "The step was taken" (median |step| / lr > 0.05) is asked of the REFERENCE's step and for B >= 63: at B = 2 both rows
    can clip, the actor's gradient is then exactly zero and the reference itself does not move half the parameters; the
    per-entry parameter bound holds the kernel to the reference's step either way."""
    n = max(2 * B, 300) + 17
    bt = LS.SoloBatch(g, D, n, seed=2000 + 7 * D + B)
    segs = R.segments(bt.pol)
    lr, b1, b2, eps = 3e-4, 0.9, 0.999, 1e-5
    worst = {"param": 0.0, "m": 0.0, "v": 0.0, "norm": 0.0, "pg": 0.0, "vf": 0.0}
    for max_norm, ent, start in ((0.5, 0.01, 0), (1e6, 0.0, 0), (0.5, 0.0, 9999)):
        cfg = g.PPOConfig(ent_coef=ent, max_grad_norm=max_norm, learning_rate=lr, clip_range=0.2)
        bt.set_old_logp("mixed", cfg.clip_range)
        fu = g.FusedUpdate(bt.pol, cfg, bt.obs, bt.act, bt.old_logp, bt.adv, bt.ret)
        assert fu.entry == ENTRY
        if start:
            fu.step_count.fill_(start)
            rng = np.random.default_rng(B)
            m_pre = rng.normal(0, 1e-2, fu.m.numel())               # moments as a long run leaves them: v >= m^2
            fu.m.copy_(torch.as_tensor(m_pre.astype(np.float32), device=DEV))
            fu.v.copy_(torch.as_tensor((m_pre ** 2 * rng.uniform(1, 4, m_pre.size) + 1e-8).astype(np.float32), device=DEV))
        for k in range(2):
            bt.nudge_off_edges(cfg.clip_range)
            idx = torch.randperm(n, device=DEV)[:B].contiguous()
            theta0 = R.flat_params(bt.pol)
            m0, v0 = fu.m.double().cpu().numpy(), fu.v.double().cpu().numpy()
            s0 = int(fu.step_count.item())
            obs, act, old, adv, ret = bt.host(idx)
            grad, pg, vf, _ = R.grad64(bt.ac_cls, cfg, D, theta0, obs, act, old, adv, ret)
            theta_ref, m_ref, v_ref, norm = R.adam64(theta0, grad, m0, v0, s0, max_norm, lr, b1, b2, eps)
            assert (norm > max_norm) == (max_norm < 1.0), (norm, max_norm)     # active / inactive as meant
            fu.step(idx)
            torch.cuda.synchronize()
            what = "D=%d B=%d max_norm=%g ent=%g step %d" % (D, B, max_norm, ent, s0 + 1)
            assert int(fu.step_count.item()) == s0 + 1, what
            assert float(fu.grad.abs().max()) == 0.0, what
            st = fu.stats.double().cpu().numpy()
            assert st[0] == 0.0 and st[1] == 0.0, what
            for key, got_, ref_, tol in (("norm", st[2], norm, 1e-5 * norm), ("pg", st[4], pg, 1e-5 * max(1.0, abs(pg))),
                                         ("vf", st[5], vf, 1e-5 * max(1.0, vf))):
                worst[key] = max(worst[key], abs(got_ - ref_) / tol * 1.0)
                assert abs(got_ - ref_) <= tol, (what, key, got_, ref_)
            m1, v1 = fu.m.double().cpu().numpy(), fu.v.double().cpu().numpy()
            worst["m"] = max(worst["m"], LS.assert_per_tensor("m " + what, m1, m_ref, segs, LS.TAU_M))
            worst["v"] = max(worst["v"], LS.assert_per_tensor("v " + what, v1, v_ref, segs, LS.TAU_V))
            theta1 = R.flat_params(bt.pol)
            ulp = np.spacing(np.abs(theta_ref).astype(np.float32)).astype(np.float64)
            excess = (np.abs(theta1 - theta_ref) - ulp) / lr
            worst["param"] = max(worst["param"], float(excess.max()))
            assert excess.max() <= 1e-2, (what, float(excess.max()), int(excess.argmax()))
            if B >= 63:
                assert np.median(np.abs(theta_ref - theta0) / lr) > 0.05, what    # the reference's step is a real one
    print("wide applied steps D=%d B=%d: worst param excess %.2e lr (bound 1e-2), m tau %.2e (bound %.0e), v tau %.2e (bound "
          "%.0e), norm / pg / vf at %.2f / %.2f / %.2f of their 1e-5 bounds"
          % (D, B, worst["param"], worst["m"], LS.TAU_M, worst["v"], LS.TAU_V, worst["norm"], worst["pg"], worst["vf"]))


@pytest.mark.gpu
@pytest.mark.parametrize("D,n,B", ((53, 6000, 2085), (197, 3000, 1000), (101, 700, 64)))
def test_wide_update_against_torch_autograd_and_adam(g, gpu, D, n, B):
    """test_ppo.py's test_fused_update_against_torch_autograd_and_adam at the wide widths, its bounds: the torch path the
    trainer otherwise runs (ppo_loss(), autograd, clip_grad_norm_, torch.optim.Adam(eps = 1e-5)) on the same minibatch --
    the raw gradient, then the loss values, the gradient norm and the parameters after one and after three updates."""
    import dataclasses
    torch.manual_seed(11)
    cfg = g.PPOConfig(ent_coef=0.01, max_grad_norm=0.5, learning_rate=3e-4)
    mine = LS.actor_critic(g, D, 5)
    ref = g.ActorCritic(D).to(DEV)
    ref.load_state_dict(mine.state_dict())
    obs = torch.rand(n, D, device=DEV) * 2 - 1
    act = torch.randn(n, device=DEV) * 0.7
    adv, ret = torch.randn(n, device=DEV) * 2, torch.randn(n, device=DEV)
    with torch.no_grad():
        mean, _ = ref.forward(obs)
        old_logp = g.ppo._normal_logp(mean, ref.log_std, act.unsqueeze(-1)) + torch.randn(n, device=DEV) * 0.25
    probe = g.FusedUpdate(mine, dataclasses.replace(cfg, max_grad_norm=-1.0), obs, act, old_logp, adv, ret)
    assert probe.entry == ENTRY
    idx0 = torch.randperm(n, device=DEV)[:B].contiguous()
    probe.step(idx0)
    loss0, _, _ = g.ppo_loss(ref, cfg, obs[idx0], act[idx0].unsqueeze(-1), old_logp[idx0], adv[idx0], ret[idx0])
    loss0.backward()
    want = torch.cat([ref.get_parameter(name).grad.reshape(-1) for name in R.PARAM_NAMES])
    got = probe.grad.clone()
    got[-1] -= cfg.ent_coef                                    # (the entropy term is added by the apply launch)
    err = float((got - want).abs().max()) / float(want.abs().max())
    cos = float(torch.dot(got, want) / (got.norm() * want.norm()))
    print("wide PPO gradient vs autograd (D = %d, B = %d): max |diff| / max |g| = %.2e, cosine %.8f, norms %.6g %.6g"
          % (D, B, err, cos, float(got.norm()), float(want.norm())))
    assert err < 2e-4 and cos > 0.999999
    ref.zero_grad(set_to_none=True)
    fu = g.FusedUpdate(mine, cfg, obs, act, old_logp, adv, ret)
    opt = torch.optim.Adam(ref.parameters(), lr=cfg.learning_rate, eps=1e-5)
    for k in range(3):
        idx = torch.randperm(n, device=DEV)[:B].contiguous()
        loss, pg, vf = g.ppo_loss(ref, cfg, obs[idx], act[idx].unsqueeze(-1), old_logp[idx], adv[idx], ret[idx])
        opt.zero_grad(set_to_none=True)
        loss.backward()
        norm = float(torch.nn.utils.clip_grad_norm_(ref.parameters(), cfg.max_grad_norm))
        opt.step()
        fu.step(idx)
        torch.cuda.synchronize()
        st = fu.last_losses()
        assert abs(st["pg_loss"] - float(pg.detach())) < 2e-5 * max(1.0, abs(float(pg.detach()))) + 2e-6, (k, st, float(pg.detach()))
        assert abs(st["value_loss"] - float(vf.detach())) < 1e-4 * float(vf.detach()), (k, st, float(vf.detach()))
        assert abs(st["grad_norm"] - norm) < 2e-4 * norm, (k, st["grad_norm"], norm)
        for (name, p), q in zip(mine.named_parameters(), ref.parameters()):
            d = float((p - q).abs().max())
            assert d < 0.02 * cfg.learning_rate, (k, name, d)        # an Adam step moves a parameter by ~lr
    assert int(fu.step_count) == 3 and float(fu.grad.abs().max()) == 0.0


@pytest.mark.gpu
def test_wide_update_writes_nothing_outside_its_workspace(g, gpu):
    """D = 197, B = 65 (a second workgroup with one live row): grad / m / v are the middle of larger tensors filled with
    a sentinel; after a probe and two applied steps every sentinel is intact, and so is every buffer the kernel reads."""
    D, B, pad, sent = 197, 65, 4096, -7.25
    n = max(2 * B, 300) + 17
    bt = LS.SoloBatch(g, D, n, seed=5)
    bt.set_old_logp("mixed", 0.2)
    reads = [t.clone() for t in (bt.obs, bt.act, bt.old_logp, bt.adv, bt.ret)]
    for max_norm, steps in ((-1.0, 1), (0.5, 2)):
        fu = g.FusedUpdate(bt.pol, g.PPOConfig(max_grad_norm=max_norm), bt.obs, bt.act, bt.old_logp, bt.adv, bt.ret)
        k = fu.grad.numel()
        big = [torch.full((k + 2 * pad,), sent, dtype=torch.float32, device=DEV) for _ in range(3)]
        for t in big:
            t[pad:pad + k].zero_()
        fu.grad, fu.m, fu.v = (t[pad:pad + k] for t in big)
        for _ in range(steps):
            idx = torch.randperm(n, device=DEV)[:B].contiguous()
            keep = idx.clone()
            fu.step(idx)
            torch.cuda.synchronize()
            assert torch.equal(idx, keep)
        for name, t in zip(("grad", "m", "v"), big):
            assert bool((t[:pad] == sent).all()) and bool((t[pad + k:] == sent).all()), (max_norm, name)
        assert float(fu.grad.abs().max()) > 0.0 if max_norm < 0 else float(fu.m.abs().max()) > 0.0      # it did run
    for t, q in zip((bt.obs, bt.act, bt.old_logp, bt.adv, bt.ret), reads):
        assert torch.equal(t, q)


@pytest.mark.gpu
@pytest.mark.parametrize("N,iters", ((16, 3), (64, 1)))
def test_trainer_trains_with_the_fused_update_at_wide_widths(g, gpu, N, iters):
    """256 envs x N traffic, collector="fused", updater="fused", n_steps 32, batch 1000, 2 epochs: 8 192 rows, so an epoch
    is eight whole minibatches and a tail of 192 rows.  Every logged loss is finite, the Adam step count is iterations x
    epochs x 9, the parameters moved, evaluate() runs.  (No learning-curve threshold: nothing says how fast PPO improves
    at these traffic counts.)"""
    import random
    venv = g.ACAS2DVecEnv(256, N, device=DEV, dtype=torch.float32, seed=13)
    tr = g.PPOTrainer(venv, g.PPOConfig(n_steps=32, batch_size=1000, n_epochs=2, seed=13), collector="fused", updater="fused")
    before = R.flat_params(tr.policy)
    assert tr.optimizer_state()["step"] == 0
    hist = tr.learn(iters * 256 * 32, log=None)
    assert len(hist) == iters
    for rec in hist:
        assert all(np.isfinite(rec[k]) for k in ("pg_loss", "value_loss", "std")), rec
    state = tr.optimizer_state()
    assert tr._fused_update.entry == ENTRY and state["updater"] == "fused"
    assert state["step"] == iters * 2 * 9
    assert state["exp_avg"].numel() == state["exp_avg_sq"].numel() == R.segments(tr.policy)[-1][2]
    after = R.flat_params(tr.policy)
    assert np.isfinite(after).all() and np.abs(after - before).max() > 1e-4
    out = tr.evaluate(10, random.Random(7))
    assert out["total_reward"].shape == (10,) and np.isfinite(out["total_reward"]).all() and (out["outcome"] != 0).all()
