"""The PPO update kernels -- acas2d_ppo_update_f32 (narrow), acas2d_ppo_update_wide_f32 (wide), acas2d_ppo_update_set_f32
(set), acas2d_ppo_update_wide_set_f32 (wide set), which share the body of csrc/acas2d_ppo.hpp -- against float64 on the hand-placed edge minibatches of
tests/edge_minibatches.py (admitted on the CPU by tests/test_edge_minibatches.py: plain float32 autograd clears a quarter
of every bound used here), through FusedUpdate and FusedUpdateSet:

  a  every case x family (narrow D = 8, 29; wide D = 53, 197; set D = 8, 29 and wide set D = 53, 197 with K = 3 members of
     their own policy, clip_range and vf_coef; `entry` is asserted) x B in (2, 65, 130): the raw gradient per tensor and one applied step from the kernel's own
     state; const_adv gives an exactly zero actor gradient and keeps every actor bit
  b  B = 8 193 (above anything a trainer here asks for): grid_adv and "mixed", D = 8 and 197, raw gradient
  c  Adam constants other than 0.9 / 0.999 / 1e-5, per member in the set, and a step count of 10 000 000
  d  set members that share rows: identical members stay bit-equal; overlapping minibatches each meet float64
  e  sentinels around every buffer the narrow and the set update write
  f  a rollout buffer of more than 2^31 floats (D = 29, D = 197)
Criteria and bounds are learner_support.py's (TAU, TAU0, TAU_M, TAU_V, parameter excess 1e-2 lr, losses 1e-5),
unchanged; every test prints what it observed.

Observed on an MI355X (one run of this file: 161 passed in 8.7 s, 209 in 13.7 s with the wide set cases; the slowest test 0.39 s -- the first, which loads
the library -- every other under 0.1 s; the two 8.6 GB cases ran, 0.07 s each).  No case exposed a fault in the kernels.
Worst per-tensor tau over D and B, raw gradient / m / v (bounds 2e-5 / 2e-5 / 5e-5; negative: within the 1e-6 max |ref|
term alone), and worst parameter excess in lr (bound 1e-2):

  case          narrow                               wide                                 set (worst member)
  saturated      1.3e-7 /  1.5e-7 / 1.21e-5, 2.0e-4   4.3e-7 /  5.1e-7 / 1.28e-5, 8.1e-4   7.9e-7 /  8.6e-7 / 1.22e-5, 1.6e-4
  wide_obs       9.2e-8 / -4.2e-7 / 1.33e-5, 9.6e-4   3.0e-6 /  2.6e-6 / 1.51e-5, 2.5e-3   6.2e-7 /  6.2e-7 / 1.27e-5, 2.4e-3
  grid_adv      -6.8e-7 / -6.1e-7 / 1.20e-5, 5.4e-5  -9.3e-7 / -6.3e-7 / 1.21e-5, 1.8e-4  -7.0e-7 / -5.2e-7 / 1.21e-5, 8.2e-5
  const_adv     -8.1e-7 / -6.6e-7 / 1.19e-5, 2.6e-5  -7.5e-7 / -6.8e-7 / 1.21e-5, 1.5e-4  -8.9e-7 / -5.9e-7 / 1.22e-5, 1.2e-4
  log_std-2.5   -3.7e-7 / -1.9e-7 / 1.23e-5, 2.0e-4   1.3e-7 / -9.1e-8 / 1.24e-5, 3.0e-4   3.0e-7 / -2.4e-7 / 1.31e-5, 2.9e-4
  log_std+1.0   -8.3e-7 / -6.2e-7 / 1.21e-5, 5.7e-5  -6.6e-7 / -6.7e-7 / 1.21e-5, 1.4e-4  -8.4e-7 / -6.1e-7 / 1.20e-5, 5.5e-5
  dup_rows      -3.2e-7 / -2.5e-7 / 1.26e-5, 5.6e-4  -1.3e-7 / -1.5e-7 / 1.30e-5, 1.7e-4  -3.0e-7 / -1.4e-7 / 1.31e-5, 3.9e-4
  underflow     -9.4e-7 / -6.5e-7 / 1.20e-5, 3.4e-5  -7.6e-7 / -5.8e-7 / 1.21e-5, 1.7e-4  -6.9e-7 / -5.7e-7 / 1.24e-5, 7.0e-5

The set update at D = 53, 197 (acas2d_ppo_update_wide_set_f32; worst member, the same four figures):

  case          wide set
  saturated      2.6e-6 /  2.6e-6 / 1.22e-5, 1.4e-3
  wide_obs       2.8e-7 /  4.8e-8 / 1.34e-5, 2.3e-3
  grid_adv      -4.5e-7 / -4.6e-7 / 1.23e-5, 1.7e-4
  const_adv     -6.5e-7 / -5.8e-7 / 1.21e-5, 1.8e-4
  log_std-2.5    4.6e-7 /  5.1e-7 / 1.30e-5, 4.8e-4
  log_std+1.0   -5.8e-7 / -6.1e-7 / 1.22e-5, 1.6e-4
  dup_rows       1.7e-7 / -1.3e-7 / 1.32e-5, 2.1e-4
  underflow      1.6e-7 /  5.9e-8 / 1.27e-5, 1.7e-4

(v sits at 1.2e-5 everywhere: the float32 0.999, as in test_learner_kernels.py.)  The worst raw gradient is wide_obs at
D = 197, B = 65, 3.0e-6 -- the case float32 torch autograd itself clears by least on the CPU (3.3e-6).  const_adv: actor
tensors, log_std entry and pg exactly 0 in all 24 runs, every actor bit kept by the applied step.  B = 8 193: tau -8.0e-7
(grid_adv) and -8.1e-7 (mixed) at worst.  Adam constants: (0.5, 0.9, 1e-3) m -8.5e-7, v -5.1e-7 (bound 3.7e-5), excess
1.1e-6 lr; (0.8, 0.99, 1e-4) v 4.0e-8, excess 2.3e-6 lr; the defaults v 1.19e-5, excess 3.5e-5 lr -- the steps from
10 000 000 included.  Shared rows: bit-equal in all four cases; overlapping rows and the rows past 2^31 floats -7.9e-7 at
worst.  With one line of a kernel changed this file fails (each run once): the narrow statistics loop stopping at B - 1,
103 tests (every narrow and set case, const_adv included, D = 8 at B = 8 193, the D = 8 Adam tests, the overlapping
rows, the narrow 2^31 case); the wide dW1 column
guard at c < D - 1, 52 (every wide case, D = 53 Adam, D = 197 at B = 8 193 and past 2^31); the set apply kernel taking
member 0's `m` for every member, 53 (every set case, the per-member Adam test, the four bit-equality cases).
"""

import numpy as np
import pytest

import edge_minibatches as E
import learner_ref as R
import learner_support as LS

torch = pytest.importorskip("torch")
DEV = "cuda:0"
LR = LS.LR


@pytest.fixture(scope="module")
def g():
    import gym_acas2d_amd as g
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    g.native.lib()
    return g


# ---- a. every case, raw gradient and one applied step -------------------------------------------------------------------
SOLO_CASES = [(D, B, case) for D in (8, 29, 53, 197) for B in (2, 65, 130) for case in E.CASES]
SET_CASES = [(D, B, case) for D in (8, 29, 53, 197) for B in (2, 65, 130) for case in E.CASES]
_ID = lambda c: "D%d-B%d-%s" % c  # noqa: E731


@pytest.mark.gpu
@pytest.mark.parametrize("D,B,case", SOLO_CASES, ids=[_ID(c) for c in SOLO_CASES])
def test_solo_update_on_edge_minibatches_vs_float64(g, D, B, case):
    """Narrow (D = 8, 29) and wide (D = 53, 197).  Raw gradient (max_grad_norm < 0, ent_coef 0.01): each of the 13 tensors
    within TAU max |ref tensor| + TAU0 max |ref|, stats[0..1] to 1e-5.  Then one applied step (max_grad_norm 0.5, lr 3e-4)
    against grad64 + adam64 from the kernel's own state.  const_adv: the 6 actor tensors of `grad` and the log_std entry
    are exactly 0, everything is finite, and with ent_coef = 0 the applied step keeps every actor bit while the critic
    moves."""
    bt = LS.edge_batch("solo", D, B, case)
    bufs, idx = LS.device_bufs(bt), LS.dev(bt.idx[0])
    pol = LS.device_policy(g, bt)
    segs = R.segments(pol)
    na = LS.n_actor(segs)
    theta0 = bt.theta()
    what = "%s %s D=%d B=%d" % ("narrow" if D < 53 else "wide", case, D, B)

    cfg = g.PPOConfig(ent_coef=0.01, max_grad_norm=-1.0, clip_range=0.2)
    fu = g.FusedUpdate(pol, cfg, *bufs)
    assert fu.entry == ("acas2d_ppo_update_f32" if D < 53 else "acas2d_ppo_update_wide_f32")
    fu.step(idx)
    torch.cuda.synchronize()
    raw = fu.grad.double().cpu().numpy()
    got = raw.copy()
    got[-1] -= cfg.ent_coef                                  # (the entropy term is added by the apply launch)
    ref, pg, vf, _ = R.grad64(bt.ac_cls, cfg, D, theta0, *bt.rows())
    assert np.isfinite(raw).all() and np.array_equal(R.flat_params(pol), theta0)
    assert np.array_equal(fu.step_count.cpu().numpy(), [0])
    LS.assert_per_tensor("raw gradient " + what, got, ref, segs, LS.TAU)
    st = fu.stats.double().cpu().numpy()
    LS.check_losses(what, st[0], st[1], pg, vf)
    if case == "const_adv":
        assert not raw[:na].any() and raw[-1] == 0.0 and st[0] == 0.0, (np.abs(raw[:na]).max(), raw[-1], st[0])
        assert np.abs(raw[na:-1]).max() > 0.0

    ent = 0.0 if case == "const_adv" else 0.01
    cfg = g.PPOConfig(ent_coef=ent, max_grad_norm=0.5, learning_rate=LR, clip_range=0.2)
    fu = g.FusedUpdate(pol, cfg, *bufs)
    grad, pg, vf, _ = R.grad64(bt.ac_cls, cfg, D, theta0, *bt.rows())
    theta_ref, m_ref, v_ref, norm = R.adam64(theta0, grad, np.zeros_like(grad), np.zeros_like(grad), 0, 0.5, LR, 0.9, 0.999, 1e-5)
    fu.step(idx)
    torch.cuda.synchronize()
    st = fu.stats.double().cpu().numpy()
    theta1, m1, v1 = R.flat_params(pol), fu.m.double().cpu().numpy(), fu.v.double().cpu().numpy()
    assert int(fu.step_count.item()) == 1 and float(fu.grad.abs().max()) == 0.0 and st[0] == 0.0 and st[1] == 0.0
    assert np.isfinite(theta1).all() and np.isfinite(m1).all() and np.isfinite(v1).all() and np.isfinite(st).all()
    assert abs(st[2] - norm) <= 1e-5 * norm, (what, st[2], norm)
    LS.check_losses(what + " applied", st[4], st[5], pg, vf)
    LS.check_applied(what, segs, theta1, m1, v1, theta_ref, m_ref, v_ref, LR)
    if case == "const_adv":
        assert np.array_equal(theta1[:na], theta0[:na]) and theta1[-1] == theta0[-1]           # every actor bit kept
        assert not m1[:na].any() and not v1[:na].any() and m1[-1] == 0.0 and v1[-1] == 0.0
        assert np.median(np.abs(theta1[na:-1] - theta0[na:-1]) / LR) > 0.05                     # the critic moved


def _set_update(g, bt, cfgs, pols=None):
    pset = g.ActorCriticSet.from_members([LS.device_policy(g, bt, k) for k in range(bt.K)] if pols is None else pols)
    return pset, g.FusedUpdateSet(pset, cfgs, *LS.device_bufs(bt))


@pytest.mark.gpu
@pytest.mark.parametrize("D,B,case", SET_CASES, ids=[_ID(c) for c in SET_CASES])
def test_set_update_on_edge_minibatches_vs_float64(g, D, B, case):
    """The solo test for K = 3 members with their own policy, clip_range 0.1 / 0.2 / 0.3 and vf_coef 0.5 / 0.25 / 1.0 on
    disjoint rows of one buffer: apply=False for the raw gradients, then one applied step of a fresh FusedUpdateSet.
    D = 8, 29 take acas2d_ppo_update_set_f32, D = 53, 197 acas2d_ppo_update_wide_set_f32 (asserted on fu.entry)."""
    bt = LS.edge_batch("set", D, B, case)
    idx = LS.dev(bt.idx)
    segs = R.segments(bt.pols[0])
    na = LS.n_actor(segs)
    theta0 = [bt.theta(k) for k in range(bt.K)]

    def cfgs(ent, max_norm):
        return [g.PPOConfig(ent_coef=ent, clip_range=bt.clips[k], vf_coef=E.VF_COEFS[k], max_grad_norm=max_norm, learning_rate=LR)
                for k in range(bt.K)]

    cf = cfgs(0.01, 0.5)
    pset, fu = _set_update(g, bt, cf)
    assert fu.entry == ("acas2d_ppo_update_set_f32" if D < 53 else "acas2d_ppo_update_wide_set_f32")
    fu.step(idx, apply=False)
    torch.cuda.synchronize()
    assert fu.step_count.cpu().tolist() == [0] * bt.K and float(fu.m.abs().max()) == 0.0 and float(fu.v.abs().max()) == 0.0
    for k in range(bt.K):
        what = "set %s D=%d B=%d member %d" % (case, D, B, k)
        assert np.array_equal(LS.theta_of(pset, k), theta0[k]), what
        raw = fu.grad[k].double().cpu().numpy()
        got = raw.copy()
        got[-1] -= 0.01
        ref, pg, vf, _ = R.grad64(bt.ac_cls, cf[k], D, theta0[k], *bt.rows(k))
        assert np.isfinite(raw).all()
        LS.assert_per_tensor("raw gradient " + what, got, ref, segs, LS.TAU)
        st = fu.stats[k].double().cpu().numpy()
        LS.check_losses(what, st[0], st[1], pg, vf)
        if case == "const_adv":
            assert not raw[:na].any() and raw[-1] == 0.0 and st[0] == 0.0, what
            assert np.abs(raw[na:-1]).max() > 0.0

    cf = cfgs(0.0 if case == "const_adv" else 0.01, 0.5)
    pset, fu = _set_update(g, bt, cf)
    fu.step(idx)
    torch.cuda.synchronize()
    assert fu.step_count.cpu().tolist() == [1] * bt.K and float(fu.grad.abs().max()) == 0.0
    assert float(fu.stats[:, 0:2].abs().max()) == 0.0 and bool(torch.isfinite(fu.stats).all())
    for k in range(bt.K):
        what = "set %s D=%d B=%d member %d" % (case, D, B, k)
        grad, pg, vf, _ = R.grad64(bt.ac_cls, cf[k], D, theta0[k], *bt.rows(k))
        theta_ref, m_ref, v_ref, norm = R.adam64(theta0[k], grad, np.zeros_like(grad), np.zeros_like(grad), 0, 0.5, LR, 0.9, 0.999, 1e-5)
        st = fu.stats[k].double().cpu().numpy()
        theta1, m1, v1 = LS.theta_of(pset, k), fu.m[k].double().cpu().numpy(), fu.v[k].double().cpu().numpy()
        assert np.isfinite(theta1).all() and np.isfinite(m1).all() and np.isfinite(v1).all()
        assert abs(st[2] - norm) <= 1e-5 * norm, (what, st[2], norm)
        LS.check_losses(what + " applied", st[4], st[5], pg, vf)
        LS.check_applied(what, segs, theta1, m1, v1, theta_ref, m_ref, v_ref, LR)
        if case == "const_adv":
            assert np.array_equal(theta1[:na], theta0[k][:na]) and theta1[-1] == theta0[k][-1], what
            assert not m1[:na].any() and not v1[:na].any() and m1[-1] == 0.0 and v1[-1] == 0.0, what
            assert np.median(np.abs(theta1[na:-1] - theta0[k][na:-1]) / LR) > 0.05, what


# ---- b. large B ------------------------------------------------------------------------------------------------------
LARGE = [(D, 8193, case) for D in (8, 197) for case in ("grid_adv", "mixed")]


@pytest.mark.gpu
@pytest.mark.parametrize("D,B,case", LARGE, ids=[_ID(c) for c in LARGE])
def test_update_raw_gradient_at_8193_rows_vs_float64(g, D, B, case):
    """B = 8 193: 129 workgroups per network, the last with one live row; the advantage statistics loops run 129 (narrow)
    and 33 (wide) times per lane.  grid_adv (c = 64, q <= 1 / 8: exact sums) and a "mixed" minibatch, raw gradient."""
    bt = LS.edge_batch("solo", D, B, case)
    pol = LS.device_policy(g, bt)
    cfg = g.PPOConfig(ent_coef=0.01, max_grad_norm=-1.0, clip_range=0.2)
    fu = g.FusedUpdate(pol, cfg, *LS.device_bufs(bt))
    fu.step(LS.dev(bt.idx[0]))
    torch.cuda.synchronize()
    got = fu.grad.double().cpu().numpy()
    got[-1] -= cfg.ent_coef
    ref, pg, vf, _ = R.grad64(bt.ac_cls, cfg, D, bt.theta(), *bt.rows())
    what = "%s D=%d B=%d" % (case, D, B)
    LS.assert_per_tensor("raw gradient " + what, got, ref, R.segments(pol), LS.TAU)
    st = fu.stats.double().cpu().numpy()
    LS.check_losses(what, st[0], st[1], pg, vf)


# ---- c. Adam constants -------------------------------------------------------------------------------------------------
def _tau_v(beta2):
    """TAU_V with its allowance for the float32 beta2 recomputed: the kernel's 1 - beta2 is |beta2_f32 - beta2| /
    (1 - beta2) relative off the reference's (1.3e-5 at 0.999, the figure TAU_V = 5e-5 was set with)."""
    term = lambda b: abs(float(np.float32(b)) - b) / (1.0 - b)  # noqa: E731
    return LS.TAU_V + (term(beta2) - term(0.999))


def _moments(rng, n):
    m = rng.normal(0, 1e-2, n)                              # moments as a long run leaves them: v >= m^2
    return m.astype(np.float32), (m ** 2 * rng.uniform(1, 4, n) + 1e-8).astype(np.float32)


ADAM_STARTS = ((0, 2, False), (9999, 2, True), (10_000_000, 1, True))       # step count, steps taken, non-zero moments


@pytest.mark.gpu
@pytest.mark.parametrize("D", (8, 53))
def test_solo_update_with_other_adam_constants_vs_float64(g, D):
    """FusedUpdate(beta1=0.5, beta2=0.9, adam_eps=1e-3): two steps from step count 0, two from 9 999 with non-zero moments,
    one from 10 000 000 (both bias corrections are exactly 1 in float32), each against adam64 from the kernel's own
    state.  Bounds of test_fused_update_applied_steps_vs_float64, TAU_V's float32-beta2 term recomputed for 0.9."""
    B, b1, b2, eps = 130, 0.5, 0.9, 1e-3
    bt = LS.edge_batch("solo", D, B, "mixed")
    bufs = LS.device_bufs(bt)
    pol = LS.device_policy(g, bt)
    segs = R.segments(pol)
    cfg = g.PPOConfig(ent_coef=0.01, max_grad_norm=0.5, learning_rate=LR, clip_range=0.2)
    rng = np.random.default_rng(D)
    tau_v = _tau_v(b2)
    assert tau_v <= LS.TAU_V
    for start, steps, moments in ADAM_STARTS:
        fu = g.FusedUpdate(pol, cfg, *bufs, beta1=b1, beta2=b2, adam_eps=eps)
        fu.step_count.fill_(start)
        if moments:
            m_pre, v_pre = _moments(rng, fu.m.numel())
            fu.m.copy_(LS.dev(m_pre))
            fu.v.copy_(LS.dev(v_pre))
        for s in range(steps):
            # (rows 0 .. B - 1 of a fresh permutation: old_logp is "mixed" on every row; a ratio that an applied step has
            # moved onto a clip edge is moved off it as RolloutBatch.nudge_off_edges does)
            rows = rng.permutation(bt.n)[:B]
            theta0 = R.flat_params(pol)
            lp = R.logp64(bt.ac_cls, D, theta0, bt.obs[rows], bt.act[rows])
            old, _ = E.nudge_off_edges(lp, bt.old_logp[rows].astype(np.float64), cfg.clip_range)
            bufs[2][LS.dev(rows)] = LS.dev(old)
            m0, v0 = fu.m.double().cpu().numpy(), fu.v.double().cpu().numpy()
            mb = [a.astype(np.float64)[rows] for a in (bt.obs, bt.act)] + [old.astype(np.float64)] + \
                 [a.astype(np.float64)[rows] for a in (bt.adv, bt.ret)]
            grad, pg, vf, _ = R.grad64(bt.ac_cls, cfg, D, theta0, *mb)
            theta_ref, m_ref, v_ref, norm = R.adam64(theta0, grad, m0, v0, start + s, 0.5, LR, b1, b2, eps)
            fu.step(LS.dev(rows))
            torch.cuda.synchronize()
            what = "adam (%g, %g, %g) D=%d step %d" % (b1, b2, eps, D, start + s + 1)
            assert int(fu.step_count.item()) == start + s + 1, what
            st = fu.stats.double().cpu().numpy()
            assert abs(st[2] - norm) <= 1e-5 * norm, (what, st[2], norm)
            LS.check_applied(what, segs, R.flat_params(pol), fu.m.double().cpu().numpy(), fu.v.double().cpu().numpy(),
                             theta_ref, m_ref, v_ref, LR, tau_v)
            assert np.median(np.abs(theta_ref - theta0) / LR) > 0.05, what           # the reference's step is a real one
    assert start == 10_000_000 and np.float32(b1) ** np.float32(start + 1) == 0.0 and np.float32(b2) ** np.float32(start + 1) == 0.0


@pytest.mark.gpu
def test_set_update_with_adam_constants_per_member_vs_float64(g):
    """D = 8, K = 3: hyper[k][5..7] written per member -- (0.5, 0.9, 1e-3), the defaults (0.9, 0.999, 1e-5), (0.8, 0.99,
    1e-4) -- the starts and step counts of the solo test on the member's own minibatch, every member against adam64 with ITS
    constants from the kernel's own state."""
    D, B = 8, 130
    consts = ((0.5, 0.9, 1e-3), (0.9, 0.999, 1e-5), (0.8, 0.99, 1e-4))
    bt = LS.edge_batch("set", D, B, "underflow")            # ("mixed" rows with a tenth of the ratios at 0)
    segs = R.segments(bt.pols[0])
    cfgs = [g.PPOConfig(ent_coef=0.01, clip_range=bt.clips[k], vf_coef=E.VF_COEFS[k], max_grad_norm=0.5, learning_rate=LR)
            for k in range(bt.K)]
    rng = np.random.default_rng(3)
    bufs, idx = LS.device_bufs(bt), LS.dev(bt.idx)
    old = bt.old_logp.copy()
    for start, steps, moments in ADAM_STARTS:
        pset = g.ActorCriticSet.from_members([LS.device_policy(g, bt, k) for k in range(bt.K)])
        fu = g.FusedUpdateSet(pset, cfgs, *bufs)
        fu.hyper[:, 5:8] = torch.tensor(consts, dtype=torch.float32, device=DEV)
        assert fu.hyper[1].cpu().tolist() == pytest.approx([0.2, 0.25, 0.01, 0.5, LR, 0.9, 0.999, 1e-5], rel=1e-6)
        fu.step_count.fill_(start)
        if moments:
            for k in range(bt.K):
                m_pre, v_pre = _moments(rng, fu.m.shape[1])
                fu.m[k].copy_(LS.dev(m_pre))
                fu.v[k].copy_(LS.dev(v_pre))
        for s in range(steps):
            theta0 = [LS.theta_of(pset, k) for k in range(bt.K)]
            for k in range(bt.K):                           # (RolloutBatch.nudge_off_edges for the member's CURRENT parameters)
                i = bt.idx[k]
                lp = R.logp64(bt.ac_cls, D, theta0[k], bt.obs[i], bt.act[i])
                old[i], _ = E.nudge_off_edges(lp, old[i].astype(np.float64), bt.clips[k])
            bufs[2].copy_(LS.dev(old))
            m0, v0 = fu.m.double().cpu().numpy(), fu.v.double().cpu().numpy()
            fu.step(idx)
            torch.cuda.synchronize()
            assert fu.step_count.cpu().tolist() == [start + s + 1] * bt.K
            for k, (b1, b2, eps) in enumerate(consts):
                what = "adam (%g, %g, %g) set member %d step %d" % (b1, b2, eps, k, start + s + 1)
                i = bt.idx[k]
                mb = [a.astype(np.float64)[i] for a in (bt.obs, bt.act, old, bt.adv, bt.ret)]
                grad, pg, vf, _ = R.grad64(bt.ac_cls, cfgs[k], D, theta0[k], *mb)
                theta_ref, m_ref, v_ref, norm = R.adam64(theta0[k], grad, m0[k], v0[k], start + s, 0.5, LR, b1, b2, eps)
                assert abs(float(fu.stats[k, 2]) - norm) <= 1e-5 * norm, what
                tau_v = _tau_v(b2)
                assert tau_v <= LS.TAU_V
                LS.check_applied(what, segs, LS.theta_of(pset, k), fu.m[k].double().cpu().numpy(),
                                 fu.v[k].double().cpu().numpy(), theta_ref, m_ref, v_ref, LR, tau_v)


# ---- d. members that share rows ----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("D,B", [(D, B) for D in (8, 29) for B in (63, 64)])
def test_set_members_on_the_same_rows_stay_bit_equal(g, D, B):
    """K = 3 copies of one policy, the same hyper-row, the same idx (drawn with replacement: duplicates inside): with one
    wave per network every gradient entry gets one atomic, so grad[k], the 13 parameter stacks, m, v and stats are the
    same bits for every k -- after the raw gradient and after each of two applied steps."""
    bt = LS.edge_batch("solo", D, B, "dup_rows")
    assert bt.labels["distinct_rows"][0] < B
    cfg = g.PPOConfig(ent_coef=0.01, max_grad_norm=0.5, learning_rate=LR, clip_range=0.2)
    idx = LS.dev(np.stack([bt.idx[0]] * 3))

    def all_equal(fu, pset, what):
        tensors = [("grad", fu.grad), ("m", fu.m), ("v", fu.v), ("stats", fu.stats), ("step", fu.step_count)]
        tensors += [(n, pset.params[n]) for n in R.PARAM_NAMES]
        for name, t in tensors:
            assert bool(torch.isfinite(t.float()).all()), (what, name)
            for k in (1, 2):
                assert torch.equal(t[k], t[0]), (what, name, k)

    pset, fu = _set_update(g, bt, [cfg] * 3, pols=[LS.device_policy(g, bt)] * 3)
    fu.step(idx, apply=False)
    torch.cuda.synchronize()
    assert float(fu.grad[0].abs().max()) > 0.0
    all_equal(fu, pset, "raw gradient")
    before = LS.theta_of(pset, 2)
    pset, fu = _set_update(g, bt, [cfg] * 3, pols=[LS.device_policy(g, bt)] * 3)
    for step in range(2):
        fu.step(idx)
        torch.cuda.synchronize()
        all_equal(fu, pset, "applied step %d" % (step + 1))
    assert fu.step_count.cpu().tolist() == [2, 2, 2] and np.abs(LS.theta_of(pset, 2) - before).max() > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("D", (8, 29))
def test_set_members_on_overlapping_rows_vs_float64(g, D):
    """B = 130: members 0 and 2 hold different policies (member 2 is member 0 with every parameter scaled by 1 + N(0,
    0.1): a nearby policy, so its ratios on rows whose old_logp came from member 0 stay finite) and minibatches that share
    65 rows; member 1 is a copy of member 0 on rows of its own.  Raw gradient of each member against float64."""
    B = 130
    bt = LS.edge_batch("solo", D, B, "mixed")
    rng = np.random.default_rng(D)
    perm = rng.permutation(bt.n)
    rows = np.stack([perm[:B], perm[200:200 + B], perm[65:65 + B]])
    assert len(np.intersect1d(rows[0], rows[2])) == 65 and len(np.intersect1d(rows[0], rows[1])) == 0
    pols = [LS.device_policy(g, bt) for _ in range(3)]
    gen = torch.Generator().manual_seed(D)
    with torch.no_grad():
        for p in pols[2].parameters():
            p.mul_((1.0 + 0.1 * torch.randn(p.shape, generator=gen)).to(DEV))
    clips = (0.2, 0.2, 0.1)
    thetas = [R.flat_params(p) for p in pols]
    old = bt.old_logp.copy()
    for _ in range(8):                                      # a ratio of EITHER member within 1e-4 of its clip edge moves off
        moved = 0
        for k in (0, 2):
            lp = R.logp64(bt.ac_cls, D, thetas[k], bt.obs[rows[k]], bt.act[rows[k]])
            old[rows[k]], e = E.nudge_off_edges(lp, old[rows[k]].astype(np.float64), clips[k])
            moved += e
        if not moved:
            break
    assert not moved
    bufs = LS.device_bufs(bt)
    bufs[2] = LS.dev(old)
    cfgs = [g.PPOConfig(ent_coef=0.01, clip_range=clips[k], vf_coef=E.VF_COEFS[k], max_grad_norm=0.5) for k in range(3)]
    pset = g.ActorCriticSet.from_members(pols)
    fu = g.FusedUpdateSet(pset, cfgs, *bufs)
    fu.step(LS.dev(rows), apply=False)
    torch.cuda.synchronize()
    segs = R.segments(pols[0])
    grads = []
    for k in range(3):
        mb = [a.astype(np.float64)[rows[k]] for a in (bt.obs, bt.act, old, bt.adv, bt.ret)]
        ref, pg, vf, ratio = R.grad64(bt.ac_cls, cfgs[k], D, thetas[k], *mb)
        assert np.log(ratio).max() <= 3.0, (k, np.log(ratio).max())
        got = fu.grad[k].double().cpu().numpy()
        got[-1] -= 0.01
        LS.assert_per_tensor("overlapping rows D=%d member %d" % (D, k), got, ref, segs, LS.TAU)
        LS.check_losses("member %d" % k, float(fu.stats[k, 0]), float(fu.stats[k, 1]), pg, vf)
        grads.append(ref)
    assert np.abs(grads[0] - grads[2]).max() > 1e-3 * np.abs(grads[0]).max()          # the members really differ


# ---- e. guard bands ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_narrow_update_writes_nothing_outside_its_workspace(g):
    """test_wide_update_writes_nothing_outside_its_workspace for the narrow kernel: D = 29, B = 65 (a second workgroup
    with one live row); grad / m / v carved from sentinel-filled tensors, one probe and two applied steps."""
    D, B = 29, 65
    bt = LS.edge_batch("solo", D, B, "dup_rows")
    bufs, idx = LS.device_bufs(bt), LS.dev(bt.idx[0])
    reads = [t.clone() for t in bufs] + [idx.clone()]
    pol = LS.device_policy(g, bt)
    for max_norm, steps in ((-1.0, 1), (0.5, 2)):
        fu = g.FusedUpdate(pol, g.PPOConfig(max_grad_norm=max_norm), *bufs)
        k = fu.grad.numel()
        carved = [LS.carve((k,)) for _ in range(3)]
        fu.grad, fu.m, fu.v = (c[0] for c in carved)
        for _ in range(steps):
            fu.step(idx)
            torch.cuda.synchronize()
        for name, (_, big) in zip(("grad", "m", "v"), carved):
            LS.intact((max_norm, name), big, k)
        assert float(fu.grad.abs().max()) > 0.0 if max_norm < 0 else float(fu.m.abs().max()) > 0.0      # it did run
    for t, q in zip(bufs + [idx], reads):
        assert torch.equal(t, q)


@pytest.mark.gpu
def test_set_update_writes_nothing_outside_its_workspace(g):
    """D = 8, K = 3, B = 65: grad, m, v, stats, step_count and every one of the 13 [K][...] parameter stacks are the
    middle of sentinel-filled tensors (the kernels address grad + member * total, stats + member * 8, prm.p[k] + member *
    count).  After one probe and two applied steps every sentinel, every input buffer, idx and hyper are intact."""
    D, B = 8, 65
    bt = LS.edge_batch("set", D, B, "dup_rows")
    bufs, idx = LS.device_bufs(bt), LS.dev(bt.idx)
    reads = [t.clone() for t in bufs] + [idx.clone()]
    cfgs = [g.PPOConfig(ent_coef=0.01, clip_range=bt.clips[k], vf_coef=E.VF_COEFS[k], max_grad_norm=0.5) for k in range(bt.K)]
    for apply, steps in ((False, 1), (True, 2)):
        pset = g.ActorCriticSet.from_members([LS.device_policy(g, bt, k) for k in range(bt.K)])
        stacks = {}
        for n in R.PARAM_NAMES:
            pset.params[n], stacks[n] = LS.carve(tuple(pset.params[n].shape), init=pset.params[n])
        start = {n: pset.params[n].clone() for n in R.PARAM_NAMES}
        fu = g.FusedUpdateSet(pset, cfgs, *bufs)
        assert all(p.data_ptr() == pset.params[n].data_ptr() for p, n in zip(fu._params, R.PARAM_NAMES))
        hyper = fu.hyper.clone()
        total = fu.grad.shape[1]
        carved = {name: LS.carve(tuple(getattr(fu, name).shape)) for name in ("grad", "m", "v", "stats")}
        carved["step_count"] = LS.carve((bt.K,), dtype=torch.int32, sent=-77)
        for name, (view, _) in carved.items():
            setattr(fu, name, view)
        for _ in range(steps):
            fu.step(idx, apply=apply)
            torch.cuda.synchronize()
        for name, (view, big) in carved.items():
            LS.intact((apply, name), big, view.numel(), -77 if name == "step_count" else LS.SENT)
        for n in R.PARAM_NAMES:
            LS.intact((apply, n), stacks[n], pset.params[n].numel())
            assert torch.equal(pset.params[n], start[n]) != apply, (apply, n)       # moved when applied, and only then
        assert fu.step_count.cpu().tolist() == [steps if apply else 0] * bt.K
        assert torch.equal(fu.hyper, hyper) and fu.grad.shape == (bt.K, total)
        assert float(fu.m.abs().max()) > 0.0 if apply else float(fu.grad.abs().max()) > 0.0             # it did run
    for t, q in zip(bufs + [idx], reads):
        assert torch.equal(t, q)


# ---- f. a rollout buffer past 2^31 floats -------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("D", (29, 197))
def test_update_gathers_rows_past_2_31_floats(g, D):
    """obs is [2^31 // D + 4 096, D] zeros (8.6 GB); the B = 130 rows of the wide_obs minibatch are written at row numbers
    of which 66 lie beyond float 2^31 of obs -- one is the last row, one straddles the boundary -- so `s * D + k` must be
    taken in 64 bits.  Raw gradient against float64 on the gathered rows.  Skipped, with the reason printed, where less
    than 12 GB of device memory is free."""
    B = 130
    free = torch.cuda.mem_get_info()[0]
    if free < 12 * 2 ** 30:
        print("skipped: %.1f GB of device memory free, the buffer needs 12" % (free / 2 ** 30))
        pytest.skip("needs 12 GB of free device memory")
    bt = LS.edge_batch("solo", D, B, "wide_obs")
    n = 2 ** 31 // D + 4096
    edge = 2 ** 31 // D                                      # the row that holds float 2^31
    assert edge * D < 2 ** 31 < (edge + 1) * D               # ... and straddles it
    rng = np.random.default_rng(D)
    rows = np.concatenate([[0, edge - 1, edge, n - 1], rng.integers(1, edge - 1, 62),
                           edge + 1 + rng.choice(n - edge - 2, 64, replace=False)])
    rows = rows[rng.permutation(B)].astype(np.int64)
    assert len(np.unique(rows)) == B and (rows * D + D - 1 >= 2 ** 31).sum() >= B // 2 and rows.max() == n - 1
    small = [a[bt.idx[0]] for a in (bt.obs, bt.act, bt.old_logp, bt.adv, bt.ret)]
    idx = LS.dev(rows)
    bufs = [torch.zeros((n, D) if i == 0 else (n,), dtype=torch.float32, device=DEV) for i in range(5)]
    fu = None
    try:
        for big, a in zip(bufs, small):
            big[idx] = LS.dev(a)
        pol = LS.device_policy(g, bt)
        cfg = g.PPOConfig(ent_coef=0.01, max_grad_norm=-1.0, clip_range=0.2)
        fu = g.FusedUpdate(pol, cfg, *bufs)
        fu.step(idx)
        torch.cuda.synchronize()
        got = fu.grad.double().cpu().numpy()
        st = fu.stats.double().cpu().numpy()
    finally:
        del bufs
        fu = None
        torch.cuda.empty_cache()
    got[-1] -= cfg.ent_coef
    ref, pg, vf, _ = R.grad64(bt.ac_cls, cfg, D, bt.theta(), *bt.rows())
    LS.assert_per_tensor("rows past 2^31 floats D=%d" % D, got, ref, R.segments(pol), LS.TAU)
    LS.check_losses("D=%d" % D, st[0], st[1], pg, vf)
