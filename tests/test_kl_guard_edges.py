"""acas2d_ppo_update_guarded_set_f32 (csrc/acas2d_ppo_guard.hip: target_kl early stop, approx_kl and clip_fraction on the
device) on the hand-placed edge minibatches of tests/edge_minibatches.py and at the edges of its own decision, against the
float64 restatements of tests/kl_guard_ref.py and tests/learner_ref.py.  Bounds and criteria are the neighbours', unchanged:
approx_kl within 1e-5 max(1, kl64), the clipped count exact, the applied step at learner_support.check_applied's bounds
(TAU_M 2e-5, TAU_V 5e-5, parameter excess 1e-2 lr), losses and norm 1e-5.

  CPU  admission, per batch and member: ppo.approx_kl_and_clip_fraction on a float32 CPU copy of the member clears a
       quarter of the approx_kl bound, counts exactly the rows float64 counts, and no row is closer to a clip edge than 10 x
       the largest |ratio32 - ratio64| of that forward (the exact-count assertion is valid only then).  The 96 three-member
       batches (D in 8, 29, 53, 197; B in 2, 65, 130; the eight cases) and the four B = 8 193 batches, those by a float32
       emulation of the accumulation (sums per 64 rows, the 129 partials added in four orders).
  GPU  a  the 96 three-member edge batches through FusedUpdateSet(diagnostics=True), every limit 0: approx_kl, the clipped
          fraction, the bookkeeping of diag, and the applied step against grad64 + adam64 -- the float64 check of the Guard =
          true instantiations above one workgroup, which the bitwise identity of test_kl_guard.py (B <= 64) cannot give
       b  B = 8 193: 129 workgroups' atomics on one diag row, through FusedUpdate(diagnostics=True) and a set of one
       c  the float32 comparison kl > 1.5f * limit at its boundary (adjacent float32 limits on either side of it), and the
          limits NaN, -1, -0, +inf and the smallest subnormal
       d  sentinels round every buffer the entry takes, with a member stopped beforehand (nothing of its rows is
          written), a member that stops in this call and one without a limit (bit-equal to its own K = 1 run at B = 64)
       e  a member with a NaN old_logp: its approx_kl is NaN, it does not stop, and its neighbours do not notice
Every test prints what it observed.

Admission on the CPU, worst over the 96 batches x 3 members: approx_kl 0.044 of the bound (log_std-2.5, D = 53, B = 2); no
clipped-count mismatch; the smallest edge distance 45 ratio errors (log_std-2.5, D = 29, B = 130; 24 with another CPU's
float32 forward); kl64 of the underflow case 10 to 55.  B = 8 193: 0.005 of the bound over the four orders, counts 5587,
5665, 5600, 5664 in float32 and float64 alike, edge distance >= 1.3e-4 = 29 ratio errors.

Observed on an MI355X (one run of this file): approx_kl at most 0.096 of the bound over the 288 members of (a) (9.6e-7
absolute; log_std-2.5, D = 53, B = 2, member 0), per case saturated 0.009, wide_obs 0.015, grid_adv 0.022, const_adv 0.019,
log_std-2.5 0.096, log_std+1.0 0.011, dup_rows 0.023, underflow 0.013; every clipped fraction exact; the least room to a
clip edge 24 x the CPU float32 ratio error.  The applied steps of (a): m 2.6e-6 (saturated), v 1.34e-5 (wide_obs),
parameter excess 2.4e-3 lr (wide_obs) at worst -- the unguarded set update's figures.  (b) at most 0.004 of the bound, the
four counts exact on both paths.  No case exposed a fault in the kernels.  Run time: 110 GPU tests in 11.0 s, the slowest
0.6 s (the first, which loads the library).
With one arithmetic line of a kernel changed, the 110 GPU tests of this file fail as follows (each build run once): kl_s
formed from the clamped ratio, 105; the guarded apply kernel dividing by the row count rounded up to 64, 103;
SetMember::clip_range() (csrc/acas2d_ppo_wide.hpp) reading member 0's row (the wide kernels only), 49.
"""
import numpy as np
import pytest

import edge_minibatches as E
import helpers as H
import kl_guard_ref as KR
import learner_ref as R
import learner_support as LS

torch = pytest.importorskip("torch")
LR = LS.LR
WIDTHS, ROWS = (8, 29, 53, 197), (2, 65, 130)
SET = [(D, B, case) for D in WIDTHS for B in ROWS for case in E.CASES]
LARGE = [(D, 8193, case) for D in (8, 197) for case in ("mixed", "grid_adv")]
_ID = lambda c: "D%d-B%d-%s" % c  # noqa: E731
KL_TOL = 1e-5                          # approx_kl: 1e-5 max(1, kl64), test_kl_guard.py's
EDGE_ROOM = 10.0                       # edge distance >= 10 x the float32 forward's ratio error


@pytest.fixture(scope="module")
def g():
    import gym_acas2d_amd as g
    g.native.lib()
    return g


@pytest.fixture(scope="module")
def gpu(g):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return g


def _kl_bound(kl64):
    return KL_TOL * max(1.0, kl64)


def _log_ratio64(bt, k, theta=None):
    obs, act, old, _, _ = bt.rows(k)
    return KR.log_ratio64(bt.ac_cls, bt.D, bt.theta(k) if theta is None else theta, obs, act, old)


def _forward32(g, bt, k):
    """Member k's minibatch through a float32 CPU copy of its policy: approx_kl and clip_fraction as
    ppo.approx_kl_and_clip_fraction gives them, and the float32 log ratios and ratios of that forward."""
    pol = R.policy64(bt.ac_cls, bt.D, bt.theta(k)).float()
    i = bt.idx[k]
    obs, act, old = torch.as_tensor(bt.obs[i]), torch.as_tensor(bt.act[i]).reshape(-1, 1), torch.as_tensor(bt.old_logp[i])
    kl, cf = g.ppo.approx_kl_and_clip_fraction(pol, g.PPOConfig(clip_range=bt.clips[k]), obs, act, old)
    with torch.no_grad():
        mean, _ = pol.forward(obs)
        lr32 = g.ppo._normal_logp(mean, pol.log_std, act) - old
    assert kl.dtype == torch.float32 and lr32.dtype == torch.float32
    return float(kl), float(cf), lr32.numpy(), lr32.exp().numpy()


def _edge_room(g, bt, k, lr64):
    """(edge distance, largest |ratio32 - ratio64| of the CPU float32 forward) of member k's minibatch."""
    _, _, _, r32 = _forward32(g, bt, k)
    return KR.edge_distance(lr64, bt.clips[k]), float(np.abs(r32.astype(np.float64) - np.exp(lr64)).max())


# ---- CPU: admission ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,B,case", SET, ids=[_ID(c) for c in SET])
def test_guarded_statistics_of_set_case_are_admitted(g, D, B, case):
    """Per member: float32 approx_kl within a quarter of 1e-5 max(1, kl64); float32 clip_fraction == float32(count64) /
    float32(B); edge distance >= 10 x the largest ratio error.  underflow: kl64 is about 110 x the share of underflowed
    rows, so the large-term path is the one checked."""
    bt = LS.edge_batch("set", D, B, case)
    for k in range(bt.K):
        lr64 = _log_ratio64(bt, k)
        kl64, (count, _) = KR.approx_kl64(lr64), KR.clip_fraction64(lr64, bt.clips[k])
        kl32, cf32, _, r32 = _forward32(g, bt, k)
        frac = abs(kl32 - kl64) / _kl_bound(kl64)
        edge, rerr = KR.edge_distance(lr64, bt.clips[k]), float(np.abs(r32.astype(np.float64) - np.exp(lr64)).max())
        print("admitted %s D=%d B=%d member %d: approx_kl %.8g vs %.8g (%.3f of the bound), clipped %d of %d, edge distance "
              "%.2e = %.0f x the ratio error %.2e" % (case, D, B, k, kl32, kl64, frac, count, B, edge, edge / max(rerr, 1e-300), rerr))
        assert frac <= 0.25, (k, kl32, kl64)
        assert np.float32(cf32) == np.float32(count) / np.float32(B), (k, cf32, count, B)
        assert edge >= EDGE_ROOM * rerr, (k, edge, rerr)
        assert kl64 > 0.0
        if case == "underflow":
            assert kl64 > 5.0, (k, kl64)                   # (>= a twentieth of the rows at 110 each)
        if B >= 65 and case != "dup_rows":             # (dup_rows at B = 65: 64 rows are one sample, clipped or not together)
            assert 0 < count < B, (k, count)


def _partials32(lr32, r32):
    """Float32 sums of (ratio - 1) - log ratio per 64 rows, in row order: one per workgroup of the gradient launch."""
    t = ((r32 - np.float32(1.0)) - lr32).astype(np.float32)
    pad = np.concatenate([t, np.zeros(-len(t) % 64, np.float32)]).reshape(-1, 64)
    return [np.add.accumulate(p, dtype=np.float32)[-1] for p in pad]


@pytest.mark.parametrize("D,B,case", LARGE, ids=[_ID(c) for c in LARGE])
def test_guarded_statistics_at_8193_rows_are_admitted(g, D, B, case):
    """129 partial sums (one per 64 rows) added in float32 forwards, backwards and in both sorted orders, then / B: each
    within a quarter of the approx_kl bound.  The count: every partial is an integer <= 64, every running sum an integer
    <= 8 193 < 2^24, so float atomics in any order give float32(count); float32 and float64 count the same rows."""
    bt = LS.edge_batch("solo", D, B, case)
    lr64 = _log_ratio64(bt, 0)
    kl64, (count, _) = KR.approx_kl64(lr64), KR.clip_fraction64(lr64, 0.2)
    _, cf32, lr32, r32 = _forward32(g, bt, 0)
    parts = _partials32(lr32, r32)
    assert len(parts) == 129
    worst = 0.0
    for order in (parts, parts[::-1], sorted(parts), sorted(parts)[::-1]):
        s = np.float32(0)
        for p in order:
            s = np.float32(s + p)
        worst = max(worst, abs(float(s / np.float32(B)) - kl64) / _kl_bound(kl64))
    count32 = int((np.abs(r32 - np.float32(1.0)) > np.float32(0.2)).sum())
    edge, rerr = KR.edge_distance(lr64, 0.2), float(np.abs(r32.astype(np.float64) - np.exp(lr64)).max())
    print("admitted %s D=%d B=%d: approx_kl64 %.8g, worst order %.3f of the bound, clipped %d (float32) %d (float64), edge "
          "distance %.2e = %.0f x the ratio error %.2e" % (case, D, B, kl64, worst, count32, count, edge, edge / rerr, rerr))
    assert worst <= 0.25
    assert count32 == count and np.float32(cf32) == np.float32(count) / np.float32(B) and 0 < count < B
    assert edge >= EDGE_ROOM * rerr, (edge, rerr)


# ---- GPU --------------------------------------------------------------------------------------------------------------
_worst = {"kl": 0.0, "room": np.inf}


def _check_statistics(g, what, bt, k, diag_k, B, lr64, clip, calls=1.0):
    """diag[k] after one guarded, applied call against float64: test_guarded_statistics_vs_float64's assertions."""
    kl64, (count, _) = KR.approx_kl64(lr64), KR.clip_fraction64(lr64, clip)
    frac = abs(float(diag_k[2]) - kl64) / _kl_bound(kl64)
    edge, rerr = _edge_room(g, bt, k, lr64)
    _worst["kl"], _worst["room"] = max(_worst["kl"], frac), min(_worst["room"], edge / max(rerr, 1e-300))
    print("  %s: approx_kl %.8g vs %.8g (%.3f of the bound), clipped %d of %d -> %.8g (float64 rows %d), edge distance "
          "%.2e = %.0f x the CPU float32 ratio error; so far worst %.3f of the bound, least room %.0f x"
          % (what, diag_k[2], kl64, frac, round(float(diag_k[3]) * B), B, diag_k[3], count, edge, edge / max(rerr, 1e-300),
             _worst["kl"], _worst["room"]))
    assert frac <= 1.0, (what, diag_k[2], kl64)
    assert diag_k[3] == np.float32(count) / np.float32(B), (what, diag_k[3], count, B)
    assert diag_k[0] == 0.0 and diag_k[1] == 0.0, what
    assert diag_k[4] == diag_k[2] and diag_k[5] == diag_k[3] and diag_k[6] == calls and diag_k[7] == calls, what
    return kl64, count


@pytest.mark.gpu
@pytest.mark.parametrize("D,B,case", SET, ids=[_ID(c) for c in SET])
def test_guarded_set_update_on_edge_minibatches_vs_float64(gpu, D, B, case):
    """One guarded call (every limit 0) of K = 3 members with their own policy, clip_range 0.1 / 0.2 / 0.3 and vf_coef 0.5 /
    0.25 / 1.0: diag[k] against float64, then the step it applied against grad64 + adam64 from the kernel's own pre-step
    state (test_set_update_on_edge_minibatches_vs_float64's second half, through the Guard = true kernels).  const_adv:
    every actor bit kept although approx_kl and, from B = 65, the clipped count are not zero."""
    g = gpu
    bt = LS.edge_batch("set", D, B, case)
    idx = LS.dev(bt.idx)
    segs = R.segments(bt.pols[0])
    na = LS.n_actor(segs)
    theta0 = [bt.theta(k) for k in range(bt.K)]
    ent = 0.0 if case == "const_adv" else 0.01
    cf = [g.PPOConfig(ent_coef=ent, clip_range=bt.clips[k], vf_coef=E.VF_COEFS[k], max_grad_norm=0.5, learning_rate=LR)
          for k in range(bt.K)]
    pset = g.ActorCriticSet.from_members([LS.device_policy(g, bt, k) for k in range(bt.K)])
    fu = g.FusedUpdateSet(pset, cf, *LS.device_bufs(bt), diagnostics=True)
    assert fu.guarded and float(fu.target_kl.abs().max()) == 0.0
    fu.begin_update()
    fu.step(idx)
    torch.cuda.synchronize()
    diag = fu.diag.cpu().numpy()
    assert fu.stopped.cpu().tolist() == [0] * bt.K and fu.step_count.cpu().tolist() == [1] * bt.K
    assert float(fu.grad.abs().max()) == 0.0 and float(fu.stats[:, 0:2].abs().max()) == 0.0
    assert bool(torch.isfinite(fu.stats).all()) and np.isfinite(diag).all()
    for k in range(bt.K):
        what = "guarded %s D=%d B=%d member %d" % (case, D, B, k)
        kl64, count = _check_statistics(g, what, bt, k, diag[k], B, _log_ratio64(bt, k), bt.clips[k])
        grad, pg, vf, _ = R.grad64(bt.ac_cls, cf[k], D, theta0[k], *bt.rows(k))
        theta_ref, m_ref, v_ref, norm = R.adam64(theta0[k], grad, np.zeros_like(grad), np.zeros_like(grad), 0, 0.5, LR, 0.9, 0.999, 1e-5)
        st = fu.stats[k].double().cpu().numpy()
        theta1, m1, v1 = LS.theta_of(pset, k), fu.m[k].double().cpu().numpy(), fu.v[k].double().cpu().numpy()
        assert np.isfinite(theta1).all() and np.isfinite(m1).all() and np.isfinite(v1).all()
        assert abs(st[2] - norm) <= 1e-5 * norm, (what, st[2], norm)
        LS.check_losses(what + " applied", st[4], st[5], pg, vf)
        LS.check_applied(what, segs, theta1, m1, v1, theta_ref, m_ref, v_ref, LR)
        if case == "underflow":
            assert kl64 > 5.0, what
        if case == "const_adv":
            assert np.array_equal(theta1[:na], theta0[k][:na]) and theta1[-1] == theta0[k][-1], what
            assert not m1[:na].any() and not v1[:na].any() and m1[-1] == 0.0 and v1[-1] == 0.0, what
            assert np.median(np.abs(theta1[na:-1] - theta0[k][na:-1]) / LR) > 0.05, what
            assert diag[k, 2] > 0.0 and (B < 65 or diag[k, 3] > 0.0), what


@pytest.mark.gpu
@pytest.mark.parametrize("D,B,case", LARGE, ids=[_ID(c) for c in LARGE])
def test_guarded_statistics_at_8193_rows_vs_float64(gpu, D, B, case):
    """B = 8 193: 129 actor workgroups add to diag[0][0] and diag[0][1], the last from one live row.  Through
    FusedUpdate(diagnostics=True) and through a FusedUpdateSet of one member: approx_kl within 1e-5 max(1, kl64), the
    clipped fraction == float32(count64) / float32(B) (every partial sum an integer below 2^24)."""
    g = gpu
    bt = LS.edge_batch("solo", D, B, case)
    cfg = g.PPOConfig(ent_coef=0.01, max_grad_norm=0.5, learning_rate=LR, clip_range=0.2)
    lr64 = _log_ratio64(bt, 0)
    bufs = LS.device_bufs(bt)
    pol = LS.device_policy(g, bt)
    solo = g.FusedUpdate(pol, cfg, *bufs, diagnostics=True)
    pset = g.ActorCriticSet.from_members([LS.device_policy(g, bt)])
    one = g.FusedUpdateSet(pset, [cfg], *bufs, diagnostics=True)
    assert solo.guarded and one.guarded
    for name, fu, idx in (("FusedUpdate", solo, LS.dev(bt.idx[0])), ("FusedUpdateSet K=1", one, LS.dev(bt.idx))):
        fu.begin_update()
        fu.step(idx)
        torch.cuda.synchronize()
        assert fu.stopped.cpu().tolist() == [0] and fu.step_count.cpu().tolist() == [1]
        kl64, count = _check_statistics(g, "%s %s D=%d B=%d" % (name, case, D, B), bt, 0, fu.diag.cpu().numpy()[0], B, lr64, 0.2)
        assert 0 < count < B and kl64 > 1e-2
    assert not np.array_equal(R.flat_params(pol), bt.theta()) and not np.array_equal(LS.theta_of(pset, 0), bt.theta())


# ---- c. the decision at its float32 boundary -----------------------------------------------------------------------------
_TENSORS = ("grad", "m", "v", "step_count", "stats", "diag", "stopped")


def _snapshot(fu, pset):
    s = {n: pset.params[n].clone() for n in R.PARAM_NAMES}
    s.update({n: getattr(fu, n).clone() for n in _TENSORS})
    return s


def _rows_equal(what, a, b, members, names=None):
    for n in (names or list(a)):
        for k in members:
            assert H.bits_equal(a[n][k], b[n][k]), (what, n, k)


def _stopped_before_anything_moved(what, now, start, k):
    """Member k as the decision test describes a member that stopped on its first minibatch."""
    _rows_equal(what, now, start, [k], list(R.PARAM_NAMES) + ["m", "v", "step_count"])
    assert int(now["stopped"][k]) == 1 and int(now["step_count"][k]) == 0, what
    assert float(now["grad"][k].abs().max()) == 0.0, what
    d, st = now["diag"][k].cpu().numpy(), now["stats"][k].cpu().numpy()
    assert d[0] == 0.0 and d[1] == 0.0 and d[4] == d[2] and d[5] == d[3] and d[6] == 1.0 and d[7] == 0.0, (what, d)
    assert st[0] == 0.0 and st[1] == 0.0 and st[2] == 0.0, (what, st)


def _guarded_run(g, bt, cfgs, idx, limits):
    """One guarded call of a fresh twin with the float32 `limits`: (state before, state after)."""
    pset = bt.policy_set()
    fu = g.FusedUpdateSet(pset, cfgs, *bt.bufs, diagnostics=True)
    fu.begin_update()
    fu.target_kl.copy_(torch.as_tensor(np.asarray(limits, np.float32)))
    assert H.bits_equal(fu.target_kl.cpu(), torch.as_tensor(np.asarray(limits, np.float32)))
    start = _snapshot(fu, pset)
    fu.step(idx)
    torch.cuda.synchronize()
    return start, _snapshot(fu, pset)


def _stops32(kl32, t):
    """The apply kernel's `limit > 0.0f && kl > 1.5f * limit` in NumPy float32."""
    with np.errstate(invalid="ignore"):
        return bool(t > np.float32(0.0)) and bool(kl32 > np.float32(1.5) * t)


@pytest.mark.gpu
@pytest.mark.parametrize("D,B", [(D, B) for D in (8, 53) for B in (2, 64)])
def test_stop_decision_at_its_float32_boundary(gpu, D, B):
    """K = 3, one workgroup per network: diag[k][2] is one atomic onto zero, then one division, so every run of the same
    minibatch gives the same kl32.  Candidates: float32(kl32 / 1.5) and its neighbours within 2 ulp; the reference
    predicate is kl32 > float32(1.5) * t in NumPy float32.  Run A, every member at its largest candidate that stops: all
    three stop with nothing moved.  Run B, every member at its smallest candidate that does not: none stops, and
    everything equals the probe bit for bit.  The two candidates of a member are adjacent float32 values.  Then NaN, -1,
    -0 (never stop), +inf (never stops) and the smallest subnormal (stops a member with kl32 > 0)."""
    g = gpu
    K = 3
    bt = LS.RolloutBatch(g, D, K, K * B + 317, seed=11000 + 7 * D + B)
    cfgs = LS.member_cfgs(g, K)
    idx = LS.draw(bt, bt.policy_set(), [c.clip_range for c in cfgs], B)
    start, probe = _guarded_run(g, bt, cfgs, idx, [0.0] * K)
    assert probe["stopped"].cpu().tolist() == [0] * K and probe["step_count"].cpu().tolist() == [1] * K
    kl32 = probe["diag"][:, 2].cpu().numpy()
    assert kl32.dtype == np.float32 and (kl32 > 1e-4).all()
    stop_at, pass_at = [], []
    for k in range(K):
        c = np.float32(kl32[k] / np.float32(1.5))
        cands = [c]
        for _ in range(2):
            cands = [np.nextafter(cands[0], np.float32(0))] + cands + [np.nextafter(cands[-1], np.float32(np.inf))]
        stop = [t for t in cands if _stops32(kl32[k], t)]
        keep = [t for t in cands if not _stops32(kl32[k], t)]
        assert stop and keep and max(stop) < min(keep), (k, kl32[k], cands)
        assert np.nextafter(max(stop), np.float32(np.inf)) == min(keep), (k, max(stop), min(keep))
        stop_at.append(max(stop))
        pass_at.append(min(keep))
        print("D=%d B=%d member %d: kl32 %.9g (%s), stops at limit %.9g (%s), does not at %.9g (%s)"
              % (D, B, k, kl32[k], kl32[k].tobytes().hex(), stop_at[k], stop_at[k].tobytes().hex(), pass_at[k], pass_at[k].tobytes().hex()))
    members = range(K)
    # ---- A: the largest limits that stop
    a0, a = _guarded_run(g, bt, cfgs, idx, stop_at)
    print("  run A: stopped %s, diag[:, 7] %s" % (a["stopped"].cpu().tolist(), a["diag"][:, 7].cpu().tolist()))
    _rows_equal("run A start", a0, start, members)
    assert a["stopped"].cpu().tolist() == [1] * K
    for k in members:
        _stopped_before_anything_moved("run A member %d" % k, a, a0, k)
    assert H.bits_equal(a["diag"][:, 2], probe["diag"][:, 2]) and H.bits_equal(a["diag"][:, 3], probe["diag"][:, 3])
    assert H.bits_equal(a["stats"][:, 4:6], probe["stats"][:, 4:6])          # the stopping minibatch's losses are logged
    # ---- B: the smallest limits that do not
    _, b = _guarded_run(g, bt, cfgs, idx, pass_at)
    print("  run B: stopped %s, diag[:, 7] %s" % (b["stopped"].cpu().tolist(), b["diag"][:, 7].cpu().tolist()))
    assert b["stopped"].cpu().tolist() == [0] * K
    _rows_equal("run B", b, probe, members)
    # ---- limits that never stop, and +inf
    for limits in ([np.nan, -1.0, -0.0], [np.inf] * K):
        _, c = _guarded_run(g, bt, cfgs, idx, limits)
        print("  limits %s: stopped %s" % (limits, c["stopped"].cpu().tolist()))
        assert c["stopped"].cpu().tolist() == [0] * K and not any(_stops32(kl32[k], np.float32(limits[k])) for k in members)
        _rows_equal("limits %s" % (limits,), c, probe, members)
    # ---- the smallest subnormal stops; its neighbours (no limit, +inf) go on
    tiny = np.float32(1e-45)
    assert tiny > 0 and _stops32(kl32[1], tiny)
    d0, d = _guarded_run(g, bt, cfgs, idx, [0.0, tiny, np.inf])
    print("  limits [0, 1e-45, inf]: stopped %s" % d["stopped"].cpu().tolist())
    assert d["stopped"].cpu().tolist() == [0, 1, 0]
    _stopped_before_anything_moved("limit 1e-45", d, d0, 1)
    _rows_equal("beside limit 1e-45", d, probe, [0, 2])


# ---- d. a stopped member writes nothing; sentinels -----------------------------------------------------------------------
def _three_kinds(g, bt, idx, B):
    """cfgs and float32 limits for: member 0 (stopped beforehand), member 1 (a limit it exceeds: a third of its float64
    approx_kl on these rows), member 2 (no limit)."""
    cfgs = [g.PPOConfig(ent_coef=0.01, clip_range=bt.clips[k], vf_coef=E.VF_COEFS[k], max_grad_norm=0.5, learning_rate=LR)
            for k in range(bt.K)]
    i = idx[1]
    lr64 = KR.log_ratio64(bt.ac_cls, bt.D, bt.theta(1), bt.obs[i], bt.act[i], bt.old_logp[i])
    kl64 = KR.approx_kl64(lr64)
    assert kl64 > 1e-5 and KR.stops(kl64, kl64 / 3.0)
    return cfgs, [0.0, kl64 / 3.0, 0.0], kl64


def _pattern(t, k):
    """Member k's row of `t` filled with a non-zero pattern no kernel would leave behind."""
    row = t[k]
    row.copy_((torch.arange(row.numel(), device=row.device) % 251).to(row.dtype).reshape(row.shape) + (3 if row.dtype == torch.int32 else 3.5))
    assert bool((row != 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("D", (8, 53))
def test_guarded_update_writes_nothing_outside_its_rows(gpu, D):
    """K = 3, B = 65 (a second workgroup with one live row).  Every buffer the guarded entry takes is the middle of a
    sentinel-filled allocation: the 13 stacks, grad, m, v, step, stats, hyper, target_kl, stopped, diag.  Member 0 has
    stopped = 1 beforehand and a non-zero pattern in its grad, m, v, stats and diag rows: after the call every byte of its
    rows is as it was (both launches return before writing anything).  Member 1 exceeds its limit: it stops as the decision
    test describes.  Member 2 has no limit and applies its step.  Every sentinel, every input, idx, hyper and target_kl are
    intact."""
    g = gpu
    B = 65
    bt = LS.edge_batch("set", D, B, "dup_rows")
    bufs, idx = LS.device_bufs(bt), LS.dev(bt.idx)
    reads = [t.clone() for t in bufs] + [idx.clone()]
    cfgs, limits, kl64 = _three_kinds(g, bt, bt.idx, B)
    pset = g.ActorCriticSet.from_members([LS.device_policy(g, bt, k) for k in range(bt.K)])
    stacks = {}
    for n in R.PARAM_NAMES:
        pset.params[n], stacks[n] = LS.carve(tuple(pset.params[n].shape), init=pset.params[n])
    fu = g.FusedUpdateSet(pset, cfgs, *bufs, diagnostics=True)
    assert fu.guarded and all(p.data_ptr() == pset.params[n].data_ptr() for p, n in zip(fu._params, R.PARAM_NAMES))
    carved = {name: LS.carve(tuple(getattr(fu, name).shape)) for name in ("grad", "m", "v", "stats", "diag")}
    carved["hyper"] = LS.carve(tuple(fu.hyper.shape), init=fu.hyper)
    carved["target_kl"] = LS.carve((bt.K,), init=torch.as_tensor(np.asarray(limits, np.float32)))
    carved["step_count"] = LS.carve((bt.K,), dtype=torch.int32, sent=-77)
    carved["stopped"] = LS.carve((bt.K,), dtype=torch.int32, sent=-77)
    for name, (view, _) in carved.items():
        setattr(fu, name, view)
    fu._guard = g.native.CPpoGuard(fu.target_kl.data_ptr(), fu.stopped.data_ptr(), fu.diag.data_ptr())
    fu.stopped[0] = 1
    for name in ("grad", "m", "v", "stats", "diag"):
        _pattern(getattr(fu, name), 0)
    start = _snapshot(fu, pset)
    hyper, target = fu.hyper.clone(), fu.target_kl.clone()
    fu.step(idx)
    torch.cuda.synchronize()
    now = _snapshot(fu, pset)
    for name, (view, big) in carved.items():
        LS.intact(name, big, view.numel(), -77 if name in ("step_count", "stopped") else LS.SENT)
    for n in R.PARAM_NAMES:
        LS.intact(n, stacks[n], pset.params[n].numel())
    for t, q in zip(bufs + [idx], reads):
        assert torch.equal(t, q)
    assert H.bits_equal(fu.hyper, hyper) and H.bits_equal(fu.target_kl, target)
    print("D=%d: stopped %s, adam_step %s, diag[:, 6] %s, diag[:, 7] %s, member 1 approx_kl %.8g vs %.8g (limit %.4g)"
          % (D, now["stopped"].cpu().tolist(), now["step_count"].cpu().tolist(), now["diag"][:, 6].cpu().tolist(),
             now["diag"][:, 7].cpu().tolist(), float(now["diag"][1, 2]), kl64, limits[1]))
    _rows_equal("member 0", now, start, [0])               # every tensor, the pattern included
    assert now["stopped"].cpu().tolist() == [1, 1, 0] and now["step_count"].cpu().tolist() == [0, 0, 1]
    _stopped_before_anything_moved("member 1", now, start, 1)
    assert abs(float(now["diag"][1, 2]) - kl64) <= _kl_bound(kl64)
    _, pg, vf, _ = R.grad64(bt.ac_cls, cfgs[1], D, bt.theta(1), *bt.rows(1))
    LS.check_losses("member 1, stopping minibatch", float(now["stats"][1, 4]), float(now["stats"][1, 5]), pg, vf)
    d2 = now["diag"][2].cpu().numpy()
    assert d2[6] == 1.0 and d2[7] == 1.0 and d2[0] == 0.0 and d2[1] == 0.0 and float(now["grad"][2].abs().max()) == 0.0
    assert float(now["m"][2].abs().max()) > 0.0 and bool(torch.isfinite(now["m"][2]).all())
    for n in R.PARAM_NAMES[:4]:
        assert not torch.equal(now[n][2], start[n][2]), n    # it did run


@pytest.mark.gpu
@pytest.mark.parametrize("D", (8, 53))
def test_member_beside_stopped_members_equals_its_own_run(gpu, D):
    """The three kinds of member again at B = 64 (one atomic per gradient entry): member 2, between a member stopped
    beforehand and one that stops in this call, leaves the bits of a K = 1 guarded run of itself on the same rows --
    parameters, moments, step count, stats and diag."""
    g = gpu
    B = 64
    bt = LS.edge_batch("set", D, 65, "underflow")               # (dup_rows' first 64 rows can be ONE row: no actor gradient)
    rows = np.ascontiguousarray(bt.idx[:, :B])
    cfgs, limits, kl64 = _three_kinds(g, bt, rows, B)
    bufs = LS.device_bufs(bt)
    pset = g.ActorCriticSet.from_members([LS.device_policy(g, bt, k) for k in range(bt.K)])
    fu = g.FusedUpdateSet(pset, cfgs, *bufs, diagnostics=True)
    fu.begin_update()
    fu.target_kl.copy_(torch.as_tensor(np.asarray(limits, np.float32)))
    fu.stopped[0] = 1
    start = _snapshot(fu, pset)
    fu.step(LS.dev(rows))
    twin_set = g.ActorCriticSet.from_members([LS.device_policy(g, bt, 2)])
    twin = g.FusedUpdateSet(twin_set, [cfgs[2]], *bufs, diagnostics=True)
    twin.begin_update()
    twin.step(LS.dev(rows[2:3]))
    torch.cuda.synchronize()
    now, alone = _snapshot(fu, pset), _snapshot(twin, twin_set)
    assert now["stopped"].cpu().tolist() == [1, 1, 0] and alone["stopped"].cpu().tolist() == [0]
    _rows_equal("member 0", now, start, [0])
    _stopped_before_anything_moved("member 1", now, start, 1)
    for n in list(R.PARAM_NAMES) + list(_TENSORS):
        assert H.bits_equal(now[n][2], alone[n][0]), n
    moved = float((now[R.PARAM_NAMES[2]][2] - start[R.PARAM_NAMES[2]][2]).abs().max())
    print("D=%d: member 2 == its K = 1 run bit for bit (parameters moved by %.2e, approx_kl %.8g)" % (D, moved, float(now["diag"][2, 2])))
    assert moved > 0.0 and int(now["step_count"][2]) == 1 and float(now["diag"][2, 7]) == 1.0


# ---- e. a non-finite member ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("D", (8, 53))
def test_member_with_a_nan_old_logp_does_not_stop_and_stays_in_its_rows(gpu, D):
    """K = 3, B = 64; one row of member 1's minibatch has old_logp = NaN.  diag[1][2] is NaN; member 1 does not stop,
    without a limit or with one (kl > 1.5f * limit is false for a NaN kl, as SB3's comparison is).  Members 0 and 2 equal
    a run without the NaN bit for bit: parameters, moments, step counts, stats and diag rows."""
    g = gpu
    K, B = 3, 64
    bt = LS.RolloutBatch(g, D, K, K * B + 317, seed=12000 + D)
    cfgs = LS.member_cfgs(g, K)
    idx = LS.draw(bt, bt.policy_set(), [c.clip_range for c in cfgs], B)
    _, clean = _guarded_run(g, bt, cfgs, idx, [0.0] * K)
    assert clean["stopped"].cpu().tolist() == [0] * K and bool(torch.isfinite(clean["diag"]).all())
    bt.old_logp[idx[1, 37]] = float("nan")
    assert not KR.stops(float("nan"), 1e-6)
    for limits in ([0.0] * K, [0.0, 1e-6, 0.0]):
        _, run = _guarded_run(g, bt, cfgs, idx, limits)
        d1 = run["diag"][1].cpu().numpy()
        print("D=%d limits %s: diag[1] %s, stopped %s, adam_step %s" % (D, limits, d1, run["stopped"].cpu().tolist(), run["step_count"].cpu().tolist()))
        assert np.isnan(d1[2]) and run["stopped"].cpu().tolist() == [0] * K
        assert d1[6] == 1.0 and d1[7] == 1.0 and run["step_count"].cpu().tolist() == [1] * K
        _rows_equal("beside the NaN member, limits %s" % (limits,), run, clean, [0, 2])
        for n in R.PARAM_NAMES:
            assert bool(torch.isfinite(run[n][0]).all()) and bool(torch.isfinite(run[n][2]).all()), n
