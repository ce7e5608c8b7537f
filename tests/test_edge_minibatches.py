"""The edge minibatches of tests/edge_minibatches.py on the CPU: every case is the case it claims to be (its labels), and
every case is ADMITTED -- ppo.ppo_loss() with float32 autograd on the CPU meets the float64 reference
(learner_ref.grad64) under the per-tensor criterion of learner_support.assert_per_tensor with tau <= TAU / 4 =
5e-6, so the bound the GPU tests hold the kernels to (TAU = 2e-5) is one that plain float32 clears with room.  A case
that misses is re-tuned in edge_minibatches.py, never given a wider bound.  Every batch tests/test_learner_edges.py runs
is admitted here: the solo batches at D = 8, 29, 53, 197, the three-member batches of the set update at the same four
widths (D = 53, 197 take acas2d_ppo_update_wide_set_f32), and the B = 8 193 batches.  The 48 three-member batches at D = 53,
197 clear the quarter bound: tau below 7e-7 in 47 of them, 4.2e-6 in one (saturated, D = 197, B = 2: two rows, one of them
saturating 197-term sums; 2.6e-6 with torch on one thread).  Each test prints the tau it observed.  The
same batches are admitted for the guarded update's approx_kl and clip_fraction in tests/test_kl_guard_edges.py."""
import numpy as np
import pytest

import edge_minibatches as E
import learner_ref as R
import learner_support as LS

torch = pytest.importorskip("torch")
ADMIT_TAU = LS.TAU / 4
WIDTHS, ROWS = (8, 29, 53, 197), (2, 65, 130)
SOLO = [(D, B, case) for D in WIDTHS for B in ROWS for case in E.CASES]
SET = [(D, B, case) for D in WIDTHS for B in ROWS for case in E.CASES]
LARGE = [(D, 8193, case) for D in (8, 197) for case in ("grid_adv", "mixed")]
_ID = lambda c: "D%d-B%d-%s" % c  # noqa: E731


def _grad32(g, bt, k, cfg):
    """ppo_loss() of member k's minibatch in float32 with torch autograd on the CPU: the flat gradient, pg, vf."""
    pol = R.policy64(bt.ac_cls, bt.D, bt.theta(k)).float()
    i = bt.idx[k]
    t = lambda a: torch.as_tensor(a[i])  # noqa: E731
    loss, pg, vf = g.ppo.ppo_loss(pol, cfg, t(bt.obs), t(bt.act).reshape(-1, 1), t(bt.old_logp), t(bt.adv), t(bt.ret))
    loss.backward()
    grad = torch.cat([pol.get_parameter(n).grad.reshape(-1) for n in R.PARAM_NAMES]).double().numpy()
    return grad, float(pg.detach()), float(vf.detach())


def _admit(kind, D, B, case):
    import gym_acas2d_amd as g
    bt = LS.edge_batch(kind, D, B, case)
    segs = R.segments(bt.pols[0])
    worst = -np.inf
    for k in range(bt.K):
        cfg = g.PPOConfig(ent_coef=0.01, clip_range=bt.clips[k], vf_coef=E.VF_COEFS[k] if bt.K > 1 else 0.5)
        ref, pg, vf, ratio = R.grad64(bt.ac_cls, cfg, D, bt.theta(k), *bt.rows(k))
        got, pg32, vf32 = _grad32(g, bt, k, cfg)
        assert np.isfinite(got).all() and np.isfinite(ref).all()
        worst = max(worst, LS.assert_per_tensor("admission %s %s D=%d B=%d member %d" % (kind, case, D, B, k), got, ref, segs,
                                                ADMIT_TAU))
        assert abs(pg32 - pg) <= 1e-5 * max(1.0, abs(pg)) / 4 and abs(vf32 - vf) <= 1e-5 * max(1.0, vf) / 4, (pg32, pg, vf32, vf)
        if case == "const_adv":
            n_actor = segs[5][2]
            assert not ref[:n_actor].any() and ref[-1] == -cfg.ent_coef and pg == 0.0, (np.abs(ref[:n_actor]).max(), ref[-1], pg)
            assert not got[:n_actor].any() and pg32 == 0.0
            assert np.abs(ref[n_actor:-1]).max() > 0.0
    print("admitted %s %s D=%d B=%d: tau %.2e (bound %.1e)" % (kind, case, D, B, worst, ADMIT_TAU))


@pytest.mark.parametrize("D,B,case", SOLO, ids=[_ID(c) for c in SOLO])
def test_solo_case_is_what_it_claims_and_is_admitted(D, B, case):
    E.check_labels(LS.edge_batch("solo", D, B, case))
    _admit("solo", D, B, case)


@pytest.mark.parametrize("D,B,case", SET, ids=[_ID(c) for c in SET])
def test_set_case_is_what_it_claims_and_is_admitted(D, B, case):
    bt = LS.edge_batch("set", D, B, case)
    assert bt.K == 3 and bt.clips == (0.1, 0.2, 0.3)
    E.check_labels(bt)
    _admit("set", D, B, case)


@pytest.mark.parametrize("D,B,case", LARGE, ids=[_ID(c) for c in LARGE])
def test_large_minibatch_is_admitted(D, B, case):
    bt = LS.edge_batch("solo", D, B, case)
    E.check_labels(bt)
    if case == "grid_adv":
        assert bt.labels["grid"][0]["c"] == 64.0
    _admit("solo", D, B, case)


def test_grid_advantage_statistics_do_not_depend_on_the_order():
    """The point of the grid: float32 mean and sum of squared deviations are the same bits forwards, backwards, in 64
    strided partial sums (the narrow kernel's lanes) and in 256 (the wide kernel's threads)."""
    for B in (2, 3, 65, 130, 4096, 8193):
        adv, c, q, k = E.grid_advantages(B, np.random.default_rng(B))
        sums, sqs = set(), set()
        for order in (np.arange(B), np.arange(B)[::-1]):
            for lanes in (1, 64, 256):
                x = adv[order]
                s = np.float32(0)
                for part in [np.add.accumulate(x[l::lanes], dtype=np.float32)[-1] for l in range(min(lanes, B))]:
                    s = np.float32(s + part)
                mean = np.float32(s / np.float32(B))
                d = x - mean
                sq = np.float32(0)
                for part in [np.add.accumulate(d[l::lanes] * d[l::lanes], dtype=np.float32)[-1] for l in range(min(lanes, B))]:
                    sq = np.float32(sq + part)
                sums.add(float(mean))
                sqs.add(float(sq))
        assert sums == {c} and len(sqs) == 1, (B, sums, sqs)
        assert sqs.pop() == float((k.astype(np.float64) ** 2).sum() * q * q)


def test_one_common_factor_cannot_place_both_layers():
    """Why `saturated` scales each hidden matrix by its own factor: at D = 8 no single factor on both hidden matrices of
    the actor puts max |z1| AND max |z2| inside [15, 30] on the case's own rows."""
    bt = LS.edge_batch("solo", 8, 130, "mixed")
    x = bt.obs[bt.idx[0]]
    ok = []
    for f in np.geomspace(1.0, 100.0, 200):
        pol = R.policy64(bt.ac_cls, 8, bt.theta(0))
        with torch.no_grad():
            pol.mlp_extractor.policy_net[0].weight.mul_(f)
            pol.mlp_extractor.policy_net[2].weight.mul_(f)
        z1, z2 = R.preactivations64(R.params64(pol), R.obs32(x))
        ok.append(all(E.Z_RANGE[0] <= np.abs(z).max() <= E.Z_RANGE[1] for z in (z1, z2)))
    assert not any(ok)


def test_cases_do_not_depend_on_the_global_generators():
    a = E.make(8, 65, "underflow", 5)
    torch.manual_seed(99)
    np.random.seed(99)
    b = E.make(8, 65, "underflow", 5)
    for name in ("obs", "act", "old_logp", "adv", "ret", "idx"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert np.array_equal(a.theta(), b.theta())
