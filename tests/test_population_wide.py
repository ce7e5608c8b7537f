"""K PPO learners at once at 16, 32 and 64 traffic aircraft: acas2d_collect_set_group_f32, acas2d_ppo_update_wide_set_f32
and the host classes over them (ACAS2DVecEnv.collect_set(group=True), ppo.FusedUpdateSet's `entry`,
ppo.PopulationTrainer(group=True)).  The recipes are tests/test_population.py's and tests/test_wide_update.py's.

  CPU  the two symbols and every rejection before a launch; the register / LDS guard of csrc/acas2d_ppo_wide_set.hip and the
       nine Mode::CollectSet kernels of the float32 unit; the host classes' choice of entry point.
  GPU  a group set collection equals K solo group collections bit for bit (and, at n_traffic = 8, the thread-per-env set
       collection); raw gradients and applied steps per member against the float64 references of tests/learner_ref.py with
       the bounds of tests/learner_support.py (the set kernel runs the solo body per member, so the solo bounds
       apply), and against the solo wide update bit for bit where there is one workgroup per network; isolation between
       members; the trainer's first iteration against K solo PPOTrainer runs; a few iterations with the callbacks.
Every criterion prints what it observed.

Observed tolerances: NOT YET RECORDED -- these tests have not run on a device yet.  The worst tau per test belongs here
(raw gradients per width, bound 2e-5; applied steps: parameter excess in lr, bound 1e-2, m / v tau, bounds 2e-5 / 5e-5,
norm / pg / vf, bound 1e-5; last values against float64, bound 5e-6) and in DESIGN.md 4.2e."""
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
GROUP_SET_TRAFFIC = (8, 16, 32, 64)    # the four group-cooperative work shapes (4,2) (4,4) (4,8) (4,16)
WIDE = (53, 101, 197)


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
def test_wide_set_entry_points_are_exported_and_declared(g):
    L = g.native.lib()
    for name in ("acas2d_collect_set_group_f32", "acas2d_ppo_update_wide_set_f32"):
        assert name in g.native.EXPORTS and getattr(L, name)
    header = re.sub(r"\s+", " ", open(os.path.join(H.ROOT, "include", "acas2d.h")).read())
    decl = lambda name: re.search(r"int %s\(([^)]*)\);" % name, header).group(1)  # noqa: E731
    assert decl("acas2d_collect_set_group_f32") == decl("acas2d_collect_set_f32")          # the sibling's signature
    assert decl("acas2d_ppo_update_wide_set_f32") == "const Acas2dPpoUpdateSet *u, void *stream"
    assert L.acas2d_abi_version() == g.native.ABI_VERSION == 7
    assert C.sizeof(g.native.CPpoUpdateSet) == 19 * 8 + 4 * 4 + 6 * 8


def test_collect_set_group_validation_needs_no_gpu(g):
    """acas2d_collect_set_group_f32 rejects every bad argument with ACAS2D_EINVAL and a message, before any launch (the
    pointers are host addresses: a launch would fail otherwise)."""
    L = g.native.lib()
    buf = (C.c_double * 8192)()
    a = C.addressof(buf)
    assert a % 16 == 0 or (a + 8) % 16 == 0
    a += a % 16                                            # 16-byte aligned
    st = g.native.CState(*([a] * 14))
    io = g.native.CStepIO(a, a, a, a, a, None, a, a)

    def ac(hidden=64, **over):
        f = {n: a for n, _ in g.native.CPolicy._fields_[:6]}
        f.update({k: v for k, v in over.items() if k in f})
        rest = {n: a for n in ("v1t", "vb1", "v2t", "vb2", "v3", "vb3", "log_std", "values", "logp")}
        rest.update({k: v for k, v in over.items() if k in rest})
        return g.native.CActorCritic(g.native.CPolicy(**f, hidden=hidden, _pad=0), **rest, noise_seed=0, noise_step=0, _pad=0)

    for N in GROUP_SET_TRAFFIC:
        cfg = g.ACAS2DConfig(n_traffic=N).to_c()

        def call(cfg_=C.byref(cfg), state=C.byref(st), io_=C.byref(io), p=None, K=3, seeds=a, obs=a, T=10, off=0, E=3 * 128,
                 n=N):
            return L.acas2d_collect_set_group_f32(cfg_, state, io_, C.byref(p) if p is not None else C.byref(ac()), K, seeds,
                                                  obs, T, 13, off, E, n, None)

        def rejects(msg, **kw):
            assert call(**kw) == -22, kw
            err = L.acas2d_last_error()
            assert msg.encode() in err and b"acas2d_collect_set_group" in err, (kw, err)

        rejects("NULL cfg", cfg_=None)
        rejects("NULL state", state=None)
        rejects("NULL cfg / io", io_=None)
        rejects("are required", obs=None)
        rejects("NULL noise_seeds", seeds=None)
        for name in ("w1t", "b1", "w2t", "b2", "w3", "b3"):
            rejects("six weight buffers", p=ac(**{name: None}))
        for name in ("v1t", "vb1", "v2t", "vb2", "v3", "vb3", "log_std", "values", "logp"):
            rejects("value net", p=ac(**{name: None}))
        for K in (0, -2):
            rejects("n_members = %d" % K, K=K)
        for E, K in ((448, 3), (300, 3), (64, 2), (127, 1), (192, 2)):
            rejects("not n_members = %d x a multiple of 64" % K, E=E, K=K)
        for narrow in (1, 2, 3, 4):                        # sent to the sibling by name
            rejects("use acas2d_collect_set_f32", n=narrow)
        rejects("n_traffic = 0", n=0)
        for badN in (5, 12):
            rejects("built for n_traffic in {8, 16, 32, 64}", n=badN)
        for name in ("w1t", "b1", "w2t", "b2", "v1t", "vb1", "v2t", "vb2"):
            rejects("16-byte aligned", p=ac(**{name: a + 4}))
        rejects("n_steps = 0", T=0)
        rejects("negative", off=-1)
    assert L.acas2d_collect_set_group_f32(None, None, None, None, 0, None, None, 0, 0, 0, 0, 0, None) == -22
    # the sibling keeps rejecting the wide counts, and now names this entry
    cfg = g.ACAS2DConfig(n_traffic=16).to_c()
    assert L.acas2d_collect_set_f32(C.byref(cfg), C.byref(st), C.byref(io), C.byref(ac()), 3, a, a, 10, 13, 0, 384, 16, None) == -22
    assert b"acas2d_collect_set_group_f32" in L.acas2d_last_error()


def test_update_wide_set_validation_needs_no_gpu(g):
    """acas2d_ppo_update_wide_set_f32 rejects every bad argument before its first launch."""
    L = g.native.lib()
    buf = (C.c_double * 64)()
    a = C.addressof(buf)
    names = [n for n, _ in g.native.CPpoUpdateSet._fields_]
    ints = dict(n_members=3, n_rows=64, obs_dim=53, apply=0)

    def call(**kw):
        return L.acas2d_ppo_update_wide_set_f32(*LS.host_update_set_args(g, a, **{**ints, **kw}))

    def rejects(msg, **kw):
        assert call(**kw) == -22, kw
        err = L.acas2d_last_error()
        assert msg.encode() in err and b"acas2d_ppo_update_wide_set" in err, (kw, err)

    for n in names:
        if n not in ints:
            rejects("every pointer is required", **{n: None})
    for K in (0, -1, 65536):
        rejects("n_members = %d" % K, n_members=K)
    for B in (1, 0, -5):
        rejects("n_rows = %d" % B, n_rows=B)
    for D in (0, 8, 29, 52, 54, 100, 198):
        rejects("obs_dim = %d" % D, obs_dim=D)
        assert b"obs_dim 53, 101, 197" in L.acas2d_last_error()
    for D in (8, 29):                                      # the narrow widths are sent to the sibling by name
        rejects("use acas2d_ppo_update_set_f32", obs_dim=D)
    assert L.acas2d_ppo_update_wide_set_f32(None, None) == -22 and b"NULL argument" in L.acas2d_last_error()


@H.needs_hipcc
def test_wide_set_update_kernels_stay_in_registers_and_lds(g, tmp_path):
    """csrc/acas2d_ppo_wide_set.hip: three gradient kernels of 256 threads (the apply kernel is acas2d_ppo_set.hip's), no
    VGPR or SGPR spill, no scratch, and acas2d_ppo_wide_lds_bytes -- the figure the launch uses -- plus the kernel's static
    LDS within gfx950's 160 KB per workgroup.  acas2d_ppo_set.hip still holds six kernels with launch_ppo_apply_set in it."""
    _, kernels = H.kernel_metadata(tmp_path, "acas2d_ppo_wide_set.hip")
    assert len(kernels) == 3
    L = g.native.lib()
    static = {}
    for k in kernels:
        name = k.name
        assert "ppo_grad_wide_set_kernel" in name
        assert k.field("vgpr_spill_count") == 0 and k.field("sgpr_spill_count") == 0, name
        assert k.field("private_segment_fixed_size") == 0 and k.field("vgpr_count") <= 256, name
        assert k.field("max_flat_workgroup_size") == 256, name
        static[int(re.search(r"kernelILi(\d+)E", name).group(1))] = k.field("group_segment_fixed_size")
        print(name, "vgpr", k.field("vgpr_count"), "sgpr", k.field("sgpr_count"))
    assert sorted(static) == list(WIDE)
    for D in WIDE:
        lds = L.acas2d_ppo_wide_lds_bytes(D)
        assert (4 * 64 * 65 + 64 * D) * 4 <= lds and lds + static[D] <= 160 * 1024, (D, lds, static[D])
        print("D = %d: %d bytes of dynamic LDS + %d static" % (D, lds, static[D]))
    assert len(H.kernel_metadata(tmp_path, "acas2d_ppo_set.hip")[1]) == 6


@H.needs_hipcc
def test_set_collector_is_nine_float32_kernels(tmp_path):
    """Mode::CollectSet (value 7) in the float32 unit: the five (C,1) shapes and the four group shapes, each without a VGPR
    spill or a private segment and under the unit's 400 SGPR spills; their registers beside Mode::Collect's (value 5) at
    the same shapes."""
    _, kernels = H.kernel_metadata(tmp_path, "acas2d_f32.hip")
    by_mode = {5: {}, 7: {}}
    for k in kernels:
        m = re.match(r"_ZN6acas2d11step_kernelIfLi(\d+)ELi(\d+)ELb1ELb1ELNS_4ModeE([57])EEEv", k.name)
        if m:
            by_mode[int(m.group(3))][(int(m.group(1)), int(m.group(2)))] = k
    assert len([k for k in kernels if "ModeE7EEEv" in k.name]) == 9
    assert sorted(by_mode[7]) == sorted([(1, 1), (2, 1), (3, 1), (4, 1), (8, 1), (4, 2), (4, 4), (4, 8), (4, 16)])
    for shape, k in sorted(by_mode[7].items()):
        solo = by_mode[5][shape]
        print("shape %s: CollectSet vgpr %d sgpr %d sgpr spills %d | Collect vgpr %d sgpr %d sgpr spills %d"
              % (shape, k.field("vgpr_count"), k.field("sgpr_count"), k.field("sgpr_spill_count"),
                 solo.field("vgpr_count"), solo.field("sgpr_count"), solo.field("sgpr_spill_count")))
        assert k.field("vgpr_spill_count") == 0 and k.field("private_segment_fixed_size") == 0, shape
        assert k.field("sgpr_spill_count") < 400, shape


def test_host_classes_pick_the_wide_set_entries(g):
    """Nothing is launched: FusedUpdateSet on CPU tensors names its entry by width, and PopulationTrainer(group=True) on a
    stub env passes its config rules at 8 / 16 / 32 / 64 (construction gets as far as the stub's missing reset())."""
    for D, entry in ((53, "acas2d_ppo_update_wide_set_f32"), (101, "acas2d_ppo_update_wide_set_f32"),
                     (197, "acas2d_ppo_update_wide_set_f32"), (29, "acas2d_ppo_update_set_f32")):
        pset = g.ActorCriticSet(2, D)
        z = torch.zeros(8, D), torch.zeros(8), torch.zeros(8), torch.zeros(8), torch.zeros(8)
        fu = g.FusedUpdateSet(pset, [g.PPOConfig(), g.PPOConfig()], *z)
        assert fu.entry == entry and fu.grad.shape == (2, 2 * (64 * D + 64 + 64 * 64 + 64 + 64 + 1) + 1)
    with pytest.raises(ValueError, match=r"8, 11, 14, 17, 29.*53, 101, 197"):
        g.FusedUpdateSet(g.ActorCriticSet(2, 30), [g.PPOConfig()] * 2, torch.zeros(8, 30), *[torch.zeros(8)] * 4)
    venv = lambda **kw: types.SimpleNamespace(**{**dict(dtype=torch.float32, n_traffic=16, obs_dim=53, num_envs=3 * 64, device="cpu"), **kw})  # noqa: E731
    cfgs = [g.PPOConfig(seed=13 + k, learning_rate=(1e-4, 3e-4, 1e-3)[k], gamma=(0.99, 0.98, 0.999)[k]) for k in range(3)]
    for N in GROUP_SET_TRAFFIC:
        with pytest.raises(AttributeError, match="reset"):
            g.PopulationTrainer(venv(n_traffic=N, obs_dim=5 + 3 * N), cfgs, group=True)
    for N in (1, 4, 5):
        with pytest.raises(ValueError, match="n_traffic"):
            g.PopulationTrainer(venv(n_traffic=N, obs_dim=5 + 3 * N), cfgs, group=True)
    with pytest.raises(ValueError, match="float32"):
        g.PopulationTrainer(venv(dtype=torch.float64), cfgs, group=True)
    with pytest.raises(ValueError, match="group=True"):    # without it the wide counts stay rejected, and say how
        g.PopulationTrainer(venv(), cfgs)


# ---- GPU: the collector ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("config", ("default", "small"))
@pytest.mark.parametrize("EM", (64, 192))
@pytest.mark.parametrize("N", GROUP_SET_TRAFFIC)
def test_collect_set_group_equals_solo_group_collections_bitwise(gpu, N, EM, config):
    """One acas2d_collect_set_group_f32 launch for K = 3 distinct actor-critics and noise keys against three solo
    collect(group=True) launches on envs of EM envs at env_offset + k EM: all nine outputs, obs[T] and the state left
    behind, compared as bit patterns.  T runs past max_steps, so every env of every member is reset inside the launch.
    EM = 64 at N = 8 puts a member boundary inside a workgroup (a wave holds 32 envs); at N = 64 a member is 16 waves."""
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
    out = env.collect_set(pset, T, seeds, noise_step=7, group=True)
    torch.cuda.synchronize()
    for k in range(K):
        solo = g.ACAS2DVecEnv(EM, N, device=DEV, seed=21, env_offset=off + k * EM, config=cfg)
        solo.reset()
        ref = solo.collect(pols[k], T, noise_seed=seeds[k], noise_step=7, group=True)
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
        print("member %d: %d episodes ended inside the launch" % (k, int(resets.sum())))
    assert not H.bits_equal(out["actions"][:, :EM], out["actions"][:, EM:2 * EM])         # the members really differ


@pytest.mark.gpu
@pytest.mark.parametrize("EM", (64, 192))
def test_collect_set_group_equals_thread_per_env_set_at_8(gpu, EM):
    """n_traffic = 8 is where both set collectors exist: same env, same members, the same bits in every output and in
    the state."""
    g = gpu
    K, N, T = 3, 8, 60
    pols = LS.members(g, 5 + 3 * N, K)
    pset = g.ActorCriticSet.from_members(pols)
    runs = []
    for group in (True, False):
        env = g.ACAS2DVecEnv(K * EM, N, device=DEV, seed=21, env_offset=37, config=g.ACAS2DConfig(n_traffic=N, max_steps=25))
        env.reset()
        runs.append((env, env.collect_set(pset, T, [5, 6, 7], noise_step=3, group=group)))
    torch.cuda.synchronize()
    (ea, a), (eb, b) = runs
    for name in LS.OUTPUTS + ("obs",):
        assert H.bits_equal(a[name], b[name]), name
    for name in LS.STATE:
        assert H.bits_equal(getattr(ea, name), getattr(eb, name)), name
    assert H.bits_equal(ea.outputs["obs"], eb.outputs["obs"])
    assert int(a["done"].sum(0).min()) >= 1
    print("EM = %d: %d episodes ended, both collectors agree in every bit" % (EM, int(a["done"].sum())))


@pytest.mark.gpu
@pytest.mark.parametrize("N", (16, 64))
def test_collect_set_group_routes_each_member_to_its_own_rows(gpu, N):
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
    out = env.collect_set(g.ActorCriticSet.from_members(pols), T, [1, 2, 3], group=True)
    a = out["actions"]
    assert bool((a[:, :EM] > 40).all()) and bool((a[:, EM:2 * EM] < -40).all()) and bool((a[:, 2 * EM:].abs() < 10).all())
    twin = g.ACAS2DVecEnv(K * EM, N, device=DEV, seed=3)
    twin.reset()
    psi0 = twin.own_psi.clone()
    o, _, done, _ = twin.step(a[0].clamp(-1, 1))
    assert H.bits_equal(o, out["obs"][1]) and H.bits_equal(done, out["done"][0])
    live = ~done
    print("N=%d: %d of %d envs ended their episode in the first step" % (N, int(done.sum()), K * EM))
    # (at 64 traffic aircraft in the default airspace most episodes end by collision in their first step -- 300 of 384 here
    # -- so the turn is read on the envs that are left: it is deterministic, "all of them" needs only that there are some)
    assert int(live[:EM].sum()) >= 8 and int(live[EM:2 * EM].sum()) >= 8, (int(live[:EM].sum()), int(live[EM:2 * EM].sum()))
    d = (twin.own_psi - psi0 + 540) % 360 - 180
    assert bool((d[:EM][live[:EM]] > 0).all()) and bool((d[EM:2 * EM][live[EM:2 * EM]] < 0).all())


# ---- GPU: the update ---------------------------------------------------------------------------------------------------
GRAD_CASES = [(D, B) for D in WIDE for B in (2, 65, 129, 2085)] + [(197, 4096)]


@pytest.mark.gpu
@pytest.mark.parametrize("D,B", GRAD_CASES, ids=["D%d-B%d" % c for c in GRAD_CASES])
def test_update_wide_set_raw_gradients_per_member_vs_float64(gpu, D, B):
    """apply = 0: the gradient launch alone, K = 3 members with different parameters, clip_range 0.1 / 0.2 / 0.3 and
    vf_coef 0.5 / 0.25 / 1.0 on disjoint rows of ONE shared buffer.  Every member's 13 tensors against ppo_loss() in
    float64 autograd (learner_ref.grad64), both old_logp modes; criterion and bounds of test_learner_kernels.py."""
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
        assert fu.entry == "acas2d_ppo_update_wide_set_f32"
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


APPLY_CASES = [(D, B) for D in WIDE for B in (65, 2085)]


@pytest.mark.gpu
@pytest.mark.parametrize("D,B", APPLY_CASES, ids=["D%d-B%d" % c for c in APPLY_CASES])
def test_update_wide_set_applied_steps_per_member_vs_float64(gpu, D, B):
    """Two applied steps of K = 4 members with the roles of test_update_set_applied_steps_per_member_vs_float64: clip
    active / inactive, a late step with non-zero moments, and a learning_rate-0 member that keeps every parameter bit.
    Each reference step (learner_ref.grad64 + adam64) starts from the kernel's OWN parameters, moments and step count."""
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


BITWISE_CASES = [(D, B) for D in WIDE for B in (2, 63, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("D,B", BITWISE_CASES, ids=["D%d-B%d" % c for c in BITWISE_CASES])
def test_update_wide_set_single_workgroup_equals_solo_bitwise(gpu, D, B):
    """The set kernel and the solo wide kernel run ONE body (csrc/acas2d_ppo_wide.hpp: grad_wide), so where the result does
    not depend on the order of the atomics it is the same bits: with B <= 64 there is one workgroup per network, and each
    gradient entry receives exactly one atomic add from exactly one of its four waves.  K = 3 members with different
    weights, minibatches, hyper-rows and Adam step counts through FusedUpdateSet; the same member by member through
    FusedUpdate (acas2d_ppo_update_wide_f32).  First the raw gradient, then three applied steps, compared after each:
    grad, the 13 parameters, m, v, step_count, stats[2] / [4] / [5] with torch.equal."""
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
    assert fs.entry == "acas2d_ppo_update_wide_set_f32"
    fs.step(idx, apply=False)
    for k in range(K):
        fu = g.FusedUpdate(solo[k], probes[k], *bufs)
        assert fu.entry == "acas2d_ppo_update_wide_f32"
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
    print("D=%d B=%d: set and solo wide updates agree in every bit over the raw gradient and three applied steps" % (D, B))


@pytest.mark.gpu
def test_update_wide_set_writes_only_its_members_rows(gpu):
    """D = 197, B = 129, K = 3, with grad / adam_m / adam_v / stats / adam_step handed over as the middle K rows of
    K + 2-row tensors filled with a sentinel: the outer rows keep it through a raw-gradient call and an applied step.
    Member 1's advantages are one constant (2.0: every partial sum is exact, so the normalised advantage is exactly 0):
    its actor gradient and log_std gradient are exactly 0 while its critic's and its neighbours' are not."""
    g = gpu
    D, B, K = 197, 129, 3
    n = K * B + 317
    bt = LS.RolloutBatch(g, D, K, n, seed=77)
    pset = bt.policy_set()
    idx = torch.randperm(n, device=DEV)[:K * B].reshape(K, B).contiguous()
    bt.adv[idx[1]] = 2.0
    for k in range(K):
        bt.set_old_logp(LS.theta_of(pset, k), idx[k], "mixed", 0.2)
    cfgs = [g.PPOConfig(ent_coef=0.0, learning_rate=(3e-4, 1e-3, 1e-4)[k]) for k in range(K)]
    fu = g.FusedUpdateSet(pset, cfgs, bt.obs, bt.act, bt.old_logp, bt.adv, bt.ret)
    W = fu.grad.shape[1]
    SENT_F, SENT_I = -12345.5, -777
    big = {name: torch.full((K + 2, width), SENT_F, dtype=torch.float32, device=DEV)
           for name, width in (("grad", W), ("m", W), ("v", W), ("stats", 8))}
    big_step = torch.full((K + 2,), SENT_I, dtype=torch.int32, device=DEV)
    for name in big:
        big[name][1:K + 1].zero_()
        setattr(fu, name, big[name][1:K + 1])
    big_step[1:K + 1] = 0
    fu.step_count = big_step[1:K + 1]
    assert fu.grad.is_contiguous() and fu.grad.data_ptr() == big["grad"].data_ptr() + 4 * W

    def outer_rows_untouched():
        for name, t in big.items():
            assert bool((t[0] == SENT_F).all()) and bool((t[K + 1] == SENT_F).all()), name
        assert big_step[0].item() == SENT_I and big_step[K + 1].item() == SENT_I

    fu.step(idx, apply=False)
    torch.cuda.synchronize()
    outer_rows_untouched()
    net = 64 * D + 64 + 64 * 64 + 64 + 64 + 1
    actor = lambda k: torch.cat([fu.grad[k, :net], fu.grad[k, 2 * net:]])  # noqa: E731  (the actor's block and log_std)
    assert float(actor(1).abs().max()) == 0.0
    assert float(fu.grad[1, net:2 * net].abs().max()) > 0.0
    assert float(actor(0).abs().max()) > 0.0 and float(actor(2).abs().max()) > 0.0
    print("constant advantages: member 1's actor gradient is exactly 0, its neighbours' max |g| %.3e / %.3e"
          % (float(actor(0).abs().max()), float(actor(2).abs().max())))
    fu.grad.zero_()
    fu.stats.zero_()
    fu.step(idx)
    torch.cuda.synchronize()
    outer_rows_untouched()
    assert fu.step_count.cpu().tolist() == [1, 1, 1] and float(fu.m.abs().max()) > 0.0


@pytest.mark.gpu
def test_update_wide_set_hyper_row_reaches_only_what_it_enters(gpu):
    """D = 197, B = 64 (one workgroup per network: fixed bits).  Members 0 and 2 hold the same weights and the same rows
    and differ in vf_coef (0.5 / 1.0), ent_coef, max_grad_norm and learning_rate: the raw actor gradient, the log_std
    gradient and both loss sums agree bit for bit, and member 2's critic gradient is member 0's times two, exactly (the
    factor enters d loss / d value as a power of two)."""
    g = gpu
    D, B, K = 197, 64, 3
    n = 2 * B + 100
    bt = LS.RolloutBatch(g, D, K, n, seed=91)
    pset = bt.policy_set()
    for name in R.PARAM_NAMES:
        pset.params[name][2].copy_(pset.params[name][0])
    rows = torch.randperm(n, device=DEV)[:2 * B].reshape(2, B)
    idx = torch.stack([rows[0], rows[1], rows[0]]).contiguous()
    bt.set_old_logp(LS.theta_of(pset, 0), idx[0], "mixed", 0.2)
    bt.set_old_logp(LS.theta_of(pset, 1), idx[1], "mixed", 0.2)
    cfgs = [g.PPOConfig(clip_range=0.2, vf_coef=(0.5, 0.25, 1.0)[k], ent_coef=(0.0, 0.01, 0.02)[k],
                        max_grad_norm=(0.5, 1e6, 0.3)[k], learning_rate=(3e-4, 1e-3, 1e-4)[k]) for k in range(K)]
    fu = g.FusedUpdateSet(pset, cfgs, bt.obs, bt.act, bt.old_logp, bt.adv, bt.ret)
    fu.step(idx, apply=False)
    torch.cuda.synchronize()
    net = 64 * D + 64 + 64 * 64 + 64 + 64 + 1
    assert float(fu.grad[0, :net].abs().max()) > 0.0
    assert torch.equal(fu.grad[0, :net], fu.grad[2, :net]) and torch.equal(fu.grad[0, 2 * net:], fu.grad[2, 2 * net:])
    assert torch.equal(fu.stats[0, 0:2], fu.stats[2, 0:2])
    assert torch.equal(fu.grad[0, net:2 * net] * 2.0, fu.grad[2, net:2 * net])
    assert not torch.equal(fu.grad[0, :net], fu.grad[1, :net])
    print("hyper rows: actor gradient and losses of the twin members agree in every bit; critic gradient x 2 exactly")


# ---- GPU: the trainer --------------------------------------------------------------------------------------------------
def _population(g, N, K, EM, T, group, gae=None, batch=1024, max_steps=15):
    cfgs = [g.PPOConfig(seed=13 + k, learning_rate=(1e-4, 3e-4, 1e-3)[k], gamma=(0.99, 0.98, 0.999)[k],
                        gae_lambda=(0.95, 0.9, 0.97)[k], n_steps=T, batch_size=batch, n_epochs=2) for k in range(K)]
    ecfg = g.ACAS2DConfig(n_traffic=N, max_steps=max_steps)           # short episodes: dones inside the first collection
    venv = g.ACAS2DVecEnv(K * EM, N, device=DEV, seed=13, config=ecfg)
    return g.PopulationTrainer(venv, cfgs, gae=gae, **({"group": True} if group else {})), cfgs, ecfg


_BUFFERS = ("b_obs", "b_act", "b_logp", "b_val", "b_rew", "b_done")


@pytest.mark.gpu
@pytest.mark.parametrize("N", (16, 64))
def test_wide_population_first_iteration_equals_solo_trainers(gpu, N):
    """K = 3 members with different seeds, learning rates and gamma / lambda, EM = 64: the buffers of the first collection
    equal three solo PPOTrainer(collector="fused", updater="fused") on env_offset = k EM bit for bit, GAE equals
    compute_gae on the member's own columns, the last values are the critics', and gae="kernel" gives "torch"'s bits."""
    g = gpu
    K, EM, T = 3, 64, 24
    pop, cfgs, ecfg = _population(g, N, K, EM, T, group=True)
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
        for name in _BUFFERS:
            assert H.bits_equal(getattr(pop, name)[:, cols], getattr(tr, name)), (k, name)
        assert bool(pop.b_done[:, cols].any())
        gk, lk = (torch.tensor(v, dtype=torch.float32, device=DEV) for v in (cfgs[k].gamma, cfgs[k].gae_lambda))
        adv, ret = g.compute_gae(pop.b_rew[:, cols], pop.b_val[:, cols], pop.b_done[:, cols], pop.last_value[cols], gk, lk)
        assert H.bits_equal(pop.b_adv[:, cols], adv) and H.bits_equal(pop.b_ret[:, cols], ret), k
        _, v64 = R.forward64(R.params64(pop.member(k)), pop.obs[cols].double().cpu().numpy(), sample=True)
        got = pop.last_value[cols].double().cpu().numpy()
        rel = float((np.abs(got - v64) / np.maximum(1.0, np.abs(v64))).max())
        print("member %d: last values within %.2e of float64 (bound 5e-6)" % (k, rel))
        assert rel <= 5e-6
    assert pop.num_timesteps == T * EM
    popk, _, _ = _population(g, N, K, EM, T, group=True, gae="kernel")
    popk.collect()
    torch.cuda.synchronize()
    for name in _BUFFERS + ("b_adv", "b_ret", "last_value"):
        assert H.bits_equal(getattr(popk, name), getattr(pop, name)), name
    print("N=%d: gae='kernel' gives the bits of gae='torch'" % N)


@pytest.mark.gpu
def test_population_at_8_is_the_same_with_and_without_group(gpu):
    """n_traffic = 8 trains either way: PopulationTrainer(group=True) and PopulationTrainer() fill identical buffers."""
    g = gpu
    a, _, _ = _population(g, 8, 3, 64, 24, group=True)
    b, _, _ = _population(g, 8, 3, 64, 24, group=False)
    assert a.group and not b.group
    a.collect()
    b.collect()
    torch.cuda.synchronize()
    for name in _BUFFERS + ("b_adv", "b_ret", "last_value", "obs"):
        assert H.bits_equal(getattr(a, name), getattr(b, name)), name
    assert bool(a.b_done.any())


@pytest.mark.gpu
def test_wide_population_learns_a_few_iterations_with_callbacks(gpu, tmp_path):
    g = gpu
    K, EM, N, T, batch = 3, 64, 16, 32, 1024
    cfgs = [g.PPOConfig(seed=13 + k, learning_rate=(1e-4, 3e-4, 1e-3)[k], n_steps=T, batch_size=batch, n_epochs=2)
            for k in range(K)]
    venv = g.ACAS2DVecEnv(K * EM, N, device=DEV, seed=13, config=g.ACAS2DConfig(n_traffic=N, max_steps=40))
    pop = g.PopulationTrainer(venv, cfgs, group=True)
    start = [{n: pop.policy_set.params[n][k].clone() for n in R.PARAM_NAMES} for k in range(K)]
    per_it, iters, n_eval = T * EM, 3, 10
    hist = pop.learn(iters * per_it, log=None, eval_every=per_it, eval_episodes=n_eval, eval_seed=99, save_dir=str(tmp_path),
                     checkpoint_every=per_it)
    assert pop._fused_update.entry == "acas2d_ppo_update_wide_set_f32"
    assert pop.num_timesteps == iters * per_it
    train = [r for r in hist if not r.get("eval")]
    evals = [r for r in hist if r.get("eval")]
    assert sorted((r["member"], r["iteration"]) for r in train) == [(k, i) for k in range(K) for i in range(1, iters + 1)]
    assert len(evals) == K * iters and hist is pop.history
    for r in train:
        assert np.isfinite([r["pg_loss"], r["value_loss"], r["std"]]).all() and r["timesteps"] == r["iteration"] * per_it
    assert pop.optimizer_state()["step"] == [iters * 2 * (per_it // batch)] * K
    for k in range(K):
        for n in R.PARAM_NAMES:
            assert bool(torch.isfinite(pop.policy_set.params[n][k]).all()), (k, n)
        moved = max(float((pop.policy_set.params[n][k] - start[k][n]).abs().max()) for n in R.PARAM_NAMES)
        print("member %d: parameters moved by up to %.3e" % (k, moved))
        assert moved > 1e-4, (k, moved)
    for a, b in ((0, 1), (1, 2), (0, 2)):
        assert not torch.equal(pop.policy_set.params[R.PARAM_NAMES[2]][a], pop.policy_set.params[R.PARAM_NAMES[2]][b])
    # the files, member by member
    rng = random.Random(99)
    episodes = [g.reset_parity.draw_episodes(venv.config, n_eval, rng) for _ in range(iters)]
    own, trf, goal = episodes[-1]
    final = g.evaluate_policies_fused(pop.policy_set.actor_weights(), own, trf, goal, dtype=torch.float32, device=DEV,
                                      config=venv.config, group=True)
    for k in range(K):
        d = tmp_path / ("member_%d" % k)
        ev = np.load(d / "results" / "evaluations.npz")
        assert ev["timesteps"].tolist() == [per_it * (i + 1) for i in range(iters)]
        assert ev["results"].shape == (iters, n_eval) and ev["ep_lengths"].shape == (iters, n_eval)
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
