"""What the tests of the fused PPO update share (a plain module: not a test file, not a conftest; the package never
imports it): the bounds and the per-tensor criterion, the rollout buffer and its members, the hyper-parameter table and the
minibatch draws, the admitted edge batches on the device, the host-address structs of the validation tests, the trainer
helpers and the collector tests' policies.  The float64 mathematics stays in learner_ref.py, kl_guard_ref.py,
sb3_options_ref.py and edge_minibatches.py."""
import ctypes as C

import numpy as np
import pytest

import edge_minibatches as E
import kl_guard_ref as KR
import learner_ref as R

torch = pytest.importorskip("torch")
DEV = "cuda:0"

# ---- the bounds and the criterion -------------------------------------------------------------------------------------
# raw gradient, per tensor: max |got - ref| <= TAU * max |ref tensor| + TAU0 * max |ref, all 13 tensors|
# (observed at most 2.1e-6 over every case of tests/test_learner_kernels.py: tau 2e-5 leaves 10x headroom, and is 10x
# tighter than the global 2e-4 of test_fused_update_against_torch_autograd_and_adam)
TAU, TAU0 = 2e-5, 1e-6
# moments after a step, per tensor with the same tau0: m (observed within the tau0 term) and v -- the kernel's 0.999f
# makes its 1 - beta2 1.3e-5 relative off the reference's (observed 1.4e-5)
TAU_M, TAU_V = 2e-5, 5e-5


def worst_ratio(errs, ref_all, tau0=TAU0):
    """max over tensors of (max |diff| - tau0 max |ref_all|) / max |ref tensor|: the per-tensor criterion's tau."""
    return max((e - tau0 * ref_all) / max(m, 1e-300) for e, m in errs.values())


def assert_per_tensor(what, got, ref, segs, tau, tau0=TAU0):
    """The criterion; prints and returns the tau it observed."""
    errs, ref_all = R.per_tensor_errors(got, ref, segs)
    bad = {n: (e, m) for n, (e, m) in errs.items() if not e <= tau * m + tau0 * ref_all}
    obs = worst_ratio(errs, ref_all, tau0)
    print("%s: observed tau %.2e (bound %.0e, tau0 %.0e)" % (what, obs, tau, tau0))
    assert not bad, (what, bad, ref_all)
    return obs


# ---- members and the rollout buffer -----------------------------------------------------------------------------------
def members(g, D, K, seed=1, scale=40.0, device=DEV):
    """K actor-critics away from SB3's near-zero head (ratios spread, some clip; actions that steer), with different
    log-stds."""
    out = []
    for k in range(K):
        torch.manual_seed(seed + 17 * k)
        pol = g.ActorCritic(D).to(device)
        with torch.no_grad():
            pol.action_net.weight.mul_(scale)
            pol.log_std.fill_(-0.7 + 0.2 * k)
        out.append(pol)
    return out


def actor_critic(g, D, seed=1, device=DEV):
    return members(g, D, 1, seed, device=device)[0]


def theta_of(pset, k):
    """Member k's flat float64 parameters (PARAM_NAMES order) out of an ActorCriticSet."""
    return torch.cat([pset.params[n][k].reshape(-1) for n in R.PARAM_NAMES]).double().cpu().numpy()


class RolloutBatch:
    """One flat rollout buffer of n rows on `device` (the kernels gather a minibatch by idx, a random subset), shared by K
    members with different parameters."""

    def __init__(self, g, D, K, n, seed, device=DEV):
        rng = np.random.default_rng(seed)
        self.g, self.rng, self.D, self.K, self.n, self.device = g, rng, D, K, n, device
        f = lambda a: torch.as_tensor(np.asarray(a, np.float32), device=device).contiguous()  # noqa: E731
        self.obs = f(rng.uniform(-1, 1, (n, D)))
        self.act = f(rng.normal(0, 0.7, n))
        self.adv, self.ret = f(rng.normal(0, 2, n)), f(rng.normal(2, 3, n))     # (value offset: gradient norm > 0.5 at any B)
        self.old_logp = torch.zeros(n, dtype=torch.float32, device=device)
        self.pols = members(g, D, K, seed, device=device)
        self.bufs = (self.obs, self.act, self.old_logp, self.adv, self.ret)

    def policy_set(self):
        """A fresh ActorCriticSet holding copies of the members as constructed (twins start from the same bits)."""
        return self.g.ActorCriticSet.from_members(self.pols)

    def host(self, rows):
        i = rows.cpu().numpy()
        return [t.cpu().numpy().astype(np.float64)[i] for t in self.bufs]

    def _logp(self, theta, i):
        return R.logp64(self.g.ActorCritic, self.D, theta, self.obs.cpu().numpy()[i], self.act.cpu().numpy()[i])

    def set_old_logp(self, theta, rows, mode, clip):
        """old_logp of `rows` (None: the whole buffer) for the member with parameters `theta`: "mixed" its float64 log-prob
        plus N(0, 0.5) noise -- ratios on both sides of the clip range; "first" the log-prob itself (a first-epoch
        minibatch: ratio ~ 1, surr1 == surr2).  Ratios within 1e-4 of a clip edge are moved off it (float32 and float64
        would take different branches there).  Returns how many were."""
        i = slice(None) if rows is None else rows.cpu().numpy()
        lp = self._logp(theta, i)
        old = lp + (self.rng.normal(0, 0.5, len(lp)) if mode == "mixed" else 0.0)
        old, moved = E.nudge_off_edges(lp, old.astype(np.float32).astype(np.float64), clip)
        self.old_logp[i if rows is None else rows] = torch.as_tensor(old, device=self.device)
        return moved

    def nudge_off_edges(self, theta, clip):
        """set_old_logp's edge rule over the whole buffer for the CURRENT parameters (an applied step moves the ratios)."""
        old, moved = E.nudge_off_edges(self._logp(theta, slice(None)), self.old_logp.cpu().numpy().astype(np.float64), clip)
        if moved:
            self.old_logp.copy_(torch.as_tensor(old, device=self.device))

    def log_ratio(self, theta, rows):
        obs, act, old, _, _ = self.host(rows)
        return KR.log_ratio64(self.g.ActorCritic, self.D, theta, obs, act, old)


class SoloBatch(RolloutBatch):
    """The buffer with one member, `pol`, whose old log-probs are set over the whole buffer from its current parameters."""

    def __init__(self, g, D, n, seed, device=DEV):
        super().__init__(g, D, 1, n, seed, device)
        self.pol, self.ac_cls = self.pols[0], g.ActorCritic

    def set_old_logp(self, mode, clip):
        return super().set_old_logp(R.flat_params(self.pol), None, mode, clip)

    def nudge_off_edges(self, clip):
        super().nudge_off_edges(R.flat_params(self.pol), clip)


# ---- the configs and the draws ----------------------------------------------------------------------------------------
HYPER = dict(clip_range=(0.2, 0.1, 0.3), vf_coef=(0.5, 0.25, 1.0), ent_coef=(0.01, 0.0, 0.02),
             max_grad_norm=(0.5, 1e6, 0.5), learning_rate=(3e-4, 1e-3, 1e-4))


def member_cfgs(g, K, per_member=(), **over):
    """K configs with different clip ranges, learning rates, ... (member 0 has the entropy term and an active norm clip);
    `over` for all of them, per_member[k] member k's own."""
    return [g.PPOConfig(**{**{f: v[k] for f, v in HYPER.items()}, **over, **(per_member[k] if per_member else {})})
            for k in range(K)]


def device_rows(bt, K, B):
    """K x B disjoint rows of the buffer from torch's generator on the device."""
    return torch.randperm(bt.n, device=bt.device)[:K * B].reshape(K, B).contiguous()


def host_rows(bt, K, B):
    """K x B disjoint rows of the buffer, drawn on the host from the batch's own generator: the same on every machine."""
    return torch.as_tensor(bt.rng.permutation(bt.n)[:K * B].reshape(K, B), device=bt.device).contiguous()


def draw(bt, pset, clips, B, mode="mixed", rows=device_rows):
    """A fresh minibatch per member on disjoint rows, old log-probs from each member's CURRENT parameters, ratios kept
    1e-4 off the clip range given per member."""
    idx = rows(bt, len(clips), B)
    for k, clip in enumerate(clips):
        bt.set_old_logp(theta_of(pset, k), idx[k], mode, clip)
    return idx


# ---- the admitted edge batches (tests/edge_minibatches.py) on the device -------------------------------------------------
LR = 3e-4
PAD, SENT = 4096, -7.25
_edge_batches = {}


def edge_batch(kind, D, B, case):
    """The batch tests/test_edge_minibatches.py admits for this case, built once per session and never written to."""
    key = (kind, D, B, case)
    if key not in _edge_batches:
        _edge_batches[key] = E.make(D, B, case, E.seed_of(D, B, case), **(E.SET_LAYOUT if kind == "set" else {}))
    return _edge_batches[key]


def dev(a):
    return torch.as_tensor(a, device=DEV).contiguous()


def device_bufs(bt):
    return [dev(a) for a in (bt.obs, bt.act, bt.old_logp, bt.adv, bt.ret)]


def device_policy(g, bt, k=0):
    """A device copy of member k's policy (the batch's own stays as admitted)."""
    pol = g.ActorCritic(bt.D)
    pol.load_state_dict(bt.pols[k].state_dict())
    return pol.to(DEV)


def n_actor(segs):
    return segs[5][2]                 # the 6 actor tensors come first in the flat layout


def check_losses(what, st0, st1, pg, vf):
    print("  %s: pg %.6e vs %.6e, vf %.6e vs %.6e" % (what, st0, pg, st1, vf))
    assert abs(st0 - pg) <= 1e-5 * max(1.0, abs(pg)) and abs(st1 - vf) <= 1e-5 * max(1.0, vf), (what, st0, pg, st1, vf)


def check_applied(what, segs, theta1, m1, v1, theta_ref, m_ref, v_ref, lr, tau_v=None):
    """The bounds of test_fused_update_applied_steps_vs_float64 on one member's state after a step."""
    assert_per_tensor("m " + what, m1, m_ref, segs, TAU_M)
    assert_per_tensor("v " + what, v1, v_ref, segs, TAU_V if tau_v is None else tau_v)
    ulp = np.spacing(np.abs(theta_ref).astype(np.float32)).astype(np.float64)
    excess = float(((np.abs(theta1 - theta_ref) - ulp) / lr).max())
    print("  %s: parameter excess %.2e lr (bound 1e-2)" % (what, excess))
    assert excess <= 1e-2, (what, excess)


def carve(shape, dtype=torch.float32, sent=SENT, init=None):
    """A tensor of `shape` that is the middle of a sentinel-filled one: (view, whole)."""
    k = int(np.prod(shape))
    big = torch.full((k + 2 * PAD,), sent, dtype=dtype, device=DEV)
    view = big[PAD:PAD + k].view(*shape)
    if init is None:
        view.zero_()
    else:
        view.copy_(init)
    assert view.is_contiguous() and view.data_ptr() == big.data_ptr() + PAD * big.element_size()
    return view, big


def intact(name, big, k, sent=SENT):
    assert bool((big[:PAD] == sent).all()) and bool((big[PAD + k:] == sent).all()), name


# ---- the structs of the validation tests ------------------------------------------------------------------------------
def host_update(g, **over):
    """An Acas2dPpoUpdate whose pointers are host addresses: every case built from it must be rejected before any launch.
    Returns it with the buffer its pointers name."""
    buf = (C.c_char * 64)()
    f = {n: C.addressof(buf) for n, t in g.native.CPpoUpdate._fields_ if t is C.c_void_p}
    f.update(n_rows=64, obs_dim=8, clip_range=0.2, vf_coef=0.5, ent_coef=0.0, max_grad_norm=0.5, learning_rate=3e-4,
             beta1=0.9, beta2=0.999, adam_eps=1e-5)
    f.update(over)
    return g.native.CPpoUpdate(**f), buf


_ABSENT = object()


def host_update_set_args(g, a, guard=_ABSENT, opts=_ABSENT, **over):
    """The arguments of a set-update entry, every pointer of the Acas2dPpoUpdateSet the host address `a`, then `over`
    (which carries the four ints): the struct, then the Acas2dPpoGuard and the Acas2dPpoOptions where the entry takes them
    -- a triple of addresses each, or None for a NULL struct -- and a NULL stream."""
    f = {n: a for n, _ in g.native.CPpoUpdateSet._fields_}
    f.update(over)
    args = [C.byref(g.native.CPpoUpdateSet(**f))]
    for struct, triple in ((g.native.CPpoGuard, guard), (g.native.CPpoOptions, opts)):
        if triple is not _ABSENT:
            args.append(None if triple is None else C.byref(struct(*triple)))
    return args + [None]


# ---- the trainer helpers ----------------------------------------------------------------------------------------------
def count_calls(g, monkeypatch, symbol):
    """Wrap the bound function: every call through it is counted."""
    L = g.native.lib()
    inner = getattr(L, symbol)
    calls = []

    def counted(*args):
        calls.append(1)
        return inner(*args)

    monkeypatch.setattr(L, symbol, counted)
    return calls


def solo_trainer(g, cfg, envs=64, offset=0, **kw):
    venv = g.ACAS2DVecEnv(envs, 1, device=DEV, seed=13, env_offset=offset)
    return g.PPOTrainer(venv, cfg, collector="fused", updater="fused", gae="kernel", **kw)


def iterate(tr):
    tr.collect()
    st = tr.update()
    torch.cuda.synchronize()
    return st


# ---- the collector tests' states and policies -------------------------------------------------------------------------
# the set collectors' env state and outputs (+ obs = nine)
STATE = ("own_x", "own_y", "own_psi", "own_v", "goal_x", "goal_y", "trf_x", "trf_y", "trf_psi", "trf_v", "steps",
         "total_reward", "episode", "status")
OUTPUTS = ("actions", "values", "logp", "reward", "done", "outcome", "episode_return", "episode_steps")


def parallel_flight(env, rows):
    """Put traffic[0] of the env rows `rows` on the player's heading and speed (the NaN rows of ref_edge_n1 / n3: the
    reference's d_cpa is 0 / 0) and observe.  Returns (own, trf, goal) as injected and the first observation."""
    own = torch.stack([env.own_x, env.own_y, env.own_psi, env.own_v], 1).double().cpu().numpy()
    trf = torch.stack([env.trf_x, env.trf_y, env.trf_psi, env.trf_v], -1).double().cpu().numpy()
    goal = torch.stack([env.goal_x, env.goal_y], 1).double().cpu().numpy()
    trf[rows, 0, 2], trf[rows, 0, 3] = own[rows, 2], own[rows, 3]
    obs0 = env.set_state(own, trf, goal, np.zeros(env.num_envs, np.int32), observe=True).double().cpu().numpy()
    return (own, trf, goal), obs0


def scaled_actor(g, D, kind, obs0):
    """An SB3 actor whose hidden pre-activations reach |z| = 60 on obs0 in both layers ("saturating": v_exp_f32 in
    tanh_hw overflows to inf / underflows to 0), stay within 0.05 of 0 ("small"), or are SB3's own ("plain"); the head
    is scaled so that |mean - b3| reaches 1.5 (some actions clip, most do not) -- 0.3 for the near-zero one: there
    1 - 2 / (exp(2x) + 1) cancels, tanh_hw's ~1e-7 absolute error is large relative to h ~ 0.05, and the head's weights
    multiply it."""
    torch.manual_seed(7)
    pol = g.ActorCritic(D).double()
    pn = pol.mlp_extractor.policy_net
    x = R.obs32(obs0[np.isfinite(obs0).all(1)])
    with torch.no_grad():
        if kind != "plain":
            target = 60.0 if kind == "saturating" else 0.05
            z1, _ = R.preactivations64(R.params64(pol), x)
            pn[0].weight.mul_(target / np.abs(z1).max())
            _, z2 = R.preactivations64(R.params64(pol), x)
            pn[2].weight.mul_(target / np.abs(z2).max())
        p = R.params64(pol)
        mean = R.mlp64(p, "mlp_extractor.policy_net", "action_net", x) - p["action_net.bias"][0]
        pol.action_net.weight.mul_((0.3 if kind == "small" else 1.5) / np.abs(mean).max())
    return pol.float().to(DEV)
