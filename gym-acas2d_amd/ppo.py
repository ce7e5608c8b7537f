"""PPO on the device-resident ACAS2DVecEnv.

The reference trains with Stable-Baselines3 (`training_main.py:44-52`:
`PPO('MlpPolicy', env, seed=13).learn(1_048_576)`), one env, CPU.  SB3 is not available here and
its one-env-at-a-time loop is exactly what the batched engine replaces, so this module restates
the algorithm SB3 1.1.0 runs (clipped surrogate, advantages normalised per minibatch, MSE value loss
with SB3's optional clip_range_vf, learning-rate / clip-range schedules of progress_remaining,
state-independent log-std, orthogonal init, Adam eps 1e-5, gradient-norm clipping)
on E parallel envs: rollouts, GAE and the updates all stay on the GPU.  `PPOConfig.sb3()` carries the
hyper-parameters recorded in the reference's model zips (n_steps 2048, batch 64, epochs 10, gamma
0.99, lambda 0.95, clip 0.2, lr 3e-4, ent 0, vf 0.5, max-grad-norm 0.5); the DEFAULTS differ in the two
sizes that only make sense for one env (n_steps 128 per env, minibatch 16 384: a choice for E >= 1024,
stated here so that it is not mistaken for SB3's).  SB3's own semantics stay *parity unpinned*: no SB3
fixture exists in the reference; what is pinned is the arithmetic of one update (tests/test_ppo.py:
a float64 NumPy restatement with finite-difference gradients) and graph path == eager path.

The network uses SB3's `MlpPolicy` parameter names (separate 2x64 tanh actor / critic), so the
reference's trained zips load as initial weights (`ActorCritic.load_sb3_state_dict`) and a policy
trained here can be evaluated with `policy.SB3ActorPolicy` / `evaluate_policy`.

The loop is launch-bound (a 2x64 MLP on a few thousand rows: ~25 small kernels per env step, ~60 per
minibatch update), so on the GPU it runs from three hipGraphs (`use_graphs`, default on CUDA
devices): ONE env step of the collector (policy forward, sample, log-prob, the step kernel, the
buffer writes -- the time index is a device counter, so the same graph is replayed n_steps times),
the GAE recursion, and ONE minibatch update (gather by a static index buffer, losses, backward,
gradient clipping, capturable Adam).  No host synchronisation inside an iteration; episode
statistics are read once per iteration from the [T, E] side-channel buffers.

One learner (PPOTrainer) and K learners in the same launches (PopulationTrainer, PBTTrainer) differ in their random
streams and in the kernels they call, not in their host code, which is written once: `_Trainer` holds the static rollout
buffers, the intake of a fused collection and learn()'s loop; minibatch_buffers() / minibatch_schedule() the static index
buffers and an epoch's walk through them; `_FusedUpdater` what FusedUpdate and FusedUpdateSet share (the entry by width,
the workspace, hyper_row(), the struct of the set entries, the target_kl guard, clip_range_vf and the schedule factors);
policy.kernel_layout() the network as every kernel reads it.
"""
import dataclasses
import json
import math
import os
import random
import time
from typing import Optional

import numpy as np
import torch
from torch import nn

from .policy import kernel_layout


@dataclasses.dataclass
class PPOConfig:
    # The large-batch defaults (E >= 1 024 envs): 512 steps per env and iteration, minibatches of 4 096.  Measured for
    # seed robustness (tools/ppo_seed_sweep.py, 1 024 envs, fused collector + fused update, 60 M steps, seeds 13 / 14 /
    # 15, deterministic evaluation on the reference's 100 test episodes): 100 / 100 / 100 goals (mean return 1 257 /
    # 1 247 / 1 210; the reference's own policy: 100 goals, 1 210.07) -- against 24 / 42 / 44 goals at 30 M steps with
    # 256 steps per iteration and 91 - 99 with 512 (profiles/r03_ppo_seed_sweep_*.jsonl).  SB3's own values: sb3().
    n_steps: int = 512            # per env per iteration (SB3 default 2048 with ONE env; E envs here)
    batch_size: int = 4096        # minibatch (SB3 default 64 is sized for a 2048-sample buffer)
    n_epochs: int = 10
    gamma: float = 0.99
    gae_lambda: float = 0.95
    clip_range: float = 0.2
    learning_rate: float = 3e-4
    ent_coef: float = 0.0
    vf_coef: float = 0.5
    max_grad_norm: float = 0.5
    seed: int = 13                # settings.py:28
    # SB3's target_kl: PPO.train() abandons the rest of an update as soon as one minibatch's approx_kl exceeds 1.5 x
    # target_kl, before that minibatch's optimizer step.  None (SB3's default, and sb3()'s): no limit.
    target_kl: Optional[float] = None
    # SB3's clip_range_vf: the value loss is taken on old_values + clamp(values - old_values, -c, c).  None (SB3's
    # default, and sb3()'s): the plain MSE.  It depends on the reward scale; the returns of this env are of order 1e3.
    # SB3's schedules, as FACTORS: a callable progress_remaining (1 at the start of learn(), 0 at its end) -> factor
    # that multiplies learning_rate / clip_range / clip_range_vf -- or, in a population, whatever the member's hyper
    # row holds at that moment, so that a schedule composes with PBT's exploit step.  SB3's linear_schedule(3e-4) is
    # learning_rate=3e-4, learning_rate_schedule=linear_schedule().  None: constant.
    # The four are constructor arguments and attributes that dataclasses.replace() carries over, but InitVars, not fields:
    # tests/test_ppo_host.py holds every FIELD of a fully set config to differ from its default, and that file stays as it
    # is.  So dataclasses.fields(), asdict(), repr() and == do NOT see them: two configs that differ only in
    # clip_range_vf or a schedule compare equal, and PPOConfig(**asdict(c)) drops them.  Compare or copy them by name
    # (OPTION_FIELDS below); tests/test_sb3_options.py pins this.
    clip_range_vf: dataclasses.InitVar[Optional[float]] = None
    learning_rate_schedule: dataclasses.InitVar[Optional[object]] = None
    clip_range_schedule: dataclasses.InitVar[Optional[object]] = None
    clip_range_vf_schedule: dataclasses.InitVar[Optional[object]] = None

    def __post_init__(self, clip_range_vf, learning_rate_schedule, clip_range_schedule, clip_range_vf_schedule):
        if clip_range_vf is not None and not clip_range_vf > 0:
            raise ValueError("PPOConfig.clip_range_vf must be positive (None: no value clipping), got %r" % (clip_range_vf,))
        self.clip_range_vf = clip_range_vf
        self.learning_rate_schedule, self.clip_range_schedule = learning_rate_schedule, clip_range_schedule
        self.clip_range_vf_schedule = clip_range_vf_schedule

    @classmethod
    def sb3(cls, **overrides):
        """The values SB3 1.1.0's PPO ran the reference's training with (training_main.py:44-52 passes none, so
        these are SB3's defaults as recorded in models/**/*.zip): sized for ONE env -- with E envs the buffer
        is E x 2048 samples cut into minibatches of 64."""
        return cls(**{**dict(n_steps=2048, batch_size=64, n_epochs=10, gamma=0.99, gae_lambda=0.95, clip_range=0.2,
                             learning_rate=3e-4, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5), **overrides})


def linear_schedule(final=0.0):
    """The factor form of SB3's linear schedule: progress_remaining p -> final + (1 - final) * p, 1 at the start of
    learn() and `final` at its end."""
    final = float(final)
    return lambda p: final + (1.0 - final) * p


SCHEDULE_FIELDS = ("learning_rate_schedule", "clip_range_schedule", "clip_range_vf_schedule")
# PPOConfig's options that are attributes but not dataclass fields (the comment in PPOConfig says why)
OPTION_FIELDS = ("clip_range_vf",) + SCHEDULE_FIELDS


def schedule_factors(cfg, progress_remaining=1.0):
    """The three factors (on learning_rate, clip_range, clip_range_vf) of `cfg`'s schedules at `progress_remaining`; 1.0
    where there is no schedule.  A factor that is negative or not finite is a ValueError, here where it is evaluated."""
    out = []
    for name in SCHEDULE_FIELDS:
        f = getattr(cfg, name)
        x = 1.0 if f is None else float(f(progress_remaining))
        if not (math.isfinite(x) and x >= 0.0):
            raise ValueError("PPOConfig.%s(%r) = %r: a schedule's factor must be finite and >= 0"
                             % (name, progress_remaining, x))
        out.append(x)
    return out


def has_options(cfg):
    """True where `cfg` asks for clip_range_vf or a schedule: what acas2d_ppo_update_sb3_set_f32 exists for."""
    return cfg.clip_range_vf is not None or any(getattr(cfg, n) is not None for n in SCHEDULE_FIELDS)


def effective_config(cfg, progress_remaining=1.0):
    """`cfg` as one update at `progress_remaining` runs it: learning_rate, clip_range and clip_range_vf multiplied by
    their schedules' factors (a clip_range_vf that comes to 0 is None: the plain MSE), the schedules gone."""
    if not any(getattr(cfg, n) is not None for n in SCHEDULE_FIELDS):
        return cfg
    f = schedule_factors(cfg, progress_remaining)
    vf = None if cfg.clip_range_vf is None or not cfg.clip_range_vf * f[2] > 0 else cfg.clip_range_vf * f[2]
    return dataclasses.replace(cfg, learning_rate=cfg.learning_rate * f[0], clip_range=cfg.clip_range * f[1], clip_range_vf=vf,
                               **{n: None for n in SCHEDULE_FIELDS})


def _ortho(layer, gain):
    nn.init.orthogonal_(layer.weight, gain=gain)
    nn.init.zeros_(layer.bias)
    return layer


class _Mlp(nn.Module):
    def __init__(self, obs_dim):
        super().__init__()
        self.policy_net = nn.Sequential(_ortho(nn.Linear(obs_dim, 64), math.sqrt(2)), nn.Tanh(),
                                        _ortho(nn.Linear(64, 64), math.sqrt(2)), nn.Tanh())
        self.value_net = nn.Sequential(_ortho(nn.Linear(obs_dim, 64), math.sqrt(2)), nn.Tanh(),
                                       _ortho(nn.Linear(64, 64), math.sqrt(2)), nn.Tanh())


class ActorCritic(nn.Module):
    """SB3 `ActorCriticPolicy` for a Box(1) action: same parameter names as its state dict."""

    def __init__(self, obs_dim, log_std_init=0.0):
        super().__init__()
        self.mlp_extractor = _Mlp(obs_dim)
        self.action_net = _ortho(nn.Linear(64, 1), 0.01)
        self.value_net = _ortho(nn.Linear(64, 1), 1.0)
        self.log_std = nn.Parameter(torch.full((1,), float(log_std_init)))

    def load_sb3_state_dict(self, sd):
        self.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()
                              if k in self.state_dict()}, strict=True)

    def actor_weights(self):
        """(w1 [64,D], b1, w2 [64,64], b2, w3 [1,64], b3) for ACAS2DVecEnv.rollout_policy()."""
        pn = self.mlp_extractor.policy_net
        return tuple(t.detach() for t in (pn[0].weight, pn[0].bias, pn[2].weight, pn[2].bias,
                                          self.action_net.weight, self.action_net.bias))

    def forward(self, obs):
        x = obs.to(self.log_std.dtype)                     # float32 (SB3 casts observations the same way)
        mean = self.action_net(self.mlp_extractor.policy_net(x))
        value = self.value_net(self.mlp_extractor.value_net(x)).squeeze(-1)
        return mean, value

    def distribution(self, obs):
        mean, value = self.forward(obs)
        return torch.distributions.Normal(mean, self.log_std.exp().expand_as(mean)), value

    @torch.no_grad()
    def predict(self, obs, deterministic=True):
        mean, _ = self.forward(obs)
        a = mean if deterministic else torch.normal(mean, self.log_std.exp().expand_as(mean))
        return a.clamp(-1.0, 1.0)


@torch.no_grad()
def compute_gae(rewards, values, dones, last_value, gamma, lam):
    """SB3 RolloutBuffer.compute_returns_and_advantage.  rewards/values/dones: [T, E] where
    dones[t] says the episode ended AT step t (the value after it is not bootstrapped)."""
    T = rewards.shape[0]
    adv = torch.zeros_like(rewards)
    last = torch.zeros_like(last_value)
    for t in reversed(range(T)):
        next_value = last_value if t == T - 1 else values[t + 1]
        nonterminal = 1.0 - dones[t].to(rewards.dtype)
        delta = rewards[t] + gamma * next_value * nonterminal - values[t]
        last = delta + gamma * lam * nonterminal * last
        adv[t] = last
    return adv, adv + values


# observation widths the in-kernel bootstrap value of acas2d_gae_f32 is built for (n_traffic 1, 2, 3, 4, 8)
GAE_BOOTSTRAP_WIDTHS = (8, 11, 14, 17, 29)


def gae_constants(gamma, gae_lambda, n_members, device):
    """The two float32 [K] device tensors acas2d_gae_f32 reads, in compute_gae's semantics: Python numbers give
    float32(gamma) and float32(gamma * gae_lambda) with the product taken in double (what torch does with a Python scalar);
    if either is a tensor ([K], or one element), both are rounded to float32 first and multiplied in float32."""
    K = int(n_members)
    if torch.is_tensor(gamma) or torch.is_tensor(gae_lambda):
        g, l = (torch.as_tensor(x, dtype=torch.float32, device=device).reshape(-1) for x in (gamma, gae_lambda))
        if g.numel() not in (1, K) or l.numel() not in (1, K):
            raise ValueError("gamma / gae_lambda tensors need one element per member (%d), got %d / %d"
                             % (K, g.numel(), l.numel()))
        g, l = g.expand(K), l.expand(K)
        return g.contiguous(), (g * l).contiguous()
    g = torch.full((K,), float(gamma), dtype=torch.float32, device=device)
    return g, torch.full((K,), float(gamma) * float(gae_lambda), dtype=torch.float32, device=device)


def _critic_stacks(critic, n_members, obs_dim, device):
    """The six value-net tensors in Acas2dActorCritic's layout: from an ActorCritic (K = 1), an ActorCriticSet, or a
    sequence of six tensors already in that layout."""
    if isinstance(critic, ActorCriticSet):
        if critic.n_members != n_members or critic.obs_dim != obs_dim:
            raise ValueError("critic: a set of %d members of obs_dim %d, needed %d of %d"
                             % (critic.n_members, critic.obs_dim, n_members, obs_dim))
        w = critic.collector_weights()[6:12]
    elif isinstance(critic, nn.Module):
        if n_members != 1:
            raise ValueError("critic: one ActorCritic serves n_members = 1; pass an ActorCriticSet for %d" % n_members)
        vn = critic.mlp_extractor.value_net
        w = kernel_layout(vn[0].weight, vn[0].bias, vn[2].weight, vn[2].bias, critic.value_net.weight, critic.value_net.bias)
    else:
        w = list(critic)
    w = [t.to(device=device, dtype=torch.float32).contiguous() for t in w]
    want = (n_members * obs_dim * 64, n_members * 64, n_members * 64 * 64, n_members * 64, n_members * 64, n_members)
    if len(w) != 6 or tuple(t.numel() for t in w) != want:
        raise ValueError("critic must be the SB3 MlpPolicy value net %d -> 64 -> 64 -> 1 of %d member(s)" % (obs_dim, n_members))
    return w


@torch.no_grad()
def gae_fused(rewards, values, dones, last_value=None, gamma=0.99, gae_lambda=0.95, n_members=1, critic=None,
              obs_last=None, out=None, nan_count=None, constants=None):
    """compute_gae() as ONE hand-written launch (acas2d_gae_f32, csrc/acas2d_gae.hip), equal to it bit for bit.
    rewards / values [T, E] float32 and dones [T, E] bool or uint8 are the collector's buffers on the GPU; a NaN reward
    counts as 0 and an infinite one as +-FLT_MAX (torch.nan_to_num), so the raw rewards may be passed.
      last_value      [E] float32, or None: the kernel evaluates `critic` on obs_last [E, D] itself (a non-finite entry fed
                      as 0; D in {8, 11, 14, 17, 29}) with the collector's arithmetic, and the value is returned as well
      gamma, gae_lambda   Python numbers, or float32 tensors with one element per member: see gae_constants() for how
                      each form rounds gamma x lambda (as compute_gae does); `constants` = gae_constants(...) kept by the
                      caller saves forming them at every call
      n_members       K: member k owns the envs [k E / K, (k + 1) E / K); for K > 1, E / K must be a multiple of 64
      critic          an ActorCritic (K = 1), an ActorCriticSet, or the six value-net tensors in the collector's layout
      out             optional dict of preallocated outputs: "adv", "ret" [T, E] and "last_value" [E]
      nan_count       optional int32 [K] device tensor: the NaN rewards of member k are ADDED to nan_count[k]
    Returns (adv, ret), or (adv, ret, last_value) when the kernel computed the bootstrap value."""
    import ctypes as C
    from . import native
    if rewards.dim() != 2 or values.shape != rewards.shape or dones.shape != rewards.shape:
        raise ValueError("gae_fused takes rewards, values and dones of one shape [T, E]")
    T, E = rewards.shape
    K, dev = int(n_members), rewards.device
    if dev.type != "cuda":
        raise ValueError("gae_fused runs on the GPU (there is no CPU path: compute_gae is the torch one)")
    if rewards.dtype != torch.float32 or values.dtype != torch.float32 or dones.dtype not in (torch.bool, torch.uint8):
        raise ValueError("gae_fused takes float32 rewards / values and bool or uint8 dones")
    if K < 1 or (K > 1 and (E % K or (E // K) % 64)):
        raise ValueError("gae_fused needs E = K x a multiple of 64 for K > 1 members, got E = %d, K = %d" % (E, K))
    rewards, values, dones = rewards.contiguous(), values.contiguous(), dones.contiguous()
    out = {} if out is None else out
    adv = out["adv"] if "adv" in out else torch.empty_like(rewards)
    ret = out["ret"] if "ret" in out else torch.empty_like(rewards)
    for t in (adv, ret):
        if t.shape != rewards.shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
            raise ValueError("out['adv'] / out['ret'] must be contiguous float32 [T, E] tensors on the inputs' device")
    g_t, gl_t = constants if constants is not None else gae_constants(gamma, gae_lambda, K, dev)
    keep, lv_out, D = [], None, 0
    if last_value is None:
        if critic is None or obs_last is None:
            raise ValueError("gae_fused needs last_value, or critic and obs_last for the in-kernel bootstrap value")
        D = obs_last.shape[-1]
        if D not in GAE_BOOTSTRAP_WIDTHS:
            raise ValueError("the in-kernel bootstrap value is built for obs_dim in {8, 11, 14, 17, 29} (n_traffic 1, 2, 3, 4, "
                             "8), got %d -- pass last_value" % D)
        obs_last = obs_last.to(device=dev, dtype=torch.float32).contiguous()
        if obs_last.shape != (E, D):
            raise ValueError("obs_last must be [E, D] = [%d, %d]" % (E, D))
        keep = _critic_stacks(critic, K, D, dev)
        lv_out = out["last_value"] if "last_value" in out else torch.empty(E, dtype=torch.float32, device=dev)
    else:
        last_value = last_value.to(device=dev, dtype=torch.float32).contiguous()
        if last_value.shape != (E,):
            raise ValueError("last_value must be [E] = [%d]" % E)
    if nan_count is not None and (nan_count.dtype != torch.int32 or nan_count.numel() != K or nan_count.device != dev):
        raise ValueError("nan_count must be an int32 device tensor of %d element(s)" % K)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    g = native.CGae(p(rewards), p(values), p(dones), p(last_value), p(obs_last) if last_value is None else None,
                    *([p(t) for t in keep] if keep else [None] * 6), p(g_t), p(gl_t), p(adv), p(ret), p(lv_out), p(nan_count),
                    E, T, K, D, 0)
    with torch.cuda.device(dev):
        native.check(native.lib().acas2d_gae_f32(C.byref(g), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return (adv, ret) if last_value is not None else (adv, ret, lv_out)


# ---- reward normalisation: SB3's VecNormalize(norm_obs=False, norm_reward=True), on the device (csrc/acas2d_rewnorm.hip) ----
def _reward_norm_gamma(gamma, n_members, device):
    """The float64 [K] tensor of the members' discounts from a number or one per member."""
    K = int(n_members)
    g = torch.as_tensor(gamma, dtype=torch.float64).reshape(-1)
    if g.numel() not in (1, K):
        raise ValueError("gamma needs one element per member (%d), got %d" % (K, g.numel()))
    return g.expand(K).contiguous().to(device)


@torch.no_grad()
def normalize_rewards_reference(rewards, dones, returns, stats, gamma, epsilon=1e-8, clip_reward=10.0, n_members=1, out=None):
    """RewardNormalizer.normalize() as torch float64 operations, row by row: the documented slow path (about ten small
    launches per row on a GPU; it runs on the CPU too) and the baseline of tools/bench_reward_norm.py.  The arithmetic is
    include/acas2d.h's (acas2d_reward_normalize_f32), the two sums over a member's envs in torch's order.
      rewards   [T, E] float32 (NaN counts as 0, +-inf as +-FLT_MAX); dones [T, E] bool or uint8
      returns   float64 [E] and stats float64 [K, 3] (mean, var, count): the state, UPDATED in place
      gamma     a number, one per member, or a float64 [K] tensor
    Returns the normalised rewards, float32 [T, E] (`out`, which may be `rewards`, if given).  No host read."""
    T, E = rewards.shape
    K = int(n_members)
    if K < 1 or E % K:
        raise ValueError("normalize_rewards_reference needs E = K x EM, got E = %d, K = %d" % (E, K))
    EM, dev = E // K, rewards.device
    if returns.dtype != torch.float64 or stats.dtype != torch.float64 or tuple(returns.shape) != (E,) or tuple(stats.shape) != (K, 3):
        raise ValueError("normalize_rewards_reference: returns float64 [%d] and stats float64 [%d, 3]" % (E, K))
    g = _reward_norm_gamma(gamma, K, dev).view(K, 1)
    r64 = torch.nan_to_num(rewards.to(torch.float32), nan=0.0).to(torch.float64).view(T, K, EM)
    dones = dones.view(T, K, EM).to(torch.bool)
    out = torch.empty(T, E, dtype=torch.float32, device=dev) if out is None else out
    G = returns.view(K, EM)
    mean, var, count = stats[:, 0].clone(), stats[:, 1].clone(), stats[:, 2].clone()
    for t in range(T):
        r = r64[t]
        G.mul_(g).add_(r)
        bm = G.sum(1) / EM
        d = G - bm.unsqueeze(1)
        bv = (d * d).sum(1) / EM
        delta, tot = bm - mean, count + EM
        mean_new = mean + delta * EM / tot
        m2 = var * count + bv * EM + delta * delta * count * EM / tot
        var, mean, count = m2 / tot, mean_new, tot
        out[t].copy_(torch.clamp(r / torch.sqrt(var + epsilon).unsqueeze(1), -clip_reward, clip_reward).view(E))
        G.masked_fill_(dones[t], 0.0)
    stats.copy_(torch.stack((mean, var, count), 1))
    return out


class RewardNormalizer:
    """SB3's VecNormalize(norm_obs=False, norm_reward=True) for a [T, E] buffer of collected rewards, as ONE call of
    acas2d_reward_normalize_f32 (four small launches, no host synchronisation): every reward is divided by the running
    standard deviation of the discounted return and clipped to +-clip_reward.  It owns the state -- `returns` float64 [E],
    the discounted return of every env, and `stats` float64 [K, 3], member k's running mean, variance and count (SB3's
    RunningMeanStd: 0, 1, 1e-4 at the start) -- and the kernel's workspace.  Member k owns the envs [k EM, (k + 1) EM);
    for K > 1, EM must be a multiple of 64.  `gamma`: a number, or one per member.  The same inputs give the same bits, a
    buffer may be passed in pieces (the state carries everything), and a member's numbers do not depend on the others."""

    def __init__(self, n_envs, n_members=1, gamma=0.99, epsilon=1e-8, clip_reward=10.0, device="cuda:0"):
        E, K = int(n_envs), int(n_members)
        if E < 1 or K < 1 or (K > 1 and (E % K or (E // K) % 64)):
            raise ValueError("RewardNormalizer needs n_envs = K x a multiple of 64 for K > 1 members, got n_envs = %d, K = %d"
                             % (E, K))
        if not (math.isfinite(epsilon) and epsilon > 0 and math.isfinite(clip_reward) and clip_reward > 0):
            raise ValueError("RewardNormalizer: epsilon and clip_reward must be finite and positive, got %r, %r"
                             % (epsilon, clip_reward))
        self.n_envs, self.n_members, self.device = E, K, torch.device(device)
        self.epsilon, self.clip_reward = float(epsilon), float(clip_reward)
        self.gamma = _reward_norm_gamma(gamma, K, self.device)
        self.returns = torch.zeros(E, dtype=torch.float64, device=self.device)
        self.stats = torch.tensor([[0.0, 1.0, 1e-4]] * K, dtype=torch.float64).to(self.device)
        self._workspace = None

    def normalize(self, rewards, dones, out=None):
        """Normalise the rows of `rewards` [T, E] (float32, on the device; NaN counts as 0, +-inf as +-FLT_MAX) in order,
        resetting an env's discounted return where `dones` [T, E] (bool or uint8) is set; the state moves on by T steps.
        out: a float32 [T, E] tensor, `rewards` itself for in place, or None for a new one.  One ABI call on the current
        stream; returns `out`."""
        import ctypes as C
        from . import native
        dev, E, K = self.device, self.n_envs, self.n_members
        if dev.type != "cuda":
            raise ValueError("RewardNormalizer.normalize runs on the GPU (normalize_rewards_reference is the torch path)")
        if rewards.dim() != 2 or rewards.shape[1] != E or dones.shape != rewards.shape:
            raise ValueError("normalize takes rewards and dones of one shape [T, %d]" % E)
        if rewards.dtype != torch.float32 or dones.dtype not in (torch.bool, torch.uint8):
            raise ValueError("normalize takes float32 rewards and bool or uint8 dones")
        out = torch.empty_like(rewards) if out is None else out
        for t in (rewards, dones, out):
            if t.device != dev or not t.is_contiguous():
                raise ValueError("normalize takes contiguous tensors on %s" % dev)
        if out.shape != rewards.shape or out.dtype != torch.float32:
            raise ValueError("out must be a float32 tensor of the rewards' shape")
        T = rewards.shape[0]
        L = native.lib()
        need = L.acas2d_reward_norm_workspace_bytes(E, T, K)
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        p = lambda t: t.data_ptr()  # noqa: E731
        n = native.CRewardNorm(p(rewards), p(dones), p(out), p(self.returns), p(self.stats), p(self.gamma), p(self._workspace),
                               self.epsilon, self.clip_reward, E, T, K)
        with torch.cuda.device(dev):
            native.check(L.acas2d_reward_normalize_f32(C.byref(n), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        return out

    def reward_std(self):
        """sqrt(var + epsilon) per member, float64 [K] on the device: what a reward is divided by now."""
        return torch.sqrt(self.stats[:, 1] + self.epsilon)

    def inherit(self, donor):
        """stats[k] = stats[donor[k]] for every member, as one device gather (donor: an integer device tensor [K], as
        population_exploit returns it); `returns`, the envs' own discounted returns, stay."""
        self.stats.copy_(self.stats.index_select(0, donor.to(device=self.device, dtype=torch.int64)))

    def state_dict(self, member=None):
        """The state and the constants (CPU copies); member=k: member k's alone, as a normaliser of one member holds it."""
        E, K = self.n_envs, self.n_members
        EM = E // K
        env = slice(None) if member is None else slice(member * EM, (member + 1) * EM)
        mem = slice(None) if member is None else slice(member, member + 1)
        return {"returns": self.returns[env].cpu().clone(), "stats": self.stats[mem].cpu().clone(),
                "gamma": self.gamma[mem].cpu().clone(), "epsilon": self.epsilon, "clip_reward": self.clip_reward,
                "n_envs": E if member is None else EM, "n_members": K if member is None else 1}

    def load_state_dict(self, sd):
        if (sd["n_envs"], sd["n_members"]) != (self.n_envs, self.n_members):
            raise ValueError("load_state_dict: the state of %d envs / %d member(s), this normaliser has %d / %d"
                             % (sd["n_envs"], sd["n_members"], self.n_envs, self.n_members))
        self.returns.copy_(sd["returns"])                 # in place: the addresses stay (captured graphs may hold them)
        self.stats.copy_(sd["stats"])
        self.gamma.copy_(sd["gamma"])
        self.epsilon, self.clip_reward = float(sd["epsilon"]), float(sd["clip_reward"])


def _reward_normalizer_for(reward_norm, n_envs, configs, device):
    """A trainer's `reward_norm` argument: True (SB3's defaults, gamma from the configs) or a RewardNormalizer."""
    K = len(configs)
    if reward_norm is True:
        return RewardNormalizer(n_envs, K, gamma=[c.gamma for c in configs], device=device)
    if not isinstance(reward_norm, RewardNormalizer):
        raise TypeError("reward_norm must be None, True or a RewardNormalizer, got %r" % (reward_norm,))
    same = lambda a, b: a.type == b.type and (a.index or 0) == (b.index or 0)  # noqa: E731
    if (reward_norm.n_envs, reward_norm.n_members) != (n_envs, K) or not same(reward_norm.device, torch.device(device)):
        raise ValueError("reward_norm: a RewardNormalizer of %d envs / %d member(s) on %s, the trainer has %d / %d on %s"
                         % (reward_norm.n_envs, reward_norm.n_members, reward_norm.device, n_envs, K, device))
    return reward_norm


LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)


def _normal_logp(mean, log_std, x):
    """log N(x; mean, exp(log_std)) summed over the action dimension (torch.distributions.Normal.log_prob)."""
    return (-((x - mean) ** 2) / (2.0 * (2.0 * log_std).exp()) - log_std - LOG_SQRT_2PI).sum(-1)


def ppo_loss(policy, cfg, obs, act, old_logp, adv, ret, old_val=None):
    """SB3 1.1.0 PPO.train() for one minibatch of a Box(1) action space: advantages normalised over the
    minibatch, clipped surrogate, MSE value loss -- plain with cfg.clip_range_vf = None, otherwise on old_val +
    clamp(value - old_val, -clip_range_vf, clip_range_vf) (`old_val`: the rollout's values of the rows, then required;
    no max with the unclipped loss) -- and the entropy of the state-independent Gaussian.  cfg's numbers are used as they
    are: effective_config() applies the schedules.  The ONE loss both the captured and the op-by-op update run.
    Returns (loss, pg, vf)."""
    mean, value = policy.forward(obs)
    log_std = policy.log_std
    logp = _normal_logp(mean, log_std, act)
    a = (adv - adv.mean()) / (adv.std() + 1e-8)
    ratio = (logp - old_logp).exp()
    pg = -torch.min(a * ratio, a * ratio.clamp(1 - cfg.clip_range, 1 + cfg.clip_range)).mean()
    if cfg.clip_range_vf is None:
        vf = torch.nn.functional.mse_loss(value, ret)
    else:
        if old_val is None:
            raise ValueError("ppo_loss: clip_range_vf needs old_val, the rollout's values of the minibatch's rows")
        value_pred = old_val + (value - old_val).clamp(-cfg.clip_range_vf, cfg.clip_range_vf)
        vf = torch.nn.functional.mse_loss(ret, value_pred)
    ent = -(0.5 + LOG_SQRT_2PI + log_std).sum()           # -entropy of N(., exp(log_std)), the same for every state
    return pg + cfg.ent_coef * ent + cfg.vf_coef * vf, pg, vf


@torch.no_grad()
def approx_kl_and_clip_fraction(policy, cfg, obs, act, old_logp):
    """What SB3 1.1.0's PPO.train() measures on a minibatch beside its loss, under no_grad: approx_kl = mean((ratio - 1)
    - log ratio) (Schulman's low-variance estimator, the one `target_kl` is compared with) and clip_fraction =
    mean(|ratio - 1| > clip_range), with ppo_loss()'s log-prob.  Returns two 0-d tensors."""
    mean, _ = policy.forward(obs)
    log_ratio = _normal_logp(mean, policy.log_std, act) - old_logp
    ratio = log_ratio.exp()
    return ((ratio - 1.0) - log_ratio).mean(), ((ratio - 1.0).abs() > cfg.clip_range).to(log_ratio.dtype).mean()


def explained_variance(values, returns):
    """SB3's train/explained_variance, 1 - Var(returns - values) / Var(returns) (population variances, as np.var), over
    the LAST dimension: flat buffers give a 0-d tensor, [K, n] per-member rows give [K].  NaN where Var(returns) == 0."""
    var_ret = returns.var(dim=-1, unbiased=False)
    ev = 1.0 - (returns - values).var(dim=-1, unbiased=False) / var_ret
    return torch.where(var_ret == 0, torch.full_like(ev, float("nan")), ev)


# observation widths the fused minibatch update is built for: acas2d_ppo_update_f32 (a lane holds its observation row in
# registers; n_traffic 1, 2, 3, 4, 8) and acas2d_ppo_update_wide_f32 (four waves tile it through LDS; n_traffic 16, 32, 64)
FUSED_UPDATE_WIDTHS = (8, 11, 14, 17, 29)
FUSED_UPDATE_WIDE_WIDTHS = (53, 101, 197)
# the 13 parameter tensors in FusedUpdate's order (the flat grad / moment layout of include/acas2d.h)
PARAM_NAMES = ("mlp_extractor.policy_net.0.weight", "mlp_extractor.policy_net.0.bias",
               "mlp_extractor.policy_net.2.weight", "mlp_extractor.policy_net.2.bias", "action_net.weight", "action_net.bias",
               "mlp_extractor.value_net.0.weight", "mlp_extractor.value_net.0.bias",
               "mlp_extractor.value_net.2.weight", "mlp_extractor.value_net.2.bias", "value_net.weight", "value_net.bias",
               "log_std")
# hyper[k]: the row acas2d_ppo_update_set_f32 reads for member k (target_kl is not in it: FusedUpdateSet.target_kl)
HYPER_SLOTS = ("clip_range", "vf_coef", "ent_coef", "max_grad_norm", "learning_rate", "beta1", "beta2", "adam_eps")


def hyper_row(cfg, beta1=0.9, beta2=0.999, adam_eps=1e-5):
    """One learner's hyper-parameters as the update kernels take them, in HYPER_SLOTS order."""
    return [cfg.clip_range, cfg.vf_coef, cfg.ent_coef, cfg.max_grad_norm, cfg.learning_rate, beta1, beta2, adam_eps]


def _flat_rollout(obs, act, old_logp, adv, ret):
    """The five rollout buffers as the update kernels take them: obs [n, D], the others [n] (views of the storage)."""
    bufs = [t.reshape(-1) if i else t.reshape(-1, obs.shape[-1]) for i, t in enumerate((obs, act, old_logp, adv, ret))]
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in bufs)
    return bufs


class _FusedUpdater:
    """What FusedUpdate and FusedUpdateSet share: the choice of the entry by width, the workspace (`grad`, `m`, `v`,
    `step_count`, `stats`) with a leading [K] for a set, the flat rollout, the `hyper` rows, the struct of the set entries
    and the guarded update (acas2d_ppo_update_guarded_set_f32, csrc/acas2d_ppo_guard.hip): the per-member `target_kl`
    limits, the `stopped` flags and the `diag` rows the kernels keep, as ONE device buffer so that begin_update() is one
    memset.  Where a config has a clip_range_vf or a schedule (`options`; the updater is then guarded by implication)
    every step goes through acas2d_ppo_update_sb3_set_f32 (csrc/acas2d_ppo_sb3.hip) instead: `clip_range_vf` float32 [K]
    (0: plain MSE) and `scale` float32 [K, 4], the factors on learning_rate, clip_range and clip_range_vf that
    begin_update(progress_remaining) evaluates on the host and writes with one non-blocking copy; the kernels multiply
    them into whatever `hyper` holds."""
    # one row per width class: the widths, the solo symbol, the set symbol (`_symbol` names a subclass's column)
    _ENTRIES = ((FUSED_UPDATE_WIDTHS, "acas2d_ppo_update_f32", "acas2d_ppo_update_set_f32"),
                (FUSED_UPDATE_WIDE_WIDTHS, "acas2d_ppo_update_wide_f32", "acas2d_ppo_update_wide_set_f32"))

    @classmethod
    def _entry_for(cls, D):
        for row in cls._ENTRIES:
            if D in row[0]:
                return row[cls._symbol]
        built = " and ".join("{%s} (n_traffic %s: %s)" % (", ".join(map(str, row[0])), ", ".join(str((d - 5) // 3) for d in row[0]),
                                                          row[cls._symbol]) for row in cls._ENTRIES)
        raise ValueError("%s is built for obs_dim in %s%s %d" % (cls.__name__, built, cls._got, D))

    def __init__(self, params, configs, rollout, lead, beta1, beta2, adam_eps, diagnostics, old_val=None):
        import ctypes as C
        from . import native
        self.D, K, dev = rollout[0].shape[-1], len(configs), rollout[0].device
        self.entry = self._entry_for(self.D)
        self._C, self._native, self._lib, self.device = C, native, native.lib(), dev
        self._update = getattr(self._lib, self.entry)
        n = int(self._lib.acas2d_ppo_workspace_floats(self.D))
        z = lambda *shape, dt=torch.float32: torch.zeros(*shape, dtype=dt, device=dev)  # noqa: E731
        self.grad, self.m, self.v, self.step_count, self.stats = z(*lead, n), z(*lead, n), z(*lead, n), z(K, dt=torch.int32), z(*lead, 8)
        self.hyper = torch.tensor([hyper_row(c, beta1, beta2, adam_eps) for c in configs], dtype=torch.float32).to(dev)
        self._params = params
        assert all(p.dtype == torch.float32 and p.is_contiguous() and p.device == dev for p in params)
        self._bufs = _flat_rollout(*rollout)
        self.configs = list(configs)
        self.options = any(has_options(c) for c in configs)
        self.factors = [[1.0, 1.0, 1.0] for _ in configs]  # of the update begin_update() last opened
        self.guarded = bool(diagnostics) or self.options or any(c.target_kl is not None for c in configs)
        if self.guarded:
            # a config's target_kl as the kernels take it: None is 0, no limit
            self.target_kl = torch.tensor([0.0 if c.target_kl is None else float(c.target_kl) for c in configs],
                                          dtype=torch.float32).to(dev)
            self._guard_state = torch.zeros(K * 9, dtype=torch.float32, device=dev)
            self.diag = self._guard_state[:K * 8].view(K, 8)
            self.stopped = self._guard_state[K * 8:].view(torch.int32)
            self._guarded_update = self._lib.acas2d_ppo_update_guarded_set_f32
            self._guard = native.CPpoGuard(self.target_kl.data_ptr(), self.stopped.data_ptr(), self.diag.data_ptr())
        if self.options:
            if old_val is None and any(c.clip_range_vf is not None for c in configs):
                raise ValueError("clip_range_vf needs old_val, the rollout's values (flat, rows as obs / act / ...)")
            # no clip_range_vf anywhere: the kernels read old_val for no member, and `ret` stands in for the pointer
            self.old_val = self._bufs[4] if old_val is None else old_val.reshape(-1)
            if (self.old_val.dtype != torch.float32 or not self.old_val.is_contiguous() or self.old_val.device != dev
                    or self.old_val.numel() != self._bufs[4].numel()):
                raise ValueError("old_val must be a contiguous float32 tensor of the rollout's %d rows on %s"
                                 % (self._bufs[4].numel(), dev))
            self.clip_range_vf = torch.tensor([0.0 if c.clip_range_vf is None else float(c.clip_range_vf) for c in configs],
                                              dtype=torch.float32).to(dev)
            self.scale = torch.ones(K, 4, dtype=torch.float32, device=dev)
            self._scale_host = torch.ones(K, 4, dtype=torch.float32, pin_memory=dev.type == "cuda")
            self._scale_copied = torch.cuda.Event() if dev.type == "cuda" else None   # recorded after every copy
            self._scale_pending = False
            self._sb3_update = self._lib.acas2d_ppo_update_sb3_set_f32
            self._opts = native.CPpoOptions(self.old_val.data_ptr(), self.clip_range_vf.data_ptr(), self.scale.data_ptr())

    def _stream(self):
        return self._C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _set_struct(self, idx, K, B, apply=True):
        """The Acas2dPpoUpdateSet of one minibatch: `idx` names B rows for each of the K members."""
        assert idx.dtype == torch.int64 and idx.is_contiguous()
        p = lambda t: t.data_ptr()  # noqa: E731
        return self._native.CPpoUpdateSet(*[p(t) for t in self._params], *[p(t) for t in self._bufs], p(idx), K, B, self.D,
                                          1 if apply else 0, p(self.hyper), p(self.grad), p(self.m), p(self.v),
                                          p(self.step_count), p(self.stats))

    def _step_guarded(self, idx, K, B):
        u = self._set_struct(idx, K, B)
        if self.options:
            self._native.check(self._sb3_update(self._C.byref(u), self._C.byref(self._guard), self._C.byref(self._opts),
                                                self._stream()))
            return
        self._native.check(self._guarded_update(self._C.byref(u), self._C.byref(self._guard), self._stream()))

    def begin_update(self, progress_remaining=1.0):
        """Where SB3 enters train(): every member runs again and the statistics start over.  One memset on the current
        stream, no synchronisation; nothing to do for an update that is not guarded.  With `options`, the configs'
        schedules are evaluated at `progress_remaining` (schedule_factors: a bad factor is a ValueError) and the [K, 4]
        rows of `scale` written with one non-blocking copy beside the memset; `factors` keeps them for the log."""
        if self.options:
            factors = [schedule_factors(c, progress_remaining) for c in self.configs]
            if self._scale_pending:
                self._scale_copied.synchronize()           # (the last update's copy has long left the pinned rows)
            self._scale_host[:, :3] = torch.tensor(factors, dtype=torch.float32)
            self.scale.copy_(self._scale_host, non_blocking=True)
            if self._scale_copied is not None:
                self._scale_copied.record(torch.cuda.current_stream(self.device))
                self._scale_pending = True
            self.factors = factors
        if self.guarded:
            self._guard_state.zero_()

    def effective(self, hyper_rows=None):
        """Per member, the learning_rate, clip_range and (where set) clip_range_vf the update begin_update() last
        opened runs with: the hyper row's value -- `hyper_rows` ([K][8] numbers read back by the caller), else the
        config's -- times the factor."""
        out = []
        for k, (c, f) in enumerate(zip(self.configs, self.factors)):
            lr, clip = (c.learning_rate, c.clip_range) if hyper_rows is None else (hyper_rows[k][4], hyper_rows[k][0])
            out.append({"learning_rate": lr * f[0], "clip_range": clip * f[1],
                        **({} if c.clip_range_vf is None else {"clip_range_vf": c.clip_range_vf * f[2]})})
        return out

    def _diagnostics(self):
        if not self.guarded:
            raise RuntimeError("diagnostics() needs the guarded update: a target_kl in the config, or diagnostics=True")
        d, stopped = self.diag.cpu().tolist(), self.stopped.cpu().tolist()
        nan = float("nan")
        return [{"approx_kl": r[4] / r[6] if r[6] else nan, "clip_fraction": r[5] / r[6] if r[6] else nan,
                 "n_minibatches": int(r[6]), "n_applied": int(r[7]), "early_stop": bool(f),
                 "last_approx_kl": r[2], "last_clip_fraction": r[3]} for r, f in zip(d, stopped)]


class FusedUpdate(_FusedUpdater):
    """One PPO minibatch update as two hand-written launches (acas2d_ppo_update_f32, csrc/acas2d_ppo.hip; for obs_dim
    53, 101, 197 acas2d_ppo_update_wide_f32, csrc/acas2d_ppo_wide.hip -- `entry` names the one chosen): forward,
    ppo_loss(), backward, clip_grad_norm_ and Adam for the SB3 MlpPolicy actor-critic, on the parameter tensors in
    place.  `obs` [n, D], `act` / `old_logp` / `adv` / `ret` [n] are the flat float32 rollout buffers (their storage
    must stay put), `idx` an int64 device tensor naming the minibatch's rows (rewritten by the caller between
    calls).  Keeps its own Adam moments (torch.optim.Adam's arithmetic, eps 1e-5 as SB3 sets it).
    With `cfg.target_kl` or `diagnostics=True` every step goes through acas2d_ppo_update_guarded_set_f32 instead, as a
    population of one (`guarded`; the hyper-parameters are then `hyper`, the config's at construction): call
    begin_update() once per PPO update, step() for every minibatch whether the learner has stopped or not, and read
    diagnostics() afterwards.  With `cfg.clip_range_vf` or a schedule the guarded steps go through
    acas2d_ppo_update_sb3_set_f32 (`options`; `old_val` [n]: the rollout's values, required with clip_range_vf) and
    begin_update(progress_remaining) sets the schedules' factors.  Otherwise the calls are the ones above and
    begin_update() does nothing."""
    _symbol, _got = 1, ", got"

    def __init__(self, policy, cfg, obs, act, old_logp, adv, ret, beta1=0.9, beta2=0.999, adam_eps=1e-5,
                 diagnostics=False, old_val=None):
        super().__init__([policy.get_parameter(name) for name in PARAM_NAMES], [cfg], (obs, act, old_logp, adv, ret), (),
                         beta1, beta2, adam_eps, diagnostics, old_val)
        self.cfg, self.betas, self.adam_eps = cfg, (beta1, beta2), adam_eps

    def _struct(self, idx):
        assert idx.dtype == torch.int64 and idx.is_contiguous()
        p = lambda t: t.data_ptr()  # noqa: E731
        return self._native.CPpoUpdate(*[p(t) for t in self._params], *[p(t) for t in self._bufs], p(idx), idx.numel(), self.D,
                                       *hyper_row(self.cfg, *self.betas, self.adam_eps), p(self.grad), p(self.m), p(self.v),
                                       p(self.step_count), p(self.stats))

    def step(self, idx):
        if self.guarded:                                  # the learner's tensors are K = 1 stacks
            self._step_guarded(idx, 1, idx.numel())
            return
        u = self._struct(idx)
        self._native.check(self._update(self._C.byref(u), self._stream()))

    def last_losses(self):
        s = self.stats.cpu().tolist()
        return {"pg_loss": s[4], "value_loss": s[5], "grad_norm": s[2]}

    def diagnostics(self):
        """Since begin_update(): approx_kl and clip_fraction (SB3's train/ values: means over the minibatches the learner
        took, the stopping one included), n_minibatches, n_applied (optimizer steps), early_stop, and the last minibatch's
        own last_approx_kl / last_clip_fraction.  One read-back."""
        return self._diagnostics()[0]


# traffic counts at which PPOTrainer takes the group-cooperative launches by itself (float32; at 8 the thread-per-env
# kernel exists and is the better design: its weights are scalar operands)
GROUP_TRAFFIC = (16, 32, 64)


def episode_summary(returns, lengths, outcomes):
    """recent_episodes() for one learner, from its lists of per-collection tensors (None where no episode ended)."""
    if not returns:
        return None
    r, l, o = torch.cat(returns), torch.cat(lengths), torch.cat(outcomes)
    return {"episodes": int(r.numel()), "ep_rew_mean": float(r.mean()), "ep_len_mean": float(l.float().mean()),
            "goal": float((o == 1).float().mean()), "collision": float((o == 2).float().mean()),
            "timeout": float((o == 3).float().mean())}


class _Callbacks:
    """learn()'s EvalCallback / CheckpointCallback bookkeeping for ONE learner, whose files go under `save_dir` and whose
    ActorCritic `policy()` gives when one is saved; `head` opens every record (a population's {"member": k}).  With
    reward normalisation on, `reward_norm()` gives the learner's RewardNormalizer.state_dict(), saved beside every zip:
    best_model_reward_norm.pt, checkpoints/reward_norm_<num_timesteps>_steps.pt (the zips are SB3's, untouched).  A
    learner that trains under a disturbance passes it as `disturbance` (Disturbance.to_dict()'s numbers): saved likewise
    as best_model_disturbance.json, checkpoints/disturbance_<num_timesteps>_steps.json."""

    def __init__(self, save_dir, policy, head=(), reward_norm=None, disturbance=None):
        self.save_dir, self.policy, self.head, self.reward_norm = save_dir, policy, dict(head), reward_norm
        self.disturbance = disturbance
        self.evals = {"timesteps": [], "results": [], "ep_lengths": []}
        self.best = -math.inf

    def evaluated(self, timesteps, ret, steps, outcome, unfinished):
        from .policy import save_sb3_policy
        mean = float(ret.mean())
        new_best = mean > self.best
        self.best = max(self.best, mean)
        rec = {**self.head, "eval": True, "timesteps": timesteps, "mean_reward": mean, "std_reward": float(ret.std()),
               "mean_ep_length": float((steps - 1).mean()), "goal": float((outcome == 1).mean()),
               "collision": float((outcome == 2).mean()), "timeout": float((outcome == 3).mean()),
               "unfinished": int(unfinished), "new_best": new_best}
        if self.save_dir:
            ev = self.evals
            ev["timesteps"].append(timesteps)
            ev["results"].append(ret.astype(np.float64))
            ev["ep_lengths"].append(steps.astype(np.int64) - 1)
            os.makedirs(os.path.join(self.save_dir, "results"), exist_ok=True)
            np.savez(os.path.join(self.save_dir, "results", "evaluations.npz"),
                     timesteps=np.asarray(ev["timesteps"], np.int64), results=np.stack(ev["results"]),
                     ep_lengths=np.stack(ev["ep_lengths"]))
            if new_best:
                save_sb3_policy(self.policy(), os.path.join(self.save_dir, "best_model.zip"))
                if self.reward_norm is not None:
                    torch.save(self.reward_norm(), os.path.join(self.save_dir, "best_model_reward_norm.pt"))
                self._save_disturbance(os.path.join(self.save_dir, "best_model_disturbance.json"))
        return rec

    def _save_disturbance(self, path):
        if self.disturbance is not None:
            with open(path, "w") as f:
                json.dump(self.disturbance, f)

    def checkpoint(self, timesteps):
        from .policy import save_sb3_policy
        save_sb3_policy(self.policy(), os.path.join(self.save_dir, "checkpoints", "model_%d_steps.zip" % timesteps))
        if self.reward_norm is not None:
            torch.save(self.reward_norm(), os.path.join(self.save_dir, "checkpoints", "reward_norm_%d_steps.pt" % timesteps))
        self._save_disturbance(os.path.join(self.save_dir, "checkpoints", "disturbance_%d_steps.json" % timesteps))


def minibatch_buffers(n, batch_size, device, lead=()):
    """The static index buffers of an update over n rows (each with the leading shape `lead`: a population's (K,)):
    `mb_idx` for the whole minibatches of B = min(batch_size, n) rows and `mb_tail` for the partial last one of an epoch,
    as SB3 takes it -- None if there is none or it is ONE row: the advantage normalisation divides by the standard
    deviation of the minibatch, which one row does not have (NaN in SB3 as well)."""
    B = min(batch_size, n)
    mb_idx = torch.zeros(*lead, B, dtype=torch.int64, device=device)
    return mb_idx, (torch.zeros(*lead, n % B, dtype=torch.int64, device=device) if n % B > 1 else None)


def minibatch_schedule(rows, mb_idx, mb_tail):
    """One epoch: `rows` ([n], or [K, n]) is its permutation; every whole minibatch is copied into `mb_idx` and that
    buffer yielded, then the partial one through `mb_tail` where there is one."""
    n, B = rows.shape[-1], mb_idx.shape[-1]
    for i in range(0, n - B + 1, B):
        mb_idx.copy_(rows[..., i:i + B])
        yield mb_idx
    if mb_tail is not None:
        mb_tail.copy_(rows[..., n - n % B:])
        yield mb_tail


class _Trainer:
    """What PPOTrainer and PopulationTrainer share: the static [T, E] rollout buffers `b_*`, the intake of a fused
    collection into them, and learn()'s loop."""

    def _alloc_rollout(self):
        E, T, D, dev = self.venv.num_envs, self.cfg.n_steps, self.venv.obs_dim, self.device
        f32 = dict(dtype=torch.float32, device=dev)
        # zeros, not empty: PPOTrainer's capture warm-up runs GAE and two updates over the whole buffer
        self.b_obs = torch.zeros(T, E, D, **f32)
        self.b_act = torch.zeros(T, E, 1, **f32)
        self.b_logp, self.b_val, self.b_rew = (torch.zeros(T, E, **f32) for _ in range(3))
        self.b_adv, self.b_ret, self.b_epret = (torch.zeros(T, E, **f32) for _ in range(3))
        self.b_done = torch.zeros(T, E, dtype=torch.bool, device=dev)
        self.b_eplen = torch.zeros(T, E, dtype=torch.int32, device=dev)
        self.b_outcome = torch.zeros(T, E, dtype=torch.uint8, device=dev)

    def _store_collection(self, out):
        """A fused collector's dict (ACAS2DVecEnv.collect / collect_set) into the buffers and `self.obs`, cast to float32
        first and then cleaned of NaN.  Returns the NaN events per sample, int64 [T, E].  A disturbed collection
        ("obs_read" in the dict): b_obs holds the rows the networks READ, `obs_boot` the row the bootstrap value is of;
        `self.obs` stays the true observation."""
        T = self.b_obs.shape[0]
        obs_all, rew = out["obs"].to(torch.float32), out["reward"].to(torch.float32)
        nan = torch.isnan(rew).to(torch.int64) + torch.isnan(obs_all[1:]).any(-1)
        obs_all = torch.nan_to_num(obs_all, nan=0.0, posinf=0.0, neginf=0.0)    # what the kernel fed the networks
        if out.get("obs_read") is not None:
            read = torch.nan_to_num(out["obs_read"].to(torch.float32), nan=0.0, posinf=0.0, neginf=0.0)
            self.b_obs.copy_(read[:T])
            self.obs_boot.copy_(read[T])
        else:
            self.b_obs.copy_(obs_all[:T])
        self.obs.copy_(obs_all[T])
        self.b_act.copy_(out["actions"].to(torch.float32).unsqueeze(-1))
        self.b_val.copy_(out["values"].to(torch.float32))
        self.b_logp.copy_(out["logp"].to(torch.float32))
        self.b_rew.copy_(torch.nan_to_num(rew, nan=0.0))
        self.b_done.copy_(out["done"])
        self.b_epret.copy_(out["episode_return"].to(torch.float32))
        self.b_eplen.copy_(out["episode_steps"])
        self.b_outcome.copy_(out["outcome"])
        return nan

    def _evaluate_rows(self, policies, group, n_episodes, rng, disturbance=None):
        """evaluate_policies_fused() of `policies` on `n_episodes` fresh episodes drawn from `rng`: rows = policies."""
        from . import reset_parity
        from .policy import evaluate_policies_fused
        own, trf, goal = reset_parity.draw_episodes(self.venv.config, n_episodes, rng)
        return evaluate_policies_fused(policies, own, trf, goal, dtype=self.venv.dtype, device=self.device,
                                       config=self.venv.config, group=group,
                                       **({} if disturbance is None else {"disturbance": disturbance}))

    disturbances = None                                   # a DisturbanceSet: the trainer collects under it

    def _set_disturbances(self, disturbances, n_members, who):
        """The trainer's `disturbances` (a DisturbanceSet, or None) from its argument: checked here, before any launch."""
        from .policy import DisturbanceSet
        if disturbances is None:
            return
        if getattr(self.venv, "dtype", torch.float32) != torch.float32:
            raise ValueError("%s: training under a disturbance is float32 only, this env is %s" % (who, self.venv.dtype))
        self.disturbances = (disturbances if isinstance(disturbances, DisturbanceSet)
                             else DisturbanceSet(disturbances, n_members))
        if len(self.disturbances) != n_members:
            raise ValueError("%s: %d disturbances for %d member(s)" % (who, len(self.disturbances), n_members))

    def state_dict(self):
        """What of a run lies neither in the policy zips nor in the reward normaliser's state: the disturbance it trains
        under ({"disturbance": None} without one)."""
        return {"disturbance": None if self.disturbances is None else self.disturbances.state_dict()}

    def load_state_dict(self, sd):
        """Refuses a state saved under another disturbance (or under none, or one where this run has none)."""
        saved = sd.get("disturbance")
        if self.disturbances is None:
            if saved is not None:
                raise ValueError("load_state_dict: the state was saved under the disturbance %s, this run trains under none"
                                 % (saved,))
            return
        self.disturbances.load_state_dict(saved)

    def _learn(self, total_timesteps, log, books, history, iterate, evaluate, eval_every, checkpoint_every):
        """learn() for the learners whose bookkeeping `books` holds (one _Callbacks each): iterate() runs one iteration
        and returns per learner the update's statistics, the recent episodes and the NaN events so far; evaluate() gives
        evaluate_policies_fused()'s dict, one row per learner."""
        self.total_timesteps = total_timesteps            # (update() takes its schedules' progress_remaining from it)
        try:
            return self._learn_loop(total_timesteps, log, books, history, iterate, evaluate, eval_every, checkpoint_every)
        finally:
            self.total_timesteps = None

    def _progress_remaining(self):
        """SB3's progress_remaining for the update about to run: 1 - num_timesteps / total_timesteps inside learn(),
        clamped at 0 (a departure from SB3, stated: the last iteration may overshoot total_timesteps, and would otherwise
        train with a negative rate); 1.0 outside learn()."""
        total = getattr(self, "total_timesteps", None)
        return 1.0 if not total else max(0.0, 1.0 - self.num_timesteps / total)

    def _learn_loop(self, total_timesteps, log, books, history, iterate, evaluate, eval_every, checkpoint_every):
        t0 = time.time()
        it = 0
        while self.num_timesteps < total_timesteps:
            before = self.num_timesteps
            stats, eps, nan = iterate()
            it += 1
            for k, book in enumerate(books):
                rec = {**book.head, "iteration": it, "timesteps": self.num_timesteps,
                       "fps": self.num_timesteps / max(time.time() - t0, 1e-9), **(eps[k] or {}), **stats[k],
                       "nan_events": int(nan[k])}
                history.append(rec)
                if log:
                    log(rec)
            crossed = lambda every: bool(every) and before // every < self.num_timesteps // every  # noqa: E731
            if crossed(eval_every):
                out = evaluate()
                for k, book in enumerate(books):
                    erec = book.evaluated(self.num_timesteps, out["total_reward"][k], out["steps"][k], out["outcome"][k],
                                          out["unfinished"][k])
                    history.append(erec)
                    if log:
                        log(erec)
            if crossed(checkpoint_every):
                for book in books:
                    book.checkpoint(self.num_timesteps)
        return history


class PPOTrainer(_Trainer):
    """collector: "graphs" (default on a GPU: one captured env step replayed n_steps times), "fused" (the whole
    collection of an iteration in ONE hand-written launch, ACAS2DVecEnv.collect(): actor, critic, Gaussian sampling
    and the env step inside the kernel; its noise comes from the kernel's own Philox stream instead of torch's
    generator; float32 envs with 16, 32 or 64 traffic aircraft take the launch whose lanes share an env's network,
    ACAS2DVecEnv.collect(group=True), and so does evaluate()) or "eager" (op by op).  updater: "graphs" (default with
    `use_graphs`: one captured minibatch update of torch ops) or "fused" (FusedUpdate: the minibatch update as two
    hand-written launches, its own Adam state; obs_dim in {8, 11, 14, 17, 29} or {53, 101, 197}, i.e. n_traffic 1, 2, 3,
    4, 8 or 16, 32, 64).  gae: None / "torch" (compute_gae: captured with `use_graphs`) or "kernel" (gae_fused: one
    hand-written launch on the static buffers, the bootstrap value still torch's forward, so the run is the "torch" run
    bit for bit; with `use_graphs` and collector="fused" only).
    config.target_kl (SB3's early stop): with updater="fused" the decision is taken on the device (FusedUpdate's guarded
    entry: every minibatch is still launched, the host learns of a stop from update()'s statistics), op by op it is
    SB3's break before the optimizer step; the captured torch-op updater cannot stop and rejects it.  diagnostics=True
    (updater="fused"): the guarded entry without a limit.  Either adds approx_kl, clip_fraction, n_applied, early_stop and
    explained_variance to update()'s statistics; without both, update() issues the launches it always did.
    config.clip_range_vf and the three schedules: with updater="fused" inside FusedUpdate's kernels (its `options`
    entry, guarded by implication), op by op through effective_config() -- the optimizer's lr is set per update; the
    captured torch-op updater holds its numbers in a fixed graph and rejects them.  Inside learn() an update runs at
    progress_remaining = max(0, 1 - num_timesteps / total_timesteps), outside it at 1; its statistics then carry the
    effective learning_rate, clip_range and (where set) clip_range_vf.
    reward_norm: None, True (SB3's VecNormalize(norm_obs=False, norm_reward=True) defaults, gamma from the config) or a
    RewardNormalizer; with collector="fused" only.  collect() then normalises b_rew in place (one RewardNormalizer.normalize
    call) before GAE, so GAE, the update and clip_range_vf see normalised rewards; episode returns (b_epret) and evaluate()
    stay raw, update()'s statistics gain reward_std, and learn() saves the normaliser's state beside every zip.  It is an
    env wrapper in SB3, not a hyper-parameter: PPOConfig has no field for it.  None: the calls issued are the same.
    disturbance: None or a policy.Disturbance -- train under white sensor noise and actuator disturbance, with
    collector="fused" only (ACAS2DVecEnv.collect(disturbance=): the noise is drawn inside that launch; the other collectors
    have no such step).  The actor AND the critic read the disturbed rows, b_obs holds exactly those, b_act the raw draws
    (actuator noise is the environment's), and the bootstrap value is the critic's on the disturbed row the next
    collection's first step reads: torch's forward of it, or with gae="kernel" at n_traffic 1, 2, 3, 4, 8 gae_fused's own
    critic on obs_last = that row (then the bits of the next values[0]).  It is part of the env, as reward_norm is: it goes
    into state_dict() and beside every saved zip, and evaluate(disturbance=) scores under any other.  A zero Disturbance
    trains the undisturbed run bit for bit (gae="kernel" aside, whose bootstrap value is then the kernel's).
    A policy.CorrelatedDisturbanceSet of one member in its place trains under time-correlated and biased errors
    (acas2d_collect_set_correlated_*): the set holds the per-env error state between the collection launches, everything
    above stays as said, and with every rho 0 it trains the white run's bits.  A bare CorrelatedDisturbance is refused."""

    def __init__(self, venv, config=None, policy=None, use_graphs=None, collector=None, updater=None, gae=None,
                 diagnostics=False, reward_norm=None, disturbance=None):
        self.venv = venv
        self.cfg = config or PPOConfig()
        torch.manual_seed(self.cfg.seed)
        self.device = venv.device
        self.policy = (policy or ActorCritic(venv.obs_dim)).to(self.device)
        self.use_graphs = (torch.device(self.device).type == "cuda") if use_graphs is None else bool(use_graphs)
        self.collector = collector or ("graphs" if self.use_graphs else "eager")
        if self.collector not in ("graphs", "fused", "eager") or (self.collector != "eager" and not self.use_graphs):
            raise ValueError("collector %r needs use_graphs" % (self.collector,))
        self._fused_out = None
        if disturbance is not None and not (self.use_graphs and self.collector == "fused"):
            raise ValueError("disturbance (training under sensor and actuator noise) is supported with use_graphs and "
                             "collector='fused' only: the noise is drawn inside the fused collection launch, the captured and "
                             "the op-by-op collectors have no such step; got use_graphs=%r, collector=%r"
                             % (self.use_graphs, self.collector))
        self._set_disturbances(disturbance, 1, "PPOTrainer")
        if self.collector == "graphs" and getattr(venv, "double_buffer", False):
            # ONE captured env step is replayed n_steps times: every replay must read what the previous one wrote,
            # which the double-buffered step (read generation g, write 1 - g) does not give a single-step graph
            venv.set_double_buffer(False)
        self.updater = updater or "graphs"
        if self.updater not in ("graphs", "fused") or (self.updater == "fused" and not self.use_graphs):
            raise ValueError("updater %r needs use_graphs" % (self.updater,))
        self._fused_update = None
        self.diagnostics = bool(diagnostics)
        if (self.cfg.target_kl is not None and self.use_graphs or self.diagnostics) and not (
                self.use_graphs and self.updater == "fused"):
            raise ValueError("target_kl and diagnostics=True need updater='fused' (the stop is decided inside its kernels) "
                             "or use_graphs=False (target_kl only: SB3's break, op by op); the captured torch-op updater "
                             "replays a fixed graph and cannot stop -- got use_graphs=%r, updater=%r"
                             % (self.use_graphs, self.updater))
        if has_options(self.cfg) and self.use_graphs and self.updater != "fused":
            raise ValueError("clip_range_vf and the schedules need updater='fused' (they are applied inside its kernels) or "
                             "use_graphs=False (op by op); the captured torch-op updater replays a fixed graph with the "
                             "numbers it was captured with -- got use_graphs=%r, updater=%r" % (self.use_graphs, self.updater))
        self.total_timesteps = None
        self.gae = gae or "torch"
        if self.gae not in ("torch", "kernel"):
            raise ValueError("gae must be None, 'torch' or 'kernel', got %r" % (gae,))
        if self.gae == "kernel" and not (self.use_graphs and self.collector == "fused"):
            raise ValueError("gae='kernel' (gae_fused on the static rollout buffers) is supported with use_graphs and "
                             "collector='fused' only; got use_graphs=%r, collector=%r -- use gae='torch'"
                             % (self.use_graphs, self.collector))
        self._gae_constants = None
        self.reward_norm = None
        if reward_norm is not None and not (self.use_graphs and self.collector == "fused"):
            raise ValueError("reward_norm (RewardNormalizer on the static rollout buffers) is supported with use_graphs and "
                             "collector='fused' only; got use_graphs=%r, collector=%r" % (self.use_graphs, self.collector))
        # the hand-written launches exist for the observation widths / traffic counts below: say so HERE, not at the
        # first collect() / update() of a run
        f32 = getattr(venv, "dtype", torch.float32) == torch.float32
        # float32 at 16, 32 or 64 traffic aircraft: the launches whose lanes share an env's network (group=True)
        self._group = f32 and venv.n_traffic in GROUP_TRAFFIC
        if self.collector == "fused" and not self._group and venv.n_traffic not in ((1, 2, 3, 4, 8) if f32 else (1, 2, 3)):
            raise ValueError("collector='fused' needs a thread-per-env work shape: n_traffic in {1, 2, 3, 4, 8} (float32) / "
                             "{1, 2, 3} (float64), or the group-cooperative float32 launch: n_traffic in {16, 32, 64}; "
                             "got %d -- use collector='graphs'" % venv.n_traffic)
        if self.updater == "fused" and venv.obs_dim not in FUSED_UPDATE_WIDTHS + FUSED_UPDATE_WIDE_WIDTHS:
            raise ValueError("updater='fused' is built for obs_dim in {8, 11, 14, 17, 29} (n_traffic 1, 2, 3, 4, 8) and "
                             "{53, 101, 197} (n_traffic 16, 32, 64), got %d -- use updater='graphs'" % venv.obs_dim)
        # (fused: one multi-tensor kernel for the 13 parameter tensors instead of ~10 foreach launches)
        self.opt = torch.optim.Adam(self.policy.parameters(), lr=self.cfg.learning_rate, eps=1e-5,
                                    capturable=self.use_graphs, **({"fused": True} if self.use_graphs else {}))
        self.obs = venv.reset().to(torch.float32).clone()
        # the row the bootstrap value is taken on: the observation itself, or (disturbed) what the critic would read of it
        self.obs_boot = self.obs if self.disturbances is None else self.obs.clone()
        if reward_norm is not None:
            self.reward_norm = _reward_normalizer_for(reward_norm, venv.num_envs, [self.cfg], self.device)
        # Exact parallel flight makes the reference's d_cpa 0/0 = NaN (kinematics.py:48), and its reward
        # with it when the aircraft is traffic[0]; the engine reproduces that.  In float64 it all but
        # never happens; in float32 headings coincide bit for bit about once per 2e7 env steps, and one
        # NaN poisons PPO for good -- so the collector replaces non-finite observations / rewards by 0
        # (what SB3 users wrap such envs in VecCheckNan for) and counts the events.
        self.nan_events = torch.zeros((), dtype=torch.int64, device=self.device)
        self.num_timesteps = 0
        self.ep_returns, self.ep_lengths, self.ep_outcomes = [], [], []
        self._graphs = None

    def _alloc(self):
        """The rollout buffers (static: the graphs write into them) and the collector graph's row counter."""
        self._alloc_rollout()
        self.t_idx = torch.zeros(1, dtype=torch.int64, device=self.device)

    def _collect_step(self):
        """One env step of SB3's collect_rollouts into row t_idx of the buffers (graph-capturable:
        no host reads, the row index lives on the device)."""
        v, t = self.venv, self.t_idx
        mean, value = self.policy.forward(self.obs)
        log_std = self.policy.log_std
        action = mean + log_std.exp() * torch.randn_like(mean)
        logp = _normal_logp(mean, log_std, action)
        self.b_obs.index_copy_(0, t, self.obs.unsqueeze(0))
        self.b_act.index_copy_(0, t, action.unsqueeze(0))
        self.b_val.index_copy_(0, t, value.unsqueeze(0))
        self.b_logp.index_copy_(0, t, logp.unsqueeze(0))
        # the env sees the clipped action, the buffer keeps the raw one (SB3 collect_rollouts)
        v.actions_buffer.copy_(action.clamp(-1.0, 1.0).reshape(-1))
        v.step_inplace()
        out = v.outputs
        rew, nxt = out["reward"].to(torch.float32), out["obs"].to(torch.float32)
        self.nan_events.add_(torch.isnan(rew).sum() + torch.isnan(nxt).any(-1).sum())
        self.b_rew.index_copy_(0, t, torch.nan_to_num(rew, nan=0.0).unsqueeze(0))
        self.b_done.index_copy_(0, t, out["done"].view(torch.bool).unsqueeze(0))
        self.b_epret.index_copy_(0, t, out["episode_return"].to(torch.float32).unsqueeze(0))
        self.b_eplen.index_copy_(0, t, out["episode_steps"].unsqueeze(0))
        self.b_outcome.index_copy_(0, t, out["outcome"].unsqueeze(0))
        self.obs.copy_(torch.nan_to_num(nxt, nan=0.0))
        t.add_(1)

    def _gae(self):
        _, last_value = self.policy.forward(self.obs_boot)
        adv, ret = compute_gae(self.b_rew, self.b_val, self.b_done, last_value, self.cfg.gamma, self.cfg.gae_lambda)
        self.b_adv.copy_(adv)
        self.b_ret.copy_(ret)

    def _minibatch(self, idx):
        """One PPO minibatch update on the rows named by a static index buffer."""
        T, E = self.cfg.n_steps, self.venv.num_envs
        flat = lambda x: x.reshape(T * E, *x.shape[2:])  # noqa: E731
        # (torch.distributions validates its arguments with a host read: not capturable -- ppo_loss() does not use it)
        # (with updater="fused" this body is only warmed up and captured, never replayed; clip_range_vf gets its old_val)
        loss, pg, vf = ppo_loss(self.policy, self.cfg, flat(self.b_obs)[idx], flat(self.b_act)[idx],
                                flat(self.b_logp)[idx], flat(self.b_adv)[idx], flat(self.b_ret)[idx],
                                None if self.cfg.clip_range_vf is None else flat(self.b_val)[idx])
        loss.backward()
        nn.utils.clip_grad_norm_(self.policy.parameters(), self.cfg.max_grad_norm)
        self.opt.step()
        return pg.detach(), vf.detach()

    def _capture(self):
        """Warm the three bodies up on a side stream, then capture them (PyTorch's whole-network
        capture recipe: gradients are None at capture time, so backward assigns static buffers).
        The warm-up steps the env and takes real optimizer steps on an all-zero buffer: the env, the
        observation, the parameters and the Adam state are put back IN PLACE afterwards (the graphs
        hold their addresses), so training starts from exactly the state it was constructed in."""
        self._alloc()
        self.mb_idx, self.mb_tail = minibatch_buffers(self.cfg.n_steps * self.venv.num_envs, self.cfg.batch_size, self.device)
        env_before = self.venv.state_dict()
        obs_before, env_obs_before = self.obs.clone(), self.venv.outputs["obs"].clone()
        params_before = [p.detach().clone() for p in self.policy.parameters()]
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            with torch.no_grad():
                for _ in range(2):
                    self.t_idx.zero_()
                    self._collect_step()
                self._gae()
            for idx in (self.mb_idx, self.mb_idx, self.mb_tail):
                if idx is not None:
                    self.opt.zero_grad(set_to_none=True)
                    self._minibatch(idx)
        torch.cuda.current_stream(self.device).wait_stream(side)
        g_step, g_gae, g_upd = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        self.t_idx.zero_()
        with torch.no_grad():
            with torch.cuda.graph(g_step):
                self._collect_step()
            with torch.cuda.graph(g_gae):
                self._gae()
        self.opt.zero_grad(set_to_none=True)
        with torch.cuda.graph(g_upd):
            self._pg, self._vf = self._minibatch(self.mb_idx)
        g_tail = None
        if self.mb_tail is not None:                      # the last, partial minibatch of an epoch: its own static shape
            g_tail = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g_tail):
                self._minibatch(self.mb_tail)
        self._graphs = (g_step, g_gae, g_upd, g_tail)
        with torch.no_grad():
            for p, q in zip(self.policy.parameters(), params_before):
                p.copy_(q)
            for st in self.opt.state.values():
                for v in st.values():
                    if torch.is_tensor(v):
                        v.zero_()                         # exp_avg, exp_avg_sq, step: a fresh Adam
            self.venv.load_state_dict(env_before)
            self.venv.outputs["obs"].copy_(env_obs_before)
            self.obs.copy_(obs_before)
            self.obs_boot.copy_(obs_before)
            self.nan_events.zero_()
            self.t_idx.zero_()

    def collect(self):
        cfg, E, T = self.cfg, self.venv.num_envs, self.cfg.n_steps
        if self.use_graphs:
            if self._graphs is None:
                self._capture()
            if self.collector == "fused":
                # one launch: rows t = 0 .. T-1 of the static buffers, then the captured GAE as usual
                out = self.venv.collect(self.policy, T, noise_seed=cfg.seed, noise_step=self.num_timesteps // E,
                                        out=self._fused_out, group=self._group,
                                        **({} if self.disturbances is None else {"disturbance": self.disturbances}))
                self._fused_out = out
                self.nan_events.add_(self._store_collection(out).sum())
                if self.reward_norm is not None:
                    self.reward_norm.normalize(self.b_rew, self.b_done, out=self.b_rew)
            else:
                self.t_idx.zero_()
                for _ in range(T):
                    self._graphs[0].replay()
            if self.gae == "kernel":
                if self._gae_constants is None:
                    self._gae_constants = gae_constants(cfg.gamma, cfg.gae_lambda, 1, self.device)
                if self.disturbances is not None and self.venv.obs_dim in GAE_BOOTSTRAP_WIDTHS:
                    # the kernel's own critic on the row the next collection's first step reads: the bits of its values[0]
                    gae_fused(self.b_rew, self.b_val, self.b_done, None, critic=self.policy, obs_last=self.obs_boot,
                              constants=self._gae_constants, out={"adv": self.b_adv, "ret": self.b_ret})
                else:
                    with torch.no_grad():
                        _, last_value = self.policy.forward(self.obs_boot)
                    gae_fused(self.b_rew, self.b_val, self.b_done, last_value, constants=self._gae_constants,
                              out={"adv": self.b_adv, "ret": self.b_ret})
            else:
                self._graphs[1].replay()
            done = self.b_done
            if bool(done.any()):                          # the iteration's one host synchronisation
                self.ep_returns.append(self.b_epret[done].cpu())
                self.ep_lengths.append((self.b_eplen[done] - 1).cpu())
                self.ep_outcomes.append(self.b_outcome[done].cpu())
            self.num_timesteps += T * E
            return None
        dev = self.device
        b_obs = torch.empty(T, E, self.venv.obs_dim, dtype=torch.float32, device=dev)
        b_act = torch.empty(T, E, 1, dtype=torch.float32, device=dev)
        b_logp = torch.empty(T, E, dtype=torch.float32, device=dev)
        b_val = torch.empty(T, E, dtype=torch.float32, device=dev)
        b_rew = torch.empty(T, E, dtype=torch.float32, device=dev)
        b_done = torch.empty(T, E, dtype=torch.bool, device=dev)
        with torch.no_grad():
            for t in range(T):
                dist, value = self.policy.distribution(self.obs)
                action = dist.sample()
                b_obs[t], b_act[t], b_val[t] = self.obs, action, value
                b_logp[t] = dist.log_prob(action).sum(-1)
                # the env sees the clipped action, the buffer keeps the raw one (SB3 collect_rollouts)
                obs, rew, done, infos = self.venv.step(action.clamp(-1.0, 1.0).to(self.venv.dtype))
                self.nan_events += torch.isnan(rew).sum() + torch.isnan(obs).any(-1).sum()
                b_rew[t], b_done[t] = torch.nan_to_num(rew.to(torch.float32), nan=0.0), done
                if bool(done.any()):
                    self.ep_returns.append(infos.episode_return[done].float().cpu())
                    self.ep_lengths.append((infos.episode_steps[done] - 1).cpu())
                    self.ep_outcomes.append(infos.outcome[done].cpu())
                self.obs = torch.nan_to_num(obs.to(torch.float32), nan=0.0)
            _, last_value = self.policy.forward(self.obs)
            adv, ret = compute_gae(b_rew, b_val, b_done, last_value, cfg.gamma, cfg.gae_lambda)
        self.num_timesteps += T * E
        flat = lambda x: x.reshape(T * E, *x.shape[2:])  # noqa: E731
        return flat(b_obs), flat(b_act), flat(b_logp), flat(adv), flat(ret), flat(b_val)

    def update(self, obs=None, act=None, old_logp=None, adv=None, ret=None, old_val=None):
        cfg = self.cfg
        if self.use_graphs and self.updater == "fused":
            n = cfg.n_steps * self.venv.num_envs
            if self._fused_update is None:
                self._fused_update = FusedUpdate(self.policy, cfg, self.b_obs, self.b_act, self.b_logp, self.b_adv, self.b_ret,
                                                 diagnostics=self.diagnostics, old_val=self.b_val)
            fu = self._fused_update
            fu.begin_update(self._progress_remaining())
            for _ in range(cfg.n_epochs):
                for idx in minibatch_schedule(torch.randperm(n, device=self.device), self.mb_idx, self.mb_tail):
                    fu.step(idx)
            st = fu.last_losses()
            out = {"pg_loss": st["pg_loss"], "value_loss": st["value_loss"], "std": self.policy.log_std.detach().exp().item()}
            if fu.guarded:
                d = fu.diagnostics()
                out.update({k: d[k] for k in ("approx_kl", "clip_fraction", "n_applied", "early_stop")})
                out["explained_variance"] = explained_variance(self.b_val.reshape(-1), self.b_ret.reshape(-1)).item()
            if fu.options:
                out.update(fu.effective()[0])
            if self.reward_norm is not None:
                out["reward_std"] = self.reward_norm.reward_std().item()
            return out
        if self.use_graphs:
            n = cfg.n_steps * self.venv.num_envs
            for _ in range(cfg.n_epochs):
                for idx in minibatch_schedule(torch.randperm(n, device=self.device), self.mb_idx, self.mb_tail):
                    # whole minibatches: one static shape; the partial one SB3 also takes: its own graph
                    self._graphs[2 if idx is self.mb_idx else 3].replay()
            return {"pg_loss": self._pg.item(), "value_loss": self._vf.item(),
                    "std": self.policy.log_std.detach().exp().item(),
                    **({} if self.reward_norm is None else {"reward_std": self.reward_norm.reward_std().item()})}
        n = obs.shape[0]
        stats = {}
        options = has_options(cfg)
        if options:                                       # this update's numbers: the schedules at progress_remaining
            cfg = effective_config(cfg, self._progress_remaining())
            for group in self.opt.param_groups:
                group["lr"] = cfg.learning_rate
            if cfg.clip_range_vf is not None and old_val is None:
                raise ValueError("update(): clip_range_vf needs old_val, the rollout's values")
        kls, cfs, n_applied, go_on = [], [], 0, True
        for _ in range(cfg.n_epochs):
            perm = torch.randperm(n, device=self.device)
            for i in range(0, n, cfg.batch_size):
                idx = perm[i:i + cfg.batch_size]
                if idx.numel() < 2:
                    continue                              # a one-row tail has no advantage standard deviation
                loss, pg, vf = ppo_loss(self.policy, cfg, obs[idx], act[idx], old_logp[idx], adv[idx], ret[idx],
                                        None if cfg.clip_range_vf is None else old_val.reshape(-1)[idx])
                if cfg.target_kl is not None:             # SB3: measured under no_grad, the break before the optimizer step
                    kl, cf = approx_kl_and_clip_fraction(self.policy, cfg, obs[idx], act[idx], old_logp[idx])
                    kls.append(kl.item())
                    cfs.append(cf.item())
                    if kls[-1] > 1.5 * cfg.target_kl:
                        go_on = False
                        break
                self.opt.zero_grad(set_to_none=True)
                loss.backward()
                nn.utils.clip_grad_norm_(self.policy.parameters(), cfg.max_grad_norm)
                self.opt.step()
                n_applied += 1
            stats = {"pg_loss": pg.item(), "value_loss": vf.item(), "std": self.policy.log_std.detach().exp().item()}
            if not go_on:
                break
        if cfg.target_kl is not None:
            stats.update({"approx_kl": float(np.mean(kls)), "clip_fraction": float(np.mean(cfs)), "n_applied": n_applied,
                          "early_stop": not go_on})
            if old_val is not None:
                stats["explained_variance"] = explained_variance(old_val.reshape(-1), ret.reshape(-1)).item()
        if options:
            stats.update({"learning_rate": cfg.learning_rate, "clip_range": cfg.clip_range,
                          **({} if self.cfg.clip_range_vf is None else {"clip_range_vf": cfg.clip_range_vf or 0.0})})
        return stats

    def optimizer_state(self):
        """The Adam state that is actually being stepped: with updater='fused' the moments live in FusedUpdate's
        flat buffers (layout: actor w1 b1 w2 b2 w3 b3, critic likewise, log_std -- include/acas2d.h) and `self.opt`
        is never stepped; otherwise `self.opt.state_dict()`."""
        if self.updater == "fused" and self.use_graphs:
            fu = self._fused_update
            if fu is None:
                return {"updater": "fused", "step": 0, "exp_avg": None, "exp_avg_sq": None}
            return {"updater": "fused", "step": int(fu.step_count.item()), "exp_avg": fu.m, "exp_avg_sq": fu.v}
        return {"updater": self.updater, **self.opt.state_dict()}

    def recent_episodes(self, clear=True):
        out = episode_summary(self.ep_returns, self.ep_lengths, self.ep_outcomes)
        if clear:
            self.ep_returns, self.ep_lengths, self.ep_outcomes = [], [], []
        return out

    def evaluate(self, n_episodes, rng, disturbance=None):
        """Score the current actor deterministically on `n_episodes` fresh episodes drawn from `rng` (a `random.Random`
        fed to reset_parity, like the reference's eval env) in one launch (policy.evaluate_policies_fused, K = 1).
        Touches neither the training env, nor the captured graphs, nor any torch random stream.  disturbance: a
        policy.Disturbance handed to evaluate_policies_fused (None: the nominal score, also of a learner that trains
        under one)."""
        out = self._evaluate_rows([self.policy], self._group, n_episodes, rng, disturbance)
        return {k: (v[0] if k != "unfinished" else int(v[0])) for k, v in out.items()}

    def learn(self, total_timesteps, log=print, eval_every=None, eval_episodes=10, eval_seed=None, save_dir=None,
              checkpoint_every=None):
        """Run PPO iterations until `total_timesteps` env steps.  Off by default, SB3's callbacks as training_main.py
        sets them up:
          eval_every        EvalCallback: at each iteration boundary that crosses a multiple of `eval_every` timesteps,
                            score the deterministic actor on `eval_episodes` fresh episodes from ONE
                            random.Random(eval_seed) (default: the config's seed) kept for the whole run; the record
                            joins the history, and with `save_dir` the scores are appended to
                            save_dir/results/evaluations.npz (timesteps [n], results [n, eval_episodes] returns,
                            ep_lengths [n, eval_episodes] = steps - 1) and save_dir/best_model.zip is written whenever
                            the mean return beats the best so far
          checkpoint_every  CheckpointCallback: save_dir/checkpoints/model_<num_timesteps>_steps.zip at each boundary
                            that crosses a multiple of `checkpoint_every` timesteps
        Neither changes the training: the evaluation runs on an env of its own and draws no torch random numbers."""
        if checkpoint_every and not save_dir:
            raise ValueError("checkpoint_every needs save_dir")
        if eval_every:
            f32 = self.venv.dtype == torch.float32
            if not self._group and self.venv.n_traffic not in ((1, 2, 3, 4, 8) if f32 else (1, 2, 3, 4)):
                raise ValueError("eval_every needs a thread-per-env work shape: n_traffic in {1, 2, 3, 4, 8} (float32) / "
                                 "{1, 2, 3, 4} (float64), or the group-cooperative float32 launch: n_traffic in "
                                 "{16, 32, 64}; got %d" % self.venv.n_traffic)
            eval_rng = random.Random(self.cfg.seed if eval_seed is None else eval_seed)

        def iterate():
            batch = self.collect()
            stats = self.update() if batch is None else self.update(*batch)
            return [stats], [self.recent_episodes()], [self.nan_events]

        books = [_Callbacks(save_dir, lambda: self.policy,
                            reward_norm=self.reward_norm and self.reward_norm.state_dict,
                            disturbance=self.disturbances and self.disturbances.members[0].to_dict())]
        return self._learn(total_timesteps, log, books, [], iterate,
                           lambda: self._evaluate_rows([self.policy], self._group, eval_episodes, eval_rng), eval_every,
                           checkpoint_every)


# ---- K learners at once: the seeds or hyper-parameter sets of a sweep as ONE population ---------------------------------
# what may differ between the members of a population, and what the shared launches need equal
MEMBER_FIELDS = ("seed", "learning_rate", "clip_range", "ent_coef", "vf_coef", "max_grad_norm", "gamma", "gae_lambda",
                 "target_kl", "clip_range_vf") + SCHEDULE_FIELDS
SHARED_FIELDS = ("n_steps", "batch_size", "n_epochs")
# (HYPER_SLOTS, the row a member's hyper-parameters travel in, is defined beside hyper_row() above)


class ActorCriticSet:
    """K `ActorCritic`s held as [K, ...] stacks: `params[name]` is the float32 tensor of the K members' `name`
    (PARAM_NAMES, torch layouts) -- what acas2d_ppo_update_set_f32 updates in place and, transposed,
    acas2d_collect_set_f32 reads."""

    def __init__(self, n_members, obs_dim, device="cpu"):
        self.n_members, self.obs_dim = int(n_members), int(obs_dim)
        like = ActorCritic(obs_dim)
        self.params = {n: torch.zeros((self.n_members,) + tuple(like.get_parameter(n).shape), dtype=torch.float32,
                                      device=device) for n in PARAM_NAMES}

    @classmethod
    def from_members(cls, members, device=None):
        members = list(members)
        if not members:
            raise ValueError("ActorCriticSet.from_members needs at least one member")
        D = members[0].mlp_extractor.policy_net[0].in_features
        dev = members[0].log_std.device if device is None else device
        out = cls(len(members), D, dev)
        with torch.no_grad():
            for k, m in enumerate(members):
                if m.mlp_extractor.policy_net[0].in_features != D:
                    raise ValueError("every member must have obs_dim %d" % D)
                for n in PARAM_NAMES:
                    out.params[n][k].copy_(m.get_parameter(n).detach().to(torch.float32))
        return out

    @property
    def device(self):
        return self.params["log_std"].device

    def to(self, device):
        self.params = {n: t.to(device) for n, t in self.params.items()}
        return self

    def member(self, k):
        """A fresh `ActorCritic` holding a copy of member k's parameters, bit for bit."""
        m = ActorCritic(self.obs_dim)
        with torch.no_grad():
            for n in PARAM_NAMES:
                m.get_parameter(n).copy_(self.params[n][k].cpu())
        return m.to(self.device)

    def actor_weights(self):
        """K tuples (w1 [64,D], b1, w2 [64,64], b2, w3 [1,64], b3): the `policies` of evaluate_policies_fused()."""
        return [tuple(self.params[n][k].detach() for n in PARAM_NAMES[:6]) for k in range(self.n_members)]

    def collector_weights(self):
        """The 13 stacks as acas2d_collect_set_f32 takes them: the first two layers of each net transposed
        ([K][D][64], [K][64][64]), the heads and biases flat, log_std [K]."""
        p = self.params
        return (kernel_layout(*(p[n] for n in PARAM_NAMES[:6])) + kernel_layout(*(p[n] for n in PARAM_NAMES[6:12]))
                + [p["log_std"].detach().reshape(self.n_members).contiguous()])

    @torch.no_grad()
    def values(self, obs):
        """The K critics on their own envs: obs [K * EM, D] (member k's rows [k EM, (k + 1) EM)) -> [K * EM]."""
        p, K = self.params, self.n_members
        x = obs.to(torch.float32).reshape(K, -1, self.obs_dim)
        pre = "mlp_extractor.value_net."
        h = torch.tanh(torch.baddbmm(p[pre + "0.bias"].unsqueeze(1), x, p[pre + "0.weight"].transpose(1, 2)))
        h = torch.tanh(torch.baddbmm(p[pre + "2.bias"].unsqueeze(1), h, p[pre + "2.weight"].transpose(1, 2)))
        return torch.baddbmm(p["value_net.bias"].unsqueeze(1), h, p["value_net.weight"].transpose(1, 2)).reshape(-1)


class FusedUpdateSet(_FusedUpdater):
    """FusedUpdate for the K members of an `ActorCriticSet` in two launches whatever K is (acas2d_ppo_update_set_f32,
    csrc/acas2d_ppo_set.hip; for obs_dim 53, 101, 197 acas2d_ppo_update_wide_set_f32, csrc/acas2d_ppo_wide_set.hip --
    `entry` names the one chosen).  `obs` [n, D], `act` / `old_logp` / `adv` / `ret` [n] are ONE flat float32 rollout buffer
    shared by the members (their storage must stay put); `step(idx)` takes an int64 device tensor [K, B]: row k names
    member k's minibatch as rows of that buffer.  `hyper` is a float32 device tensor [K, 8] (HYPER_SLOTS) the kernels
    read at every call: rewrite it between calls to change a member's learning rate, clip range, ...  Keeps the
    members' Adam moments and step counts ([K, ...]).  float32.
    Where a member's config has a `target_kl`, or with `diagnostics=True`, every step goes through
    acas2d_ppo_update_guarded_set_f32 instead (`guarded`; csrc/acas2d_ppo_guard.hip): `target_kl` is a float32 device
    tensor [K] (0: no limit) beside `hyper`, `stopped` int32 [K] and `diag` float32 [K, 8] are the kernels'.  Call
    begin_update() once per PPO update, step() for every minibatch -- a stopped member's share of the two launches
    returns at once -- and read diagnostics() afterwards.  Where a member's config has a `clip_range_vf` or a schedule
    the guarded steps go through acas2d_ppo_update_sb3_set_f32 (`options`; csrc/acas2d_ppo_sb3.hip): `old_val` [n] is the
    rollout's values, `clip_range_vf` a float32 device tensor [K] (0: plain MSE) and `scale` [K, 4] the factors that
    begin_update(progress_remaining) writes; the kernels multiply them into the `hyper` rows as they are at that moment.
    Otherwise the calls are the ones above."""

    _symbol, _got = 2, ", float32; got"

    def __init__(self, policy_set, configs, obs, act, old_logp, adv, ret, beta1=0.9, beta2=0.999, adam_eps=1e-5,
                 diagnostics=False, old_val=None):
        D, K = obs.shape[-1], policy_set.n_members
        self._entry_for(D)
        if len(configs) != K or policy_set.obs_dim != D:
            raise ValueError("FusedUpdateSet needs one config per member and members of obs_dim %d" % D)
        super().__init__([policy_set.params[name] for name in PARAM_NAMES], list(configs), (obs, act, old_logp, adv, ret),
                         (K,), beta1, beta2, adam_eps, diagnostics, old_val)
        self.policy_set, self.K = policy_set, K

    def step(self, idx, apply=True):
        """One minibatch update of every member; apply=False leaves the raw gradients in `grad` and applies nothing (the
        unguarded entry: a probe has no stop to decide)."""
        assert idx.dim() == 2 and idx.shape[0] == self.K
        if self.guarded and apply:
            self._step_guarded(idx, self.K, idx.shape[1])
            return
        u = self._set_struct(idx, self.K, idx.shape[1], apply)
        self._native.check(self._update(self._C.byref(u), self._stream()))

    def last_losses(self):
        s = self.stats.cpu()
        return [{"pg_loss": float(r[4]), "value_loss": float(r[5]), "grad_norm": float(r[2])} for r in s]

    def diagnostics(self):
        """FusedUpdate.diagnostics(), one dict per member."""
        return self._diagnostics()


class PopulationTrainer(_Trainer):
    """K independent PPO learners trained side by side on ONE env: member k owns the envs [k EM, (k + 1) EM) of `venv`
    (EM = num_envs / K), collects with its own actor-critic and noise key, and is updated on its own rows with its own
    hyper-parameters -- one collection launch (ACAS2DVecEnv.collect_set), two launches per minibatch (FusedUpdateSet) and
    one evaluation launch (evaluate_policies_fused) for all K, where K PPOTrainer(collector="fused", updater="fused") runs
    take K times as many.  There is no exchange between members: no exploit / explore step, K separate runs
    (PBTTrainer, below, adds one).
    n_traffic in {1, 2, 3, 4, 8}; group=True: n_traffic in {8, 16, 32, 64}, with the group-cooperative launches
    (collect_set(group=True), evaluate_policies_fused(group=True)) and, at 16 / 32 / 64, the wide update.

    `configs`: K PPOConfig.  MEMBER_FIELDS may differ; n_steps, batch_size and n_epochs must be equal (the members share
    every launch).  Member k starts from the weights PPOTrainer(PPOConfig(seed=s_k)) constructs, draws its minibatch
    permutations from its own torch.Generator and its collection noise with the key s_k.  `num_timesteps` counts ONE
    member's env steps (n_steps x EM per iteration), so learn()'s arguments mean per member what PPOTrainer.learn()'s do.
    With per-member gamma / gae_lambda GAE takes them as per-env float32 vectors (the product gamma x lambda is then
    rounded in float32); equal values are passed as the numbers they are.
    Out of scope: float64, members with different n_steps / batch_size / n_epochs, more than one GPU.
    gae: None / "torch" (compute_gae, op by op) or "kernel" (gae_fused: one launch for all members, the same bits).
    target_kl may differ between members (None: no limit): a member whose minibatch exceeds 1.5 x its target_kl sits out
    the rest of that update() while the others go on in the same launches, decided on the device (FusedUpdateSet's
    guarded entry).  With a target_kl anywhere, or diagnostics=True, update() adds approx_kl, clip_fraction, n_applied,
    early_stop and explained_variance per member; without both it issues the launches it always did.
    clip_range_vf and the three schedules may differ between members too (None: off): with one anywhere the update goes
    through FusedUpdateSet's `options` entry, a member without them getting neutral numbers in the same launches, and
    update() adds every member's effective learning_rate, clip_range and (where set) clip_range_vf.
    reward_norm: None, True or a RewardNormalizer of K members, as PPOTrainer's: member k's rewards are normalised by its
    OWN running statistics (with its own gamma) in the one call after the collection, update() adds reward_std per member
    and learn() saves member k's normaliser state under member_<k>/ beside its zips.
    disturbances: None, one policy.Disturbance for all members or K of them with equal seeds (a population can sweep noise
    levels), as PPOTrainer's `disturbance`: member k collects under its own four standard deviations
    (ACAS2DVecEnv.collect_set(disturbances=)), b_obs holds the rows its networks read, and the bootstrap value is its
    critic's on the disturbed row -- policy_set.values() of it, or with gae="kernel" at n_traffic 1, 2, 3, 4, 8 the
    kernel's own.  Saved under member_<k>/ beside the zips and part of state_dict().  A policy.CorrelatedDisturbanceSet
    of K members in their place: member k under its own correlations too (rho keys in the saved numbers), the error state of
    all envs held by the set between launches -- it belongs to the envs, so a PBT exploit step copies none of it."""

    def __init__(self, venv, configs, gae=None, group=False, diagnostics=False, reward_norm=None, disturbances=None):
        configs = list(configs)
        if reward_norm is not None and reward_norm is not True and not isinstance(reward_norm, RewardNormalizer):
            raise TypeError("reward_norm must be None, True or a RewardNormalizer, got %r" % (reward_norm,))
        self.group = bool(group)
        self.diagnostics = bool(diagnostics)
        self.gae = gae or "torch"
        if self.gae not in ("torch", "kernel"):
            raise ValueError("gae must be None, 'torch' or 'kernel', got %r" % (gae,))
        if not configs:
            raise ValueError("PopulationTrainer needs at least one PPOConfig")
        for f in SHARED_FIELDS:
            if len({getattr(c, f) for c in configs}) != 1:
                raise ValueError("every member of a population needs the same %s (the members share every launch), got %s"
                                 % (f, [getattr(c, f) for c in configs]))
        if getattr(venv, "dtype", torch.float32) != torch.float32:
            raise ValueError("PopulationTrainer is float32 only (float64 trains one learner per process: PPOTrainer), this "
                             "env is %s" % (venv.dtype,))
        if self.group:
            if venv.n_traffic not in (8, 16, 32, 64) or venv.obs_dim not in FUSED_UPDATE_WIDTHS + FUSED_UPDATE_WIDE_WIDTHS:
                raise ValueError("PopulationTrainer(group=True) needs n_traffic in {8, 16, 32, 64}, got %d (n_traffic in "
                                 "{1, 2, 3, 4}: group=False)" % venv.n_traffic)
        elif venv.n_traffic not in (1, 2, 3, 4, 8) or venv.obs_dim not in FUSED_UPDATE_WIDTHS:
            raise ValueError("PopulationTrainer needs n_traffic in {1, 2, 3, 4, 8}, got %d (the group-cooperative launches "
                             "and the wide update of n_traffic 16 / 32 / 64: pass group=True)" % venv.n_traffic)
        K = len(configs)
        if venv.num_envs % K or (venv.num_envs // K) % 64:
            raise ValueError("PopulationTrainer needs num_envs = K x a multiple of 64, got num_envs = %d for K = %d members"
                             % (venv.num_envs, K))
        self.venv, self.configs, self.K, self.EM = venv, configs, K, venv.num_envs // K
        self.cfg = configs[0]                           # the shared fields
        self.device = venv.device
        members = []
        for c in configs:                               # PPOTrainer.__init__'s construction, member by member
            torch.manual_seed(c.seed)
            members.append(ActorCritic(venv.obs_dim))
        self.policy_set = ActorCriticSet.from_members(members, device=self.device)
        self.generators = []
        for c in configs:
            gen = torch.Generator(device=self.device)
            gen.manual_seed(c.seed)
            self.generators.append(gen)
        self.noise_seeds = torch.as_tensor(np.asarray([c.seed & (2 ** 64 - 1) for c in configs], np.uint64).view(np.int64)
                                           ).to(self.device)
        per_env = lambda f: (getattr(configs[0], f) if len({getattr(c, f) for c in configs}) == 1 else  # noqa: E731
                             torch.tensor([getattr(c, f) for c in configs], dtype=torch.float32, device=self.device
                                          ).repeat_interleave(self.EM))
        self.gamma, self.gae_lambda = per_env("gamma"), per_env("gae_lambda")
        # gae="kernel": the same two hyper-parameters per MEMBER, rounded as compute_gae rounds the per-env forms above
        per_member = lambda f: (getattr(configs[0], f) if len({getattr(c, f) for c in configs}) == 1 else  # noqa: E731
                                torch.tensor([getattr(c, f) for c in configs], dtype=torch.float32, device=self.device))
        self._gae_constants = gae_constants(per_member("gamma"), per_member("gae_lambda"), K, self.device)
        self._set_disturbances(disturbances, K, type(self).__name__)
        self.obs = venv.reset().to(torch.float32).clone()
        self.obs_boot = self.obs if self.disturbances is None else self.obs.clone()
        self.reward_norm = (None if reward_norm is None else
                            _reward_normalizer_for(reward_norm, venv.num_envs, configs, self.device))
        self.nan_events = torch.zeros(K, dtype=torch.int64, device=self.device)
        self.num_timesteps = 0
        self.ep_returns, self.ep_lengths, self.ep_outcomes = ([[] for _ in range(K)] for _ in range(3))
        self.history = []
        self.total_timesteps = None
        self._fused_out = self._fused_update = None
        E, T, dev = venv.num_envs, self.cfg.n_steps, self.device
        self._alloc_rollout()
        self.last_value = torch.zeros(E, dtype=torch.float32, device=dev)
        # member k's rows of the flat [T * E] buffer, in the order its own [T * EM] buffer would have them
        t_ = torch.arange(T, device=dev).unsqueeze(1) * E + torch.arange(self.EM, device=dev).unsqueeze(0)
        self.member_rows = (torch.arange(K, device=dev).view(K, 1, 1) * self.EM + t_.unsqueeze(0)).reshape(K, T * self.EM)
        self.mb_idx, self.mb_tail = minibatch_buffers(T * self.EM, self.cfg.batch_size, dev, lead=(K,))

    def member(self, k):
        """Member k's current actor-critic (a copy)."""
        return self.policy_set.member(k)

    def collect(self):
        T, E, K, EM = self.cfg.n_steps, self.venv.num_envs, self.K, self.EM
        out = self.venv.collect_set(self.policy_set, T, self.noise_seeds, noise_step=self.num_timesteps // EM,
                                    out=self._fused_out, **({"group": True} if self.group else {}),
                                    **({} if self.disturbances is None else {"disturbances": self.disturbances}))
        self._fused_out = out
        self.nan_events.add_(self._store_collection(out).view(T, K, EM).sum((0, 2)))
        if self.reward_norm is not None:
            self.reward_norm.normalize(self.b_rew, self.b_done, out=self.b_rew)
        # the kernel's own critics on the rows the next collection's first step reads (the bits of its values[0]), where
        # a disturbed run asks for gae="kernel" and the kernel has them; else the bootstrap value is torch's
        own_critics = self.gae == "kernel" and self.disturbances is not None and self.venv.obs_dim in GAE_BOOTSTRAP_WIDTHS
        if own_critics:
            gae_fused(self.b_rew, self.b_val, self.b_done, None, n_members=K, critic=self.policy_set, obs_last=self.obs_boot,
                      constants=self._gae_constants, out={"adv": self.b_adv, "ret": self.b_ret, "last_value": self.last_value})
        else:
            self.last_value.copy_(self.policy_set.values(self.obs_boot))
            if self.gae == "kernel":
                gae_fused(self.b_rew, self.b_val, self.b_done, self.last_value, n_members=K, constants=self._gae_constants,
                          out={"adv": self.b_adv, "ret": self.b_ret})
            else:
                adv, ret = compute_gae(self.b_rew, self.b_val, self.b_done, self.last_value, self.gamma, self.gae_lambda)
                self.b_adv.copy_(adv)
                self.b_ret.copy_(ret)
        done = self.b_done
        if bool(done.any()):                              # the iteration's one host synchronisation
            member_of = (torch.arange(E, device=self.device) // EM).expand(T, E)[done].cpu()
            r, l, o = self.b_epret[done].cpu(), (self.b_eplen[done] - 1).cpu(), self.b_outcome[done].cpu()
            for k in range(K):
                sel = member_of == k
                if bool(sel.any()):
                    self.ep_returns[k].append(r[sel])
                    self.ep_lengths[k].append(l[sel])
                    self.ep_outcomes[k].append(o[sel])
        self.num_timesteps += T * EM

    def _make_fused_update(self):
        return FusedUpdateSet(self.policy_set, self.configs, self.b_obs, self.b_act, self.b_logp, self.b_adv, self.b_ret,
                              diagnostics=self.diagnostics, old_val=self.b_val)

    def update(self):
        cfg, K = self.cfg, self.K
        n = cfg.n_steps * self.EM
        if self._fused_update is None:
            self._fused_update = self._make_fused_update()
        fu = self._fused_update
        fu.begin_update(self._progress_remaining())
        hyper_before = self._hyper_rows(fu) if fu.options else None
        for _ in range(cfg.n_epochs):
            perm = torch.stack([torch.randperm(n, device=self.device, generator=g) for g in self.generators])
            rows = self.member_rows.gather(1, perm)       # [K, n]: each member's permutation, as rows of the shared buffer
            for idx in minibatch_schedule(rows, self.mb_idx, self.mb_tail):
                fu.step(idx)
        std = self.policy_set.params["log_std"].detach().exp().reshape(K).cpu().tolist()
        out = [{"pg_loss": st["pg_loss"], "value_loss": st["value_loss"], "std": std[k]}
               for k, st in enumerate(fu.last_losses())]
        if fu.guarded:
            rows = lambda b: b.view(cfg.n_steps, K, self.EM).transpose(0, 1).reshape(K, -1)  # noqa: E731
            ev = explained_variance(rows(self.b_val), rows(self.b_ret)).cpu().tolist()
            for k, d in enumerate(fu.diagnostics()):
                out[k].update({n: d[n] for n in ("approx_kl", "clip_fraction", "n_applied", "early_stop")})
                out[k]["explained_variance"] = ev[k]
        if fu.options:
            for k, eff in enumerate(fu.effective(hyper_before)):
                out[k].update(eff)
        if self.reward_norm is not None:
            for k, sd in enumerate(self.reward_norm.reward_std().cpu().tolist()):
                out[k]["reward_std"] = sd
        return out

    def _hyper_rows(self, fu):
        """The hyper rows this update runs with, for the log's learning_rate / clip_range: None, the configs' own --
        nothing in a PopulationTrainer rewrites the rows.  PBTTrainer answers with the rows its last exploit() read back;
        a caller who writes into the device `hyper` tensor by hand changes what the kernels use, not what is logged."""
        return None

    def optimizer_state(self):
        """The members' Adam state: step [K], exp_avg / exp_avg_sq [K, n] in the flat layout of include/acas2d.h."""
        fu = self._fused_update
        if fu is None:
            return {"updater": "fused", "step": [0] * self.K, "exp_avg": None, "exp_avg_sq": None}
        return {"updater": "fused", "step": fu.step_count.cpu().tolist(), "exp_avg": fu.m, "exp_avg_sq": fu.v}

    def recent_episodes(self, clear=True):
        """One PPOTrainer.recent_episodes() dict per member (None where no episode ended)."""
        out = [episode_summary(self.ep_returns[k], self.ep_lengths[k], self.ep_outcomes[k]) for k in range(self.K)]
        if clear:
            self.ep_returns, self.ep_lengths, self.ep_outcomes = ([[] for _ in range(self.K)] for _ in range(3))
        return out

    def evaluate(self, n_episodes, rng, disturbance=None):
        """Score the K current actors deterministically on the SAME `n_episodes` fresh episodes drawn from `rng` in ONE
        launch (policy.evaluate_policies_fused): its dict, rows = members.  disturbance: one policy.Disturbance for all
        rows, handed to evaluate_policies_fused (None: the nominal score)."""
        return self._evaluate_rows(self.policy_set.actor_weights(), self.group, n_episodes, rng, disturbance)

    def learn(self, total_timesteps, log=print, eval_every=None, eval_episodes=10, eval_seed=None, save_dir=None,
              checkpoint_every=None):
        """PPOTrainer.learn() for every member at once; every count of timesteps is ONE member's.  Records carry a
        "member" key; `history` (returned, and kept as self.history) holds one record per member and iteration, plus one
        per member and evaluation.  Evaluations score all members on the same episodes (one random.Random(eval_seed),
        default the first member's seed, kept for the run).  Files go under save_dir/member_<k>/ as PPOTrainer writes them
        under save_dir: results/evaluations.npz, best_model.zip (per member: its own best), checkpoints/."""
        if checkpoint_every and not save_dir:
            raise ValueError("checkpoint_every needs save_dir")
        eval_rng = random.Random(self.configs[0].seed if eval_seed is None else eval_seed) if eval_every else None
        rn = self.reward_norm
        books = [_Callbacks(save_dir and os.path.join(save_dir, "member_%d" % k), lambda k=k: self.member(k), {"member": k},
                            reward_norm=rn and (lambda k=k: rn.state_dict(member=k)),
                            disturbance=self.disturbances and self.disturbances.members[k].to_dict())
                 for k in range(self.K)]

        def iterate():
            self.collect()
            stats = self.update()
            return stats, self.recent_episodes(), self.nan_events.cpu().tolist()

        return self._learn(total_timesteps, log, books, self.history, iterate,
                           lambda: self.evaluate(eval_episodes, eval_rng), eval_every, checkpoint_every)


# ---- population-based training: score, exploit and explore on the device (csrc/acas2d_pbt.hip) -------------------------
def member_episodes(done, outcome, episode_return, episode_steps, n_members, acc=None):
    """The episodes that ended in a collection, summed per member in ONE launch (acas2d_member_episodes_f32).  `done`
    (bool or uint8), `outcome` (uint8), `episode_return` (float32) and `episode_steps` (int32) are the collector's [T, E]
    outputs as they lie, member k owning the columns [k EM, (k + 1) EM); what lies where `done` is 0 reaches nothing.
    ADDS to `acc` -- {"count": int64 [K], "outcomes": int64 [K, 4], "steps": int64 [K] (step() calls), "return_sum":
    float64 [K]} -- and overwrites acc["score"], float32 [K]: the mean return of everything added so far, NaN where no
    episode has ended.  acc=None starts a zeroed window.  Returns acc.  No host synchronisation; the same inputs give the
    same bits."""
    import ctypes as C
    from . import native
    K = int(n_members)
    dev = done.device
    if done.dtype == torch.bool:
        done = done.view(torch.uint8)
    want = ((done, torch.uint8), (outcome, torch.uint8), (episode_return, torch.float32), (episode_steps, torch.int32))
    if done.dim() != 2 or any(t.shape != done.shape or t.dtype != dt or not t.is_contiguous() or t.device != dev
                              for t, dt in want):
        raise ValueError("member_episodes takes contiguous [T, E] tensors on one device: done bool / uint8, outcome uint8, "
                         "episode_return float32, episode_steps int32")
    if acc is None:
        z = lambda *shape, dt=torch.int64: torch.zeros(*shape, dtype=dt, device=dev)  # noqa: E731
        acc = {"count": z(K), "outcomes": z(K, 4), "steps": z(K), "return_sum": z(K, dt=torch.float64),
               "score": torch.full((K,), float("nan"), dtype=torch.float32, device=dev)}
    shapes = {"count": (K,), "outcomes": (K, 4), "steps": (K,), "return_sum": (K,), "score": (K,)}
    if any(tuple(acc[n].shape) != s or not acc[n].is_contiguous() or acc[n].device != dev for n, s in shapes.items()):
        raise ValueError("member_episodes: acc does not hold the accumulators of %d members on %s" % (K, dev))
    p = lambda t: t.data_ptr()  # noqa: E731
    T, E = done.shape
    m = native.CMemberEpisodes(p(done), p(outcome), p(episode_return), p(episode_steps), p(acc["count"]), p(acc["outcomes"]),
                               p(acc["steps"]), p(acc["return_sum"]), p(acc["score"]), E, T, K)
    native.check(native.lib().acas2d_member_episodes_f32(C.byref(m), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return acc


PBT_PERTURB = ("learning_rate", "clip_range", "ent_coef")
PBT_BOUNDS = {"learning_rate": (1e-6, 1e-2), "clip_range": (0.02, 0.5), "ent_coef": (0.0, 0.1)}


def _hyper_slots(names):
    unknown = [n for n in names if n not in HYPER_SLOTS]
    if unknown:
        raise ValueError("%s: not a slot of the hyper row %s" % (unknown, HYPER_SLOTS))
    return [HYPER_SLOTS.index(n) for n in names]


def population_exploit(policy_set, fused_update_set, score, n_replace, generation, seed, perturb=PBT_PERTURB,
                       factors=(0.8, 1.2), bounds=PBT_BOUNDS):
    """The exploit / explore step of population-based training in ONE launch (acas2d_population_exploit_f32): each of the
    `n_replace` members with the worst `score` (float32 device tensor [K]; NaN is worst, ties go to the smaller index)
    draws one of the `n_replace` best and, where that one is strictly better, becomes a bit copy of it -- the 13
    parameter stacks of `policy_set`, the Adam moments and step of `fused_update_set` -- with its `hyper` row, the slots
    named in `perturb` multiplied by one of `factors` (one random bit per slot) and clamped into `bounds[name]`.
    (generation, seed) key the draws.  Returns `donor`, int32 device tensor [K]: whom member k was copied from, k where
    nothing changed.  No host decision and no synchronisation."""
    import ctypes as C
    from . import native
    fu, K = fused_update_set, policy_set.n_members
    if fu.policy_set is not policy_set:
        raise ValueError("population_exploit: fused_update_set updates another ActorCriticSet")
    if score.dtype != torch.float32 or tuple(score.shape) != (K,) or not score.is_contiguous() or score.device != fu.device:
        raise ValueError("population_exploit: score must be a contiguous float32 tensor [%d] on %s" % (K, fu.device))
    mask, lo, hi = 0, [-math.inf] * 8, [math.inf] * 8
    for name, s in zip(perturb, _hyper_slots(perturb)):
        if name not in bounds:
            raise ValueError("population_exploit: no bounds for the perturbed %r" % name)
        mask |= 1 << s
        lo[s], hi[s] = (float(b) for b in bounds[name])
    donor = torch.empty(K, dtype=torch.int32, device=fu.device)
    p = lambda t: t.data_ptr()  # noqa: E731
    x = native.CPopulationExploit(*[p(policy_set.params[n]) for n in PARAM_NAMES], p(fu.m), p(fu.v), p(fu.step_count),
                                  p(fu.hyper), p(score), p(donor), K, policy_set.obs_dim, int(n_replace),
                                  int(generation) & 0xffffffff, int(seed) & (2 ** 64 - 1), mask, float(factors[0]),
                                  float(factors[1]), (C.c_float * 8)(*lo), (C.c_float * 8)(*hi), 0)
    native.check(native.lib().acas2d_population_exploit_f32(
        C.byref(x), C.c_void_p(torch.cuda.current_stream(fu.device).cuda_stream)))
    return donor


@dataclasses.dataclass
class PBTConfig:
    """When and how a PBTTrainer exchanges between its members (Jaderberg et al. 2017, truncation selection): every
    `ready_every` iterations the floor(fraction x K) members with the worst mean return of the window each copy one of
    the equally many best and perturb the copied `perturb` hyper-parameters by one of `factors` (the paper's 0.8 / 1.2),
    clamped into `bounds`."""
    ready_every: int
    fraction: float = 0.25
    factors: tuple = (0.8, 1.2)
    perturb: tuple = PBT_PERTURB
    bounds: dict = dataclasses.field(default_factory=lambda: dict(PBT_BOUNDS))
    seed: int = 0

    def __post_init__(self):
        if int(self.ready_every) != self.ready_every or self.ready_every < 1:
            raise ValueError("PBTConfig.ready_every counts iterations: an integer >= 1, got %r" % (self.ready_every,))
        if not 0.0 <= self.fraction <= 1.0:
            raise ValueError("PBTConfig.fraction is a share of the population, in [0, 1], got %r" % (self.fraction,))
        if len(self.factors) != 2 or not all(math.isfinite(f) and f > 0 for f in self.factors):
            raise ValueError("PBTConfig.factors must be two finite positive numbers, got %r" % (self.factors,))
        for name, s in zip(self.perturb, _hyper_slots(self.perturb)):
            if name not in self.bounds or not self.bounds[name][0] <= self.bounds[name][1]:
                raise ValueError("PBTConfig.bounds needs lo <= hi for the perturbed %r" % name)

    def n_replace(self, n_members):
        """floor(fraction x K); a ValueError where 2 x n_replace > K."""
        R = int(math.floor(self.fraction * n_members))
        if 2 * R > n_members:
            raise ValueError("PBTConfig: 2 x n_replace <= K is the rule (donors and recipients are disjoint); fraction = %r "
                             "gives n_replace = %d of K = %d" % (self.fraction, R, n_members))
        return R


class PBTTrainer(PopulationTrainer):
    """PopulationTrainer with the exchange between members that makes a population more than a seed sweep
    (population-based training, Jaderberg et al. 2017), scored and decided on the device:
      collect()   the parent's, followed by ONE member_episodes launch on the b_* buffers: `window` accumulates every
                  member's ended episodes, window["score"] is its mean return;
      update()    the parent's; every `pbt.ready_every`-th call is followed by exploit();
      exploit()   ONE population_exploit launch with the window's score, generation = the number of exploits so far and
                  pbt.seed; zeroes the window and appends one record per member to `history`:
                  {"member", "exploit": donor or None, "hyper": the member's row (HYPER_SLOTS), "score", "timesteps",
                  "generation"}.  The read-back of donor and hyper (K x 9 numbers) follows update()'s own read of the
                  losses.
    learn() is the parent's.  A recipient takes parameters, Adam state and hyper row; it keeps its envs, its noise key and
    its minibatch generator, so twins diverge.  gamma and gae_lambda live outside the hyper row and are not exchanged:
    they must be equal across members.  A member's target_kl is not in the hyper row either and belongs to its SLOT:
    an exploit step neither copies nor perturbs it, so a recipient keeps its own limit under the donor's weights and
    learning rate -- the guard against what the x 1.2 steps can build up.  clip_range_vf and the schedules belong to the
    slot likewise; a schedule's factor multiplies the hyper row as the exploit steps have left it, and update()'s
    learning_rate / clip_range are formed from the rows read back at the last exploit (no extra read-back: rows edited
    by hand through `hyper` in between reach the kernels but not that log).  fraction = 0 is PopulationTrainer bit for bit.
    group=True, gae="kernel", diagnostics=True and reward_norm as the parent's.  With reward_norm a recipient also takes the
    donor's running reward statistics (RewardNormalizer.inherit on the kernel's device `donor` vector, no host read): its
    critic is now the donor's and lives in the donor's reward scale; the envs' discounted returns stay its own.  The score
    of the exchange is the RAW mean episode return.  disturbances as the parent's: they describe a member's ENVIRONMENT, not
    the learner, so an exploit step leaves every member's standard deviations where they were -- a recipient goes on in
    its own noise under the donor's weights."""

    def __init__(self, venv, configs, pbt, gae=None, group=False, diagnostics=False, reward_norm=None, disturbances=None):
        configs = list(configs)
        for f in ("gamma", "gae_lambda"):
            if len({getattr(c, f) for c in configs}) > 1:
                raise ValueError("PBTTrainer needs the same %s for every member: it lives outside the hyper row and is not "
                                 "exchanged by an exploit step, got %s" % (f, [getattr(c, f) for c in configs]))
        self.pbt = pbt
        self.n_replace = pbt.n_replace(len(configs))
        super().__init__(venv, configs, gae=gae, group=group, diagnostics=diagnostics, reward_norm=reward_norm,
                         disturbances=disturbances)
        # built now, not at the first update: an exploit before it must find the moments and the hyper row
        self._fused_update = self._make_fused_update()
        self.window = None
        self.generation = 0
        self._updates = 0
        self._hyper_host = None                           # the rows as the last exploit's read-back found them

    @property
    def hyper(self):
        """The members' current hyper rows: float32 device tensor [K, 8] (HYPER_SLOTS)."""
        return self._fused_update.hyper

    def _hyper_rows(self, fu):
        return self._hyper_host

    def collect(self):
        super().collect()
        self.window = member_episodes(self.b_done, self.b_outcome, self.b_epret, self.b_eplen, self.K, acc=self.window)

    def update(self):
        stats = super().update()
        self._updates += 1
        if self._updates % self.pbt.ready_every == 0:
            self.exploit()
        return stats

    def exploit(self):
        """One exploit / explore step on the window's score; returns the members' records (also appended to history)."""
        if self.window is None:
            raise RuntimeError("PBTTrainer.exploit() needs a collect() first: there is no score yet")
        pbt, w = self.pbt, self.window
        donor = population_exploit(self.policy_set, self._fused_update, w["score"], self.n_replace, self.generation,
                                   pbt.seed, perturb=pbt.perturb, factors=pbt.factors, bounds=pbt.bounds)
        if self.reward_norm is not None:
            self.reward_norm.inherit(donor)
        donor, hyper, score = donor.cpu().tolist(), self.hyper.cpu().tolist(), w["score"].cpu().tolist()
        self._hyper_host = hyper
        for n in ("count", "outcomes", "steps", "return_sum"):
            w[n].zero_()
        w["score"].fill_(float("nan"))
        recs = [{"member": k, "exploit": None if donor[k] == k else donor[k], "hyper": hyper[k], "score": score[k],
                 "timesteps": self.num_timesteps, "generation": self.generation} for k in range(self.K)]
        self.history.extend(recs)
        self.generation += 1
        return recs
