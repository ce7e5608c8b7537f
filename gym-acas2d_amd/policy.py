"""Stable-Baselines3 `MlpPolicy` actor as a plain torch module + a `testing_main.py`-style
evaluation loop.

The reference ships trained PPO policies as SB3 1.1.0 zips
(gym_ACAS2D/models/best_model_1048576_11/best_model.zip, models/checkpoints_*/model_*_steps.zip)
and evaluates them with `model.predict(state, deterministic=True)` (testing_main.py:74).  SB3 is
not required here: the zip's `policy.pth` is a state dict of 13 float32 tensors, read with
`torch.load(weights_only=True)` (nothing in the file is executed).

`predict(obs, deterministic=True)` follows SB3 1.1.0's `BasePolicy.predict` for a Box action
space without squashing: observation -> float32, two tanh layers of 64, linear action head, the
mean action clipped to [-1, 1].
"""
import ctypes as C
import dataclasses
import io
import math
import os
import weakref
import zipfile

import numpy as np
import torch

from . import native, records
from .config import ACAS2DConfig

_ACTOR_KEYS = ("mlp_extractor.policy_net.0.weight", "mlp_extractor.policy_net.0.bias",
               "mlp_extractor.policy_net.2.weight", "mlp_extractor.policy_net.2.bias",
               "action_net.weight", "action_net.bias")


def kernel_layout(w1, b1, w2, b2, w3, b3, device=None):
    """One SB3 MlpPolicy net (actor or critic) as the kernels read it (CPolicy / Acas2dActorCritic, include/acas2d.h):
    from (w1 [64, D], b1, w2 [64, 64], b2, w3 [1, 64], b3) in torch's layout, each with an optional leading [K], six
    contiguous float32 tensors -- w1 and w2 transposed on their last two dimensions ([D][64], [64][64]), the head and
    the biases flat per member.  Checks no shape: every caller has its own message."""
    w = [torch.as_tensor(t).detach().to(device=device, dtype=torch.float32) for t in (w1, b1, w2, b2, w3, b3)]
    flat = (lambda t: t.reshape(t.shape[0], -1)) if w[0].dim() == 3 else (lambda t: t.reshape(-1))  # noqa: E731
    return [(t.transpose(-2, -1) if i in (0, 2) else flat(t)).contiguous() for i, t in enumerate(w)]


class SB3ActorPolicy(torch.nn.Module):
    def __init__(self, state_dict):
        super().__init__()
        w1, b1, w2, b2, wa, ba = (torch.as_tensor(np.asarray(state_dict[k]), dtype=torch.float32)
                                  for k in _ACTOR_KEYS)
        self.l1 = torch.nn.Linear(w1.shape[1], w1.shape[0])
        self.l2 = torch.nn.Linear(w2.shape[1], w2.shape[0])
        self.head = torch.nn.Linear(wa.shape[1], wa.shape[0])
        with torch.no_grad():
            for lin, w, b in ((self.l1, w1, b1), (self.l2, w2, b2), (self.head, wa, ba)):
                lin.weight.copy_(w)
                lin.bias.copy_(b)
        self.obs_dim = w1.shape[1]

    @torch.no_grad()
    def forward(self, obs):
        x = obs.to(torch.float32)
        return self.head(torch.tanh(self.l2(torch.tanh(self.l1(x)))))

    def actor_weights(self):
        """(w1 [64,D], b1, w2 [64,64], b2, w3 [1,64], b3) for ACAS2DVecEnv.rollout_policy()."""
        return tuple(t.detach() for t in (self.l1.weight, self.l1.bias, self.l2.weight, self.l2.bias,
                                          self.head.weight, self.head.bias))

    @torch.no_grad()
    def predict(self, obs, deterministic=True):
        """[E, obs_dim] -> [E, 1] float32 actions in [-1, 1] (deterministic = the mean action)."""
        if not deterministic:
            raise NotImplementedError("only the deterministic evaluation path of testing_main.py:74")
        return self.forward(obs).clamp_(-1.0, 1.0)


def load_sb3_policy(path, device="cpu"):
    """Load the actor of an SB3 PPO zip (or of an .npz export of its policy.pth)."""
    if str(path).endswith(".npz"):
        sd = dict(np.load(path, allow_pickle=False))
    else:
        with zipfile.ZipFile(path) as z:
            sd = torch.load(io.BytesIO(z.read("policy.pth")), map_location="cpu", weights_only=True)
    return SB3ActorPolicy(sd).to(device)


SB3_VERSION = "1.1.0"


def save_sb3_policy(actor_critic, path):
    """Write `actor_critic` (a `ppo.ActorCritic`) as the policy half of an SB3 1.1.0 PPO zip: `policy.pth`, the
    state dict of its 13 float32 tensors under SB3's MlpPolicy keys (ActorCritic's own parameter names), and
    `_stable_baselines3_version`.  `load_sb3_policy` / `ActorCritic.load_sb3_state_dict` read it back bit for bit.
    SB3's pickled `data` member (the class, spaces and hyper-parameters) is NOT written, so loading the file with
    SB3 itself is parity unpinned."""
    sd = {k: v.detach().to(device="cpu", dtype=torch.float32).contiguous().clone()
          for k, v in actor_critic.state_dict().items()}
    buf = io.BytesIO()
    torch.save(sd, buf)
    path = str(path)
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    tmp = path + ".tmp"
    with zipfile.ZipFile(tmp, "w", zipfile.ZIP_DEFLATED) as z:
        z.writestr("policy.pth", buf.getvalue())
        z.writestr("_stable_baselines3_version", SB3_VERSION)
    os.replace(tmp, path)
    return path


def evaluate_policy(venv, policy, max_steps=None):
    """testing_main.simulate() (testing_main.py:62-105) on a batch: every env of `venv` (which must
    NOT auto-reset and must already hold its episode, e.g. via set_state) is stepped with the
    deterministic policy until done.  Returns numpy arrays outcome, steps (game.steps at done),
    total_reward, path_length (2 px per step() call at the default airspeed; game.d_path)."""
    assert not venv.auto_reset, "evaluate_policy wants auto_reset=False (one episode per env)"
    E = venv.num_envs
    max_steps = max_steps or venv.config.max_steps
    obs = venv.outputs["obs"]
    outcome = torch.zeros(E, dtype=torch.uint8, device=venv.device)
    steps = torch.zeros(E, dtype=torch.int32, device=venv.device)
    ret = torch.zeros(E, dtype=venv.dtype, device=venv.device)
    active = torch.ones(E, dtype=torch.bool, device=venv.device)
    for _ in range(max_steps):
        obs, _, done, infos = venv.step(policy.predict(obs))
        fin = active & done
        outcome = torch.where(fin, infos.outcome, outcome)
        steps = torch.where(fin, venv.steps, steps)
        ret = torch.where(fin, venv.total_reward, ret)
        active &= ~done
        if not bool(active.any()):
            break
    steps_np = steps.cpu().numpy()
    step_len = venv.config.airspeed * venv.config.dt
    return {"outcome": outcome.cpu().numpy(), "steps": steps_np,
            "total_reward": ret.cpu().numpy().astype(np.float64),
            "path_length": step_len * (steps_np - 1), "unfinished": int(active.sum().item())}


def evaluate_policy_fused(policy, own, traffic, goal=None, dtype=torch.float64, device="cuda:0", config=None,
                          max_steps=None, group=False):
    """evaluate_policy() as ONE kernel launch (ACAS2DVecEnv.rollout_policy): the episodes given by
    `own` [E,4] / `traffic` [E,N,4] / `goal` are run with the deterministic SB3 actor evaluated inside
    the rollout kernel; results are those of each env's FIRST episode (the launch has VecEnv
    auto-reset semantics and keeps stepping the envs that finish early).  Thread-per-env shapes only
    (N in {1,2,3,4,8} float32, {1,2,3,4} float64), or with group=True the group-cooperative float32 launch
    (N in {8,16,32,64}, ACAS2DVecEnv.rollout_policy(group=True)).  A NaN observation (the reference's d_cpa in
    exact parallel flight) gives a NaN action, as policy.predict() does in evaluate_policy()."""
    from .vec_env import ACAS2DVecEnv
    if group and dtype != torch.float32:
        raise ValueError("evaluate_policy_fused(group=True) is float32 only, got %s" % (dtype,))
    own, traffic = np.asarray(own), np.asarray(traffic)
    E, N = own.shape[0], traffic.shape[1]
    v = ACAS2DVecEnv(E, N, device=device, dtype=dtype, auto_reset=True, config=config)
    v.set_state(own, traffic, goal, np.zeros(E, np.int32), observe=True)
    T = (max_steps or v.config.max_steps) + 1
    out = v.rollout_policy(policy, T, group=group)
    done = out["done"].cpu().numpy()
    fin = done.any(0)
    t0, e = done.argmax(0), np.arange(E)
    steps = np.where(fin, out["episode_steps"].cpu().numpy()[t0, e], 0)
    step_len = v.config.airspeed * v.config.dt
    return {"outcome": np.where(fin, out["outcome"].cpu().numpy()[t0, e], 0).astype(np.uint8), "steps": steps,
            "total_reward": np.where(fin, out["episode_return"].cpu().numpy()[t0, e], 0.0).astype(np.float64),
            "path_length": step_len * (steps - 1), "unfinished": int((~fin).sum())}


def stack_policies(policies, obs_dim, device):
    """K policies -- `SB3ActorPolicy` / `ppo.ActorCritic` objects, paths of SB3 zips / .npz exports, or six-tensor tuples --
    as the six stacked float32 tensors the K-policy launches read: [K][D][64], [K][64], [K][64][64], [K][64], [K][64], [K][1]."""
    ws = []
    for pol in policies:
        if isinstance(pol, (str, os.PathLike)):
            pol = load_sb3_policy(pol)
        w = pol.actor_weights() if hasattr(pol, "actor_weights") else pol
        w1, b1, w2, b2, w3, b3 = (torch.as_tensor(t, dtype=torch.float32).to(device) for t in w)
        if w1.shape != (64, obs_dim) or w2.shape != (64, 64) or w3.numel() != 64 or b3.numel() != 1:
            raise ValueError("policy must be the SB3 MlpPolicy actor %d -> 64 -> 64 -> 1, got %s %s %s"
                             % (obs_dim, tuple(w1.shape), tuple(w2.shape), tuple(w3.shape)))
        ws.append(kernel_layout(w1, b1, w2, b2, w3, b3))
    return [torch.stack(ts) for ts in zip(*ws)]                                  # [K][D][64], [K][64], ...


@dataclasses.dataclass(frozen=True, init=False)
class Disturbance:
    """White Gaussian sensor noise and actuator disturbance for the float32 evaluator and Monte Carlo campaign
    (acas2d_evaluate_policies_disturbed_*, acas2d_monte_carlo_disturbed_*; records.disturb_observation() /
    disturb_action() state the arithmetic).  Per step each traffic aircraft's normalised separation, closest-point-of-approach
    distance and closing speed, as the actor reads them, get independent noise, and the actor's clipped action gets
    `action` x a standard normal and is clipped again.

    sep, cpa   standard deviations in pixels;  closing: in the units of v_closing.  They are divided by `config`'s d_sep_max,
               d_cpa_max and v_closing_max in float64 and rounded to float32: the fields s_sep, s_cpa, s_closing (normalised
               units) are what the kernels use and what two disturbances are compared by.
    action     standard deviation in units of the action ([-1, 1]);  seed: the noise stream's 64-bit seed.
    Disturbance.normalised(sep=, cpa=, closing=, action=, seed=) takes the three in normalised units directly."""
    s_sep: float
    s_cpa: float
    s_closing: float
    s_action: float
    seed: int

    def __init__(self, sep=0.0, cpa=0.0, closing=0.0, action=0.0, seed=0, config=None):
        c = (config if config is not None else ACAS2DConfig()).to_c()
        self._set(float(sep) / float(c.d_sep_max), float(cpa) / float(c.d_cpa_max), float(closing) / float(c.v_closing_max),
                  action, seed)

    def _set(self, s_sep, s_cpa, s_closing, s_action, seed):
        for name, v in (("s_sep", s_sep), ("s_cpa", s_cpa), ("s_closing", s_closing), ("s_action", s_action)):
            with np.errstate(over="ignore"):
                object.__setattr__(self, name, float(np.float32(v)))         # the float32 the kernel reads
        object.__setattr__(self, "seed", int(seed) & 0xFFFFFFFFFFFFFFFF)

    @classmethod
    def normalised(cls, sep=0.0, cpa=0.0, closing=0.0, action=0.0, seed=0):
        d = object.__new__(cls)
        d._set(sep, cpa, closing, action, seed)
        return d

    @property
    def sigma(self):
        """(s_sep, s_cpa, s_closing): records.disturb_observation()'s argument."""
        return (self.s_sep, self.s_cpa, self.s_closing)

    def is_zero(self):
        return self.s_sep == 0 and self.s_cpa == 0 and self.s_closing == 0 and self.s_action == 0

    def to_dict(self):
        """Plain numbers (JSON, state_dict()); from_dict() gives an equal Disturbance back."""
        return {"s_sep": self.s_sep, "s_cpa": self.s_cpa, "s_closing": self.s_closing, "s_action": self.s_action,
                "seed": self.seed}

    @classmethod
    def from_dict(cls, d):
        return cls.normalised(d["s_sep"], d["s_cpa"], d["s_closing"], d["s_action"], d["seed"])

    @classmethod
    def parse(cls, text, normalised=False, config=None):
        """A Disturbance from the command-line syntax of tools/evaluate_checkpoints.py and tools/train_ppo.py,
        "sep=..,cpa=..,closing=..,action=..[,seed=..]": every key optional (0), in the constructor's units (pixels, the units
        of v_closing, action units) or, normalised=True, in normalised observation units.  ValueError on anything else."""
        kw = {}
        for item in str(text).split(","):
            key, _, val = (part.strip() for part in item.partition("="))
            if key not in ("sep", "cpa", "closing", "action", "seed") or not val or key in kw:
                raise ValueError("disturbance %r: %r (sep=, cpa=, closing=, action= and seed= are understood, each once)"
                                 % (text, item))
            try:
                kw[key] = int(val, 0) if key == "seed" else float(val)
            except ValueError:
                raise ValueError("disturbance %r: %r is no number" % (text, item)) from None
        return cls.normalised(**kw) if normalised else cls(config=config, **kw)

    def to_c(self, noise_episode=0):
        return native.CDisturbance(self.s_sep, self.s_cpa, self.s_closing, self.s_action, self.seed, int(noise_episode), 0)


@dataclasses.dataclass(frozen=True, init=False)
class CorrelatedDisturbance(Disturbance):
    """A Disturbance whose errors PERSIST: per channel a first-order Gauss-Markov process e_t = rho e_{t-1} + sqrt(1 - rho^2) z_t
    (e_1 = z_1 at an episode's first step) takes the place of the white normal z_t, for the float32 evaluator and Monte Carlo
    campaign (acas2d_evaluate_policies_correlated_*, acas2d_monte_carlo_correlated_*; records.correlated_errors() is the
    scan).  The standard deviations stay what Disturbance says: e has unit variance at every step.

    rho_sep, rho_cpa, rho_closing, rho_action   the step-to-step correlation of each channel's error, in [0, 1] (float32, as
               the kernels read them; shared by all traffic aircraft).  0: the white noise of Disturbance, bit for bit;
               1: a constant offset s z_1 per (lane, episode, channel, aircraft), a bias.
    rho        shorthand for all four (one given by name overrides it).
    A CorrelatedDisturbance never equals a Disturbance, not even with all four 0: to_dict() carries the rho keys.  The
    collectors and trainers refuse a bare one -- an episode spans their launches, and a frozen value cannot hold the error
    state between them: a CorrelatedDisturbanceSet does, and is what they take."""
    rho_sep: float
    rho_cpa: float
    rho_closing: float
    rho_action: float

    RHO = ("rho_sep", "rho_cpa", "rho_closing", "rho_action")

    def __init__(self, sep=0.0, cpa=0.0, closing=0.0, action=0.0, seed=0, config=None, rho=0.0, rho_sep=None, rho_cpa=None,
                 rho_closing=None, rho_action=None):
        Disturbance.__init__(self, sep, cpa, closing, action, seed, config)
        self._set_rho(rho, rho_sep, rho_cpa, rho_closing, rho_action)

    def _set_rho(self, rho, *each):
        for name, v in zip(self.RHO, each):
            v = float(np.float32(rho if v is None else v))                   # the float32 the kernel reads
            if not 0.0 <= v <= 1.0:                                          # (a NaN fails both comparisons)
                raise ValueError("%s = %r (every correlation coefficient must lie in [0, 1])" % (name, v))
            object.__setattr__(self, name, v)

    @classmethod
    def normalised(cls, sep=0.0, cpa=0.0, closing=0.0, action=0.0, seed=0, rho=0.0, rho_sep=None, rho_cpa=None, rho_closing=None,
                   rho_action=None):
        d = object.__new__(cls)
        d._set(sep, cpa, closing, action, seed)
        d._set_rho(rho, rho_sep, rho_cpa, rho_closing, rho_action)
        return d

    @property
    def rho(self):
        """(rho_sep, rho_cpa, rho_closing): per channel, as `sigma`."""
        return (self.rho_sep, self.rho_cpa, self.rho_closing)

    def to_dict(self):
        return {**Disturbance.to_dict(self), **{name: getattr(self, name) for name in self.RHO}}

    @classmethod
    def from_dict(cls, d):
        return cls.normalised(d["s_sep"], d["s_cpa"], d["s_closing"], d["s_action"], d["seed"],
                              **{name: d[name] for name in cls.RHO})

    @classmethod
    def parse(cls, text, normalised=False, config=None):
        """Disturbance.parse()'s syntax with rho_sep=, rho_cpa=, rho_closing=, rho_action= and rho= (all four) on top."""
        kw, rest = {}, []
        for item in str(text).split(","):
            key, _, val = (part.strip() for part in item.partition("="))
            if key != "rho" and key not in cls.RHO:
                rest.append(item)
                continue
            if not val or key in kw:
                raise ValueError("disturbance %r: %r (rho=, rho_sep=, rho_cpa=, rho_closing= and rho_action= are understood, "
                                 "each once)" % (text, item))
            try:
                kw[key] = float(val)
            except ValueError:
                raise ValueError("disturbance %r: %r is no number" % (text, item)) from None
        base = Disturbance.parse(",".join(rest), normalised, config) if rest else Disturbance()
        return cls.normalised(base.s_sep, base.s_cpa, base.s_closing, base.s_action, base.seed, **kw)

    @staticmethod
    def has_rho(text):
        """Whether a command-line disturbance names a correlation: else it is a plain Disturbance's text."""
        return any(item.partition("=")[0].strip().startswith("rho") for item in str(text).split(","))

    def to_c(self, noise_episode=0):
        """Both structs: (Acas2dDisturbance, Acas2dCorrelation)."""
        return (Disturbance.to_c(self, noise_episode),
                native.CCorrelation(self.rho_sep, self.rho_cpa, self.rho_closing, self.rho_action))


@dataclasses.dataclass(frozen=True, init=False)
class DelayedDisturbance(CorrelatedDisturbance):
    """A CorrelatedDisturbance with a RESPONSE between the policy and the aircraft, for the float32 evaluator and Monte Carlo
    campaign (acas2d_evaluate_policies_delayed_*, acas2d_monte_carlo_delayed_*; records.response_delay() and
    records.response_lag() state the two steps): first-order plus dead time.

    delay      the dead time in steps (0 .. 32767; at dt = 0.01 s a pilot's half second is 50): the aircraft flies the action the
               actor produced `delay` steps earlier in the same episode, and 0 -- straight ahead -- until the first one arrives
    lag        the pole of the first-order lag behind it, in [0, 1] (float32, as the kernels read it):
               u_s = clamp(lag u_{s-1} + (1 - lag) c_s), u = 0 in front of an episode's first step; 1: the aircraft never responds
    The actuator's error acts on u_s; the sensor errors are untouched.  With delay 0 and lag 0 the results are the
    CorrelatedDisturbance's bit for bit, but the two never compare equal: to_dict() carries the delay and lag keys.  The
    collectors, the trainers and both kinds of DisturbanceSet refuse one."""
    delay: int
    lag: float

    MAX_DELAY = 32767

    def __init__(self, sep=0.0, cpa=0.0, closing=0.0, action=0.0, seed=0, config=None, rho=0.0, rho_sep=None, rho_cpa=None,
                 rho_closing=None, rho_action=None, delay=0, lag=0.0):
        CorrelatedDisturbance.__init__(self, sep, cpa, closing, action, seed, config, rho, rho_sep, rho_cpa, rho_closing, rho_action)
        self._set_response(delay, lag)

    def _set_response(self, delay, lag):
        if isinstance(delay, bool) or not 0 <= delay <= self.MAX_DELAY or int(delay) != delay:       # (a NaN fails the range)
            raise ValueError("delay = %r (whole steps, 0 to %d)" % (delay, self.MAX_DELAY))
        lag = float(np.float32(lag))                                         # the float32 the kernel reads
        if not 0.0 <= lag <= 1.0:                                            # (a NaN fails both comparisons)
            raise ValueError("lag = %r (the lag must lie in [0, 1])" % (lag,))
        object.__setattr__(self, "delay", int(delay))
        object.__setattr__(self, "lag", lag)

    @classmethod
    def normalised(cls, sep=0.0, cpa=0.0, closing=0.0, action=0.0, seed=0, rho=0.0, rho_sep=None, rho_cpa=None, rho_closing=None,
                   rho_action=None, delay=0, lag=0.0):
        d = object.__new__(cls)
        d._set(sep, cpa, closing, action, seed)
        d._set_rho(rho, rho_sep, rho_cpa, rho_closing, rho_action)
        d._set_response(delay, lag)
        return d

    def to_dict(self):
        return {**CorrelatedDisturbance.to_dict(self), "delay": self.delay, "lag": self.lag}

    @classmethod
    def from_dict(cls, d):
        return cls.normalised(d["s_sep"], d["s_cpa"], d["s_closing"], d["s_action"], d["seed"],
                              **{name: d[name] for name in cls.RHO}, delay=d["delay"], lag=d["lag"])

    @classmethod
    def parse(cls, text, normalised=False, config=None):
        """CorrelatedDisturbance.parse()'s syntax with delay= (whole steps) and lag= on top."""
        kw, rest = {}, []
        for item in str(text).split(","):
            key, _, val = (part.strip() for part in item.partition("="))
            if key not in ("delay", "lag"):
                rest.append(item)
                continue
            if not val or key in kw:
                raise ValueError("disturbance %r: %r (delay= and lag= are understood, each once)" % (text, item))
            try:
                kw[key] = int(val, 0) if key == "delay" else float(val)
            except ValueError:
                raise ValueError("disturbance %r: %r is no number" % (text, item)) from None
        base = CorrelatedDisturbance.parse(",".join(rest), normalised, config) if rest else CorrelatedDisturbance()
        return cls.normalised(base.s_sep, base.s_cpa, base.s_closing, base.s_action, base.seed,
                              **{name: getattr(base, name) for name in cls.RHO}, **kw)

    @staticmethod
    def has_response(text):
        """Whether a command-line disturbance names a delay or a lag: else it is a (Correlated)Disturbance's text."""
        return any(item.partition("=")[0].strip() in ("delay", "lag") for item in str(text).split(","))

    def ring(self, n_envs, device):
        """The dead time's scratch for launches over `n_envs` envs (Acas2dResponse::ring): float32 [max(delay, 1), n_envs] on
        `device`, filled with NaN -- the kernels never read a slot the episode at hand has not written, and a NaN flown would
        show in every statistic."""
        return torch.full((max(self.delay, 1), int(n_envs)), float("nan"), dtype=torch.float32, device=device)

    def to_c(self, noise_episode=0, ring=None):
        """All three structs: (Acas2dDisturbance, Acas2dCorrelation, Acas2dResponse); `ring`: the tensor of ring(), which the
        caller keeps alive across the launch (None: no ring -- the library then refuses a delay above 0)."""
        return CorrelatedDisturbance.to_c(self, noise_episode) + (
            native.CResponse(self.delay, self.lag, 0 if ring is None else ring.data_ptr(), 0 if ring is None else ring.shape[1]),)


def _c_tail(disturbance, noise_episode=0, ring=None):
    """The C structs a disturbance adds behind a scoring entry's own arguments: one, (correlated) two or (delayed, with the
    caller's `ring`) three."""
    c = disturbance.to_c(noise_episode, ring) if isinstance(disturbance, DelayedDisturbance) else disturbance.to_c(noise_episode)
    return list(c) if isinstance(c, tuple) else [c]


class DisturbanceSet:
    """The disturbances K learners train under (ACAS2DVecEnv.collect(disturbance=) / collect_set(disturbances=), the
    trainers): one Disturbance for all members or K of them with EQUAL seeds -- the collector takes one noise seed per
    launch and a row of four standard deviations per member.  The rows live on the device, where the C entry cannot look
    at them, so they are checked HERE: each finite and at least 0.
      rows          float32 [K, 4]: (s_sep, s_cpa, s_closing, s_action) per member;  seed: the launch's noise seed
      members       the K Disturbances
      state_dict()  plain numbers for a trainer's state and the file saved beside its zips; load_state_dict() refuses a
                    state that names another disturbance: a run goes on under the noise it was started with."""

    def __init__(self, disturbances, n_members=1):
        ds = self._as_members(disturbances, n_members)
        if any(isinstance(d, CorrelatedDisturbance) for d in ds):
            raise ValueError("the collectors are white-noise only: a CorrelatedDisturbance is for evaluate_policies_fused() and "
                             "MonteCarlo (in a collector an episode spans launches, and the error state does not persist) -- "
                             "a CorrelatedDisturbanceSet holds that state and trains under one")
        self._set_members(ds, n_members)

    @staticmethod
    def _as_members(disturbances, n_members):
        ds = [disturbances] * int(n_members) if isinstance(disturbances, Disturbance) else list(disturbances)
        if not all(isinstance(d, Disturbance) for d in ds):
            raise TypeError("a Disturbance, or one per member, is required, got %r" % (disturbances,))
        return ds

    def _set_members(self, ds, n_members):
        K = int(n_members)
        if len(ds) != K:
            raise ValueError("one Disturbance, or one per member, is required: got %d for %d member(s)" % (len(ds), K))
        for k, d in enumerate(ds):
            for name in ("s_sep", "s_cpa", "s_closing", "s_action"):
                v = getattr(d, name)
                if not (v >= 0.0 and math.isfinite(v)):
                    raise ValueError("member %d: %s = %r (every standard deviation must be finite and at least 0)" % (k, name, v))
        if len({d.seed for d in ds}) != 1:
            raise ValueError("the members' disturbances need EQUAL seeds (one noise seed per launch: an env's noise depends "
                             "on its global index, not on its member), got %s" % [d.seed for d in ds])
        self.members, self.seed = tuple(ds), ds[0].seed
        self.rows = np.asarray([[d.s_sep, d.s_cpa, d.s_closing, d.s_action] for d in ds], np.float32)

    def __len__(self):
        return len(self.members)

    def is_zero(self):
        return all(d.is_zero() for d in self.members)

    def state_dict(self):
        return {"members": [d.to_dict() for d in self.members]}

    def load_state_dict(self, sd):
        other = None if sd is None else [Disturbance.from_dict(d) for d in sd["members"]]
        if other is None or tuple(other) != self.members:
            raise ValueError("load_state_dict: the state was saved under the disturbance %s, this run trains under %s -- "
                             "a run goes on under the noise it was started with" % (
                                 None if other is None else [d.to_dict() for d in other], [d.to_dict() for d in self.members]))


class CorrelatedDisturbanceSet(DisturbanceSet):
    """A DisturbanceSet whose members' errors may PERSIST (acas2d_collect_set_correlated_*): one disturbance for all members
    or K with equal seeds, each a Disturbance (white: rho 0) or a CorrelatedDisturbance.  An episode spans collection
    launches, so the set OWNS the error state between them -- mutable per-env data, which is why the way in is this object
    and not a CorrelatedDisturbance handed to a collector.
      rows, seed, members   as DisturbanceSet's, with the same checks
      corr_rows     float32 [K, 8]: (rho_sep, rho_cpa, rho_closing, rho_action, then their gains records.correlation_gain())
                    per member; the rho were checked when the members were made
      held          None, then the device tensor float32 [3 N + 1, E] of e_{t-1} (row 3 n + c: traffic n's channel c; the last
                    row: the actuator's), zeroed and bound to the env that first collects under the set: a second env, or a
                    state of another E or N, is a ValueError.  reset_held() zeroes it; held_numpy() / load_held(array) carry
                    it across a process restart, next to the env's own state_dict().
      state_dict()  the members' to_dict(), rho keys included where a member has them; load_state_dict() refuses another
                    disturbance or another correlation, in DisturbanceSet's words.
    An env's held value is used where its steps > 1: after the env's reset() the first step of every episode starts the
    processes afresh, so the state needs no reset of its own then."""

    def __init__(self, disturbances, n_members=1):
        ds = self._as_members(disturbances, n_members)
        if any(isinstance(d, DelayedDisturbance) for d in ds):
            raise ValueError("the collectors know no response delay or lag: a DelayedDisturbance is for evaluate_policies_fused() "
                             "and MonteCarlo")
        self._set_members(ds, n_members)
        rho = np.asarray([[getattr(d, name, 0.0) for name in CorrelatedDisturbance.RHO] for d in self.members], np.float32)
        self.corr_rows = np.concatenate([rho, records.correlation_gain(rho)], axis=1).astype(np.float32)
        self.held, self._env, self._pending = None, None, None

    def bind(self, venv):
        """The held state for a collection on `venv`: allocated (zeroed, or from load_held()'s array) at the first call,
        the same tensor at every later one of the same env."""
        shape = (3 * int(venv.n_traffic) + 1, int(venv.num_envs))
        if self._env is not None and self._env() is not venv:
            raise ValueError("this CorrelatedDisturbanceSet holds the error state of another env (the state is per env: one "
                             "set per env)")
        if self.held is None:
            if self._pending is not None and self._pending.shape != shape:
                raise ValueError("load_held: the state is %s, this env needs [3 N + 1, E] = %s"
                                 % (list(self._pending.shape), list(shape)))
            self.held = torch.zeros(shape, dtype=torch.float32, device=venv.device)
            if self._pending is not None:
                self.held.copy_(torch.as_tensor(self._pending))
            self._pending = None
        elif tuple(self.held.shape) != shape:
            raise ValueError("the held state is %s, this env needs [3 N + 1, E] = %s" % (list(self.held.shape), list(shape)))
        self._env = weakref.ref(venv)
        return self.held

    def reset_held(self):
        """Zero the state: every process restarts as q z_t at its next step (as z_t where that step is an episode's first)."""
        self._pending = None
        if self.held is not None:
            self.held.zero_()

    def held_numpy(self):
        """The state as a float32 array [3 N + 1, E] (None before the first collection and without load_held())."""
        if self.held is None:
            return None if self._pending is None else self._pending.copy()
        return self.held.detach().cpu().numpy().copy()

    def load_held(self, array):
        """Put back what held_numpy() gave: at once where the state exists (same shape), else at the first collection."""
        a = np.array(array, np.float32, copy=True)
        if a.ndim != 2:
            raise ValueError("load_held: a [3 N + 1, E] array is required, got %s" % (list(a.shape),))
        if self.held is None:
            self._pending = a
        elif tuple(self.held.shape) != a.shape:
            raise ValueError("load_held: the state is %s, this set holds %s" % (list(a.shape), list(self.held.shape)))
        else:
            self.held.copy_(torch.as_tensor(a))

    def load_state_dict(self, sd):
        make = lambda d: (CorrelatedDisturbance if any(k in d for k in CorrelatedDisturbance.RHO) else Disturbance).from_dict(d)  # noqa: E731
        other = None if sd is None else [make(d) for d in sd["members"]]
        if other is None or tuple(other) != self.members:
            raise ValueError("load_state_dict: the state was saved under the disturbance %s, this run trains under %s -- "
                             "a run goes on under the noise it was started with" % (
                                 None if other is None else [d.to_dict() for d in other], [d.to_dict() for d in self.members]))


def disturbance_draw(seed, first_lane, n_lanes, episode, first_step, n_steps, n_slots, device="cuda:0"):
    """acas2d_disturbance_draw_f32: the standard normals the disturbed kernels draw, [n_steps, n_lanes, n_slots, 3] float32
    (z_sep, z_cpa, z_closing; slot 0: the actuator's normal and two zeros; slot n + 1: traffic n) for lanes first_lane ..,
    steps first_step .. (game.steps before the step) of episode counter `episode` -- computed by the device function the
    kernels call, so a host replay that uses them reproduces a disturbed episode bit for bit."""
    dev = torch.device(device)
    shape = (max(int(n_steps), 0), max(int(n_lanes), 0), max(int(n_slots), 0), 3)
    out = torch.empty(shape, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        native.check(native.lib().acas2d_disturbance_draw_f32(int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_lane), int(n_lanes),
                                                              int(episode), int(first_step), int(n_steps), int(n_slots),
                                                              out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return out.cpu().numpy()


def _scoring_entry(caller, stem, dtype, group, disturbed, correlated=False, delayed=False):
    """The scoring family's C entry for (dtype, group, disturbed, correlated, delayed); group and the three disturbed flavours are
    float32 only, and `caller` says so."""
    disturbed, correlated = disturbed or correlated or delayed, correlated or delayed
    for flag, on in (("group=True", group), ("disturbance=...", disturbed)):
        if on and dtype != torch.float32:
            raise ValueError("%s(%s) is float32 only, got %s" % (caller, flag, dtype))
    if disturbed:
        stem = stem.replace("_stats", "") + ("_delayed" if delayed else "_correlated" if correlated else "_disturbed")
    return "acas2d_%s%s_%s" % (stem, "_group" if group else "", "f32" if dtype == torch.float32 else "f64")


class PolicyBlocks:
    """What the K-policy launches share (acas2d_evaluate_policies_*, acas2d_monte_carlo_*): policy k plays block k of
    EP = round_up(n_per_policy, 64) envs -- its n_per_policy episodes or lanes, then padding that repeats the first -- and
    the launch reads the K policies' stacked weights (stack_policies())."""

    def __init__(self, policies, n_per_policy, obs_dim, device):
        self.n_policies, self.n_per_policy = len(policies), int(n_per_policy)
        self.EP = self.block_envs(n_per_policy)
        self.weights = stack_policies(policies, obs_dim, device)
        self._policy = native.CPolicy(*[t.data_ptr() for t in self.weights], 64, 0)

    @staticmethod
    def block_envs(n_per_policy):
        return (int(n_per_policy) + 63) // 64 * 64               # EP: whole wavefronts (a wavefront's envs belong to ONE policy)

    def index(self, device=None):
        """[K x EP]: which of n_per_policy shared episodes (lanes) each env of the K blocks plays; on `device`, a tensor."""
        idx = np.tile(np.concatenate([np.arange(self.n_per_policy), np.zeros(self.EP - self.n_per_policy, np.int64)]), self.n_policies)
        return idx if device is None else torch.as_tensor(idx, device=device)

    @staticmethod
    def c_eval_stats(st_f, st_i):
        """struct Acas2dEvalStats over st_f [4, K, n]: min_sep, max_a_lat, max_dev, sum_dev; st_i [2, K, n]: min_sep_step, los_steps"""
        return native.CEvalStats(*[t.data_ptr() for t in (st_f[0], st_i[0], st_i[1], st_f[1], st_f[2], st_f[3])])

    def call(self, entry, venv, obs, n_steps, *tail):
        """`entry` on venv's K x EP envs from the observation `obs`: the family's shared arguments, the entry's own `tail`
        (addresses, and structs to pass by reference), the stream"""
        tail = [C.byref(t) if isinstance(t, C.Structure) else t for t in tail]
        native.check(getattr(native.lib(), entry)(
            C.byref(venv._ccfg), C.byref(venv._cstate), venv.num_envs, C.byref(self._policy), self.n_policies, self.n_per_policy,
            obs.data_ptr(), n_steps, venv.seed_value, venv.env_offset, venv.n_traffic, *tail, venv._stream()))


def evaluate_policies_entry(dtype, group=False, safety=False, disturbed=False, correlated=False, delayed=False):
    """The name of the C entry point evaluate_policies_fused() calls for (dtype, group, safety, disturbed, correlated, delayed)."""
    return _scoring_entry("evaluate_policies_fused", "evaluate_policies_stats" if safety else "evaluate_policies", dtype, group,
                          disturbed, correlated, delayed)


def evaluate_policies_fused(policies, own, traffic, goal=None, dtype=torch.float64, device="cuda:0", config=None,
                            max_steps=None, group=False, safety=False, disturbance=None, noise_episode=0, env_offset=0):
    """evaluate_policy_fused() for K policies on the SAME E episodes in ONE launch (acas2d_evaluate_policies_*):
    scoring the checkpoints of a run, or the policies of a seed sweep, together.  `policies`: `SB3ActorPolicy` /
    `ppo.ActorCritic` objects or paths of SB3 zips / .npz exports.  The episodes `own` [E,4] / `traffic` [E,N,4] /
    `goal` are replicated into K blocks of EP = round_up(E, 64) envs (block k: policy k; the padding repeats episode 0
    and is not scored).  Each env stops at the end of its first episode, and nothing per step is stored.
    Returns evaluate_policy_fused()'s keys as [K, E] numpy arrays (outcome, steps, total_reward, path_length) and
    `unfinished` [K]; row k equals evaluate_policy_fused(policies[k], ...) bit for bit.  group=True: the
    group-cooperative float32 launch (acas2d_evaluate_policies_group_f32, N in {8, 16, 32, 64}).
    safety=True: the launch with per-episode safety statistics (acas2d_evaluate_policies_stats_*), over the rows of the
    episode's step() calls (records.episode_safety(): row 0 of the reference's record lists is not among them) -- six
    more [K, E] keys in `dtype`'s precision: min_separation, min_separation_step (1-based step row of the minimum),
    los_steps (step rows inside the safe distance), max_abs_a_lat, max_abs_deviation and mean_abs_deviation (the sum of
    |d_dev| over the steps - 1 rows; 0 where steps <= 1).  An unfinished episode has 0 in all of them.
    disturbance=Disturbance(...): the float32 launch under sensor noise and actuator disturbance
    (acas2d_evaluate_policies_disturbed_*; it always computes the statistics, so the six keys are returned whatever
    `safety` says).  Episode i draws the noise of lane env_offset + i and episode counter `noise_episode`: what lane i of a
    MonteCarlo campaign with the same disturbance and env_offset met in its episode `noise_episode`.
    A CorrelatedDisturbance takes the launch under time-correlated and biased errors (acas2d_evaluate_policies_correlated_*), a
    DelayedDisturbance the one with a response delay and an actuation lag on top (acas2d_evaluate_policies_delayed_*)."""
    from .vec_env import ACAS2DVecEnv
    if not policies:
        raise ValueError("evaluate_policies_fused needs at least one policy")
    if disturbance is None:
        entry = evaluate_policies_entry(dtype, group, safety)
    else:
        delayed = isinstance(disturbance, DelayedDisturbance)         # (the subclass first)
        safety, entry = True, evaluate_policies_entry(dtype, group, True, disturbed=True, delayed=delayed,
                                                      correlated=not delayed and isinstance(disturbance, CorrelatedDisturbance))
    own, traffic = np.asarray(own), np.asarray(traffic)
    E, N = own.shape[0], traffic.shape[1]
    if config is None:
        config = ACAS2DConfig(n_traffic=N)
    dev = torch.device(device)
    blocks = PolicyBlocks(policies, E, config.obs_dim, dev)
    K, idx = blocks.n_policies, blocks.index()
    if goal is not None and np.asarray(goal).ndim == 2:
        goal = np.asarray(goal)[idx]
    v = ACAS2DVecEnv(len(idx), N, device=dev, dtype=dtype, auto_reset=True, config=config, env_offset=int(env_offset))
    v.set_state(own[idx], traffic[idx], goal, np.zeros(len(idx), np.int32), observe=True)
    T = (max_steps or v.config.max_steps) + 1
    outcome = torch.empty(K, E, dtype=torch.uint8, device=dev)
    steps = torch.empty(K, E, dtype=torch.int32, device=dev)
    ret = torch.empty(K, E, dtype=dtype, device=dev)
    tail = [outcome.data_ptr(), steps.data_ptr(), ret.data_ptr()]
    if safety:
        st_f = torch.empty(4, K, E, dtype=dtype, device=dev)                    # min_sep, max_a_lat, max_dev, sum_dev
        st_i = torch.empty(2, K, E, dtype=torch.int32, device=dev)              # min_sep_step, los_steps
        tail.append(blocks.c_eval_stats(st_f, st_i))
    if disturbance is not None:
        # (a DelayedDisturbance: the dead time's ring over the launch's K x EP envs, alive until the results are read back)
        ring = disturbance.ring(len(idx), dev) if isinstance(disturbance, DelayedDisturbance) else None
        tail.extend(_c_tail(disturbance, noise_episode, ring))
    with torch.cuda.device(dev):
        blocks.call(entry, v, v.outputs["obs"], T, *tail)
    oc, st = outcome.cpu().numpy(), steps.cpu().numpy()
    step_len = v.config.airspeed * v.config.dt
    res = {"outcome": oc, "steps": st, "total_reward": ret.cpu().numpy().astype(np.float64),
           "path_length": step_len * (st - 1), "unfinished": (oc == 0).sum(1)}
    if safety:
        f, i = st_f.cpu().numpy(), st_i.cpu().numpy()
        rows = np.maximum(st - 1, 1).astype(f.dtype)
        res.update(min_separation=f[0], min_separation_step=i[0], los_steps=i[1], max_abs_a_lat=f[1],
                   max_abs_deviation=f[2], mean_abs_deviation=np.where(st > 1, f[3] / rows, f.dtype.type(0)))
    return res


def monte_carlo_entry(dtype, group=False, disturbed=False, correlated=False, delayed=False):
    """The name of the C entry point MonteCarlo launches for (dtype, group, disturbed, correlated, delayed)."""
    return _scoring_entry("MonteCarlo", "monte_carlo", dtype, group, disturbed, correlated, delayed)


class MonteCarlo:
    """A Monte Carlo safety campaign (acas2d_monte_carlo_*, include/acas2d.h): K policies play randomly drawn encounters,
    `n_lanes` at a time and one after another per lane, and every finished episode is folded into accumulators that stay
    on the device -- outcome counts, steps, losses of separation, a histogram of the minimum separation, and per lane the
    return sums and the closest encounter.  Every policy meets the SAME encounters (common random numbers): encounter
    (lane, counter) is episode `counter` of RNG index env_offset + lane under `seed`, whichever policy plays it and
    however many there are, so a risk ratio between two rows is a paired comparison and any encounter can be
    regenerated (encounter()).  An all-zero policy is the unequipped aircraft (baseline_main.py's constant action [0]).

    policies   as evaluate_policies_fused(): objects with actor_weights(), paths, or six-tensor tuples
    n_lanes    encounters in flight per policy (the launch covers K x round_up(n_lanes, 64) lanes)
    group      the group-cooperative float32 launch (n_traffic in {8, 16, 32, 64}), else thread-per-env
    n_bins, hist_max   the histogram of min_separation: n_bins bins of hist_max / n_bins, the last one also taking
               everything beyond (default hist_max: 4 x the config's safe distance)
    disturbance  a Disturbance: the campaign under sensor noise and actuator disturbance (acas2d_monte_carlo_disturbed_*,
               float32).  The noise of (lane, counter) is a function of the disturbance's seed, env_offset + lane, the counter
               and the step alone, so the K policies meet the same noise on the same encounters, and encounter() names
               everything a replay needs.  A CorrelatedDisturbance: the campaign under time-correlated and biased errors
               (acas2d_monte_carlo_correlated_*); a lane's error processes restart with every episode it draws.  A
               DelayedDisturbance: with a response delay and an actuation lag on top (acas2d_monte_carlo_delayed_*); the delay
               line and the lag restart with every episode too, and the campaign owns the delay line's ring on the device.
    """

    def __init__(self, policies, n_lanes, seed=13, dtype=torch.float32, group=False, config=None, n_traffic=1, n_bins=64,
                 hist_max=None, device="cuda:0", env_offset=0, disturbance=None):
        from .vec_env import ACAS2DVecEnv
        if not policies:
            raise ValueError("MonteCarlo needs at least one policy")
        delayed = isinstance(disturbance, DelayedDisturbance)         # (the subclass first)
        self.entry = monte_carlo_entry(dtype, group) if disturbance is None else monte_carlo_entry(
            dtype, group, disturbed=True, delayed=delayed, correlated=not delayed and isinstance(disturbance, CorrelatedDisturbance))
        self.disturbance = disturbance
        self.config = config if config is not None else ACAS2DConfig(n_traffic=n_traffic)
        self.n_lanes, self.n_policies, self.dtype, self.seed = int(n_lanes), len(policies), dtype, int(seed)
        if self.n_lanes < 1:
            raise ValueError("MonteCarlo needs at least one lane, got %d" % self.n_lanes)
        self.n_bins = int(n_bins)
        self.hist_max = float(4.0 * self.config.safe_distance if hist_max is None else hist_max)
        self.inv_bin_width = self.n_bins / self.hist_max
        self.first_episode = 0
        K, L = self.n_policies, self.n_lanes
        mk = lambda n, off: ACAS2DVecEnv(n, self.config.n_traffic, device=device, dtype=dtype, seed=seed, env_offset=off,  # noqa: E731
                                         auto_reset=True, config=self.config, keep_terminal_obs=False, double_buffer=False)
        self._src = mk(L, int(env_offset))                       # draws the first episode of a launch
        self.device = dev = self._src.device
        self._blocks = PolicyBlocks(policies, L, self._src.obs_dim, dev)
        self._all = mk(K * self._blocks.EP, int(env_offset))     # ... which is replicated into its K blocks (padding: lane 0)
        self._idx = self._blocks.index(dev)
        self._ring = disturbance.ring(K * self._blocks.EP, dev) if delayed else None     # the dead time's scratch, for every launch
        npdt = np.float32 if dtype == torch.float32 else np.float64
        self._acc = {k: torch.as_tensor(v.view(np.int32) if v.dtype == np.uint32 else v).to(dev)
                     for k, v in records.monte_carlo_empty(K, L, max(self.n_bins, 1), npdt).items()}     # (n_bins < 1: the launch refuses)

    def _launch(self, episodes, events=None):
        """One launch: `episodes` episodes per lane from counter first_episode on.  `events`: a pair of torch.cuda.Events
        to record in front of and behind the kernel alone (tools/bench_monte_carlo.py)."""
        src, dst = self._src, self._all
        src.reset_to_episode(self.first_episode)
        with torch.cuda.device(self.device):
            # the first observation as an injected state's (set_state(observe=True)): what a replay of the encounter
            # through evaluate_policies_fused() starts from, and what the kernel gives the episodes it draws itself
            src.steps.zero_()
            src._launch_reset(None, do_init=0)
            for name in ("own_x", "own_y", "own_psi", "own_v", "goal_x", "goal_y", "trf_x", "trf_y", "trf_psi", "trf_v", "steps",
                         "total_reward"):
                getattr(dst, name).copy_(getattr(src, name)[self._idx])
            dst._obs.copy_(src._obs[self._idx])
            mc = native.CMonteCarlo(*[self._acc[k].data_ptr() for k in records.MONTE_CARLO_KEYS], self.n_bins, int(episodes),
                                    self.inv_bin_width, self.first_episode, 0)
            n_steps = max(int(episodes), 0) * self.config.max_steps
            tail = [mc] if self.disturbance is None else [mc] + _c_tail(self.disturbance, ring=self._ring)
            if events:
                events[0].record()
            self._blocks.call(self.entry, dst, dst._obs, n_steps, *tail)      # (dst has src's seed, env_offset and n_traffic)
            if events:
                events[1].record()
        self.first_episode += int(episodes)

    def run(self, episodes_per_lane, per_launch=8):
        """Play `episodes_per_lane` more episodes on every lane, in launches of at most `per_launch` each (launches stay
        short on purpose: the GPU is shared, and a wave waits for the longest SUM of its lanes' episodes).  The result
        does not depend on per_launch, and run(a) then run(b) equals run(a + b), bit for bit."""
        n, per_launch = int(episodes_per_lane), int(per_launch)
        if n < 1 or per_launch < 1:
            self._launch(n if n < 1 else per_launch)             # the library refuses it in its own words
        while n > 0:
            now = min(n, per_launch)
            self._launch(now)
            n -= now
        return self

    def accumulators(self):
        """The accumulators as numpy arrays (records.MONTE_CARLO_KEYS): one read-back."""
        out = {k: v.cpu().numpy() for k, v in self._acc.items()}
        out["lane_worst_episode"] = out["lane_worst_episode"].view(np.uint32)
        return out

    def summary(self, baseline=None):
        """records.monte_carlo_summary() of the accumulators (one read-back): per policy the episodes, the goal / collision /
        timeout counts and rates, the collision rate's Wilson 95 % interval, the loss-of-separation rate, mean steps, mean
        return and its standard error, the histogram and its edges; with baseline = k0 each policy's risk ratio against k0."""
        out = records.monte_carlo_summary(self.accumulators(), baseline=baseline, hist_max=self.hist_max)
        if self.disturbance is not None:
            out["disturbance"] = self.disturbance.to_dict()
        return out

    def worst(self, m=1):
        """Per policy the `m` lanes with the smallest lane_worst_sep as (lane, counter, min_sep), closest first (ties: the
        lower lane)."""
        acc = self.accumulators()
        out = []
        for sep, ctr in zip(acc["lane_worst_sep"], acc["lane_worst_episode"]):
            order = np.argsort(sep, kind="stable")[:int(m)]
            out.append([(int(i), int(ctr[i]), sep[i]) for i in order])
        return out

    def encounter(self, lane, counter):
        """The encounter (lane, counter) as `own` [1, 4], `traffic` [1, N, 4], `goal` [1, 2] float64 arrays -- ready for
        evaluate_policies_fused(), for ACAS2DVecEnv.set_state() of a latching env with record_trace=True, or for render.
        A campaign with a disturbance returns a fourth item: the keyword arguments that make evaluate_policies_fused()
        replay the DISTURBED episode (disturbance, noise_episode = counter, env_offset = the lane's RNG index)."""
        from .vec_env import ACAS2DVecEnv
        src = self._src
        if not 0 <= int(lane) < self.n_lanes:
            raise ValueError("lane %d of %d" % (lane, self.n_lanes))
        v = ACAS2DVecEnv(1, src.n_traffic, device=self.device, dtype=self.dtype, seed=self.seed, env_offset=src.env_offset + int(lane),
                         auto_reset=True, config=self.config, keep_terminal_obs=False, double_buffer=False)
        v.reset_to_episode(int(counter))
        if self.disturbance is None:
            return read_state(v)
        return read_state(v) + ({"disturbance": self.disturbance, "noise_episode": int(counter),
                                 "env_offset": src.env_offset + int(lane)},)

    def state_dict(self):
        """The accumulators and first_episode (numpy / ints): a campaign survives its process."""
        return {"accumulators": self.accumulators(), "first_episode": int(self.first_episode), "n_lanes": self.n_lanes,
                "n_policies": self.n_policies, "n_bins": self.n_bins, "hist_max": self.hist_max, "seed": self.seed,
                **({} if self.disturbance is None else {"disturbance": self.disturbance.to_dict()})}

    def load_state_dict(self, sd):
        for k in ("n_lanes", "n_policies", "n_bins", "hist_max", "seed"):
            if sd[k] != getattr(self, k):
                raise ValueError("state_dict of another campaign: %s = %r, this one has %r" % (k, sd[k], getattr(self, k)))
        mine = None if self.disturbance is None else self.disturbance.to_dict()
        if sd.get("disturbance") != mine:
            raise ValueError("state_dict of another campaign: disturbance = %r, this one has %r" % (sd.get("disturbance"), mine))
        for k, t in self._acc.items():
            a = np.ascontiguousarray(sd["accumulators"][k])
            t.copy_(torch.as_tensor(a.view(np.int32) if a.dtype == np.uint32 else a))
        self.first_episode = int(sd["first_episode"])
        return self


def encounter_search_entries(dtype, group=False):
    """The names of the C entry points EncounterSearch launches for (dtype, group): sample, evaluate, select (the refit is
    dtype-free: acas2d_encounter_refit)."""
    sfx = "f32" if dtype == torch.float32 else "f64"
    return ("acas2d_encounter_sample_" + sfx, evaluate_policies_entry(dtype, group, safety=True), "acas2d_encounter_select_" + sfx)


class EncounterSearch:
    """A cross-entropy search over encounters with importance sampling (acas2d_encounter_*, include/acas2d.h; Rubinstein's
    cross-entropy method): per generation every policy's `n_candidates` encounters are drawn from ITS proposal -- one
    piecewise-constant density per coordinate of the reset distribution's unit cube -- played by the stats evaluator
    (acas2d_evaluate_policies_stats_*), the closest ones (the smallest min_separation) are kept as the elite and the
    proposal is refit to them; every candidate carries its likelihood ratio against the reset distribution, so each
    generation also gives an unbiased estimate of the probability of min_separation <= level.  K searches run side by
    side, one per policy; with equal proposals they meet the same candidates (common random numbers).  Five launches per
    generation (sample, observe, evaluate, select, refit) and nothing read back in between.  records.search_*() is the
    specification.

    policies      as evaluate_policies_fused(): objects with actor_weights(), paths, or six-tensor tuples
    n_candidates  encounters per policy and generation (the launches cover K x round_up(n_candidates, 64) envs)
    group         the group-cooperative float32 evaluation (n_traffic in {8, 16, 32, 64}), else thread-per-env
    n_bins        bins per coordinate: a power of two, 2 .. 64
    rho           the elite quantile: n_quantile = max(1, ceil(rho x n_candidates)) unless n_quantile is given
    alpha         smoothing of the refit (0: the proposal never moves); p_floor: the least bin probability before the
                  renormalisation (default 1 / (16 n_bins))
    level         the event: min_separation <= level (default: the config's collision distance); the elite threshold never
                  goes below it
    weighted      refit with the likelihood ratios as weights (the cross-entropy update for the reset distribution); False: count
                  the elite (the estimate is then the plain event fraction of the proposal's encounters)
    """

    def __init__(self, policies, n_candidates, seed=13, dtype=torch.float32, group=False, config=None, n_traffic=1, n_bins=8,
                 rho=0.1, alpha=0.7, p_floor=None, level=None, weighted=True, device="cuda:0", env_offset=0, n_quantile=None):
        import math
        from .vec_env import ACAS2DVecEnv
        if not policies:
            raise ValueError("EncounterSearch needs at least one policy")
        self.entries = encounter_search_entries(dtype, group)
        self.config = config if config is not None else ACAS2DConfig(n_traffic=n_traffic)
        self.n_candidates, self.n_policies, self.dtype, self.seed = int(n_candidates), len(policies), dtype, int(seed)
        if self.n_candidates < 1:
            raise ValueError("EncounterSearch needs at least one candidate, got %d" % self.n_candidates)
        self.n_bins, self.alpha, self.weighted = int(n_bins), float(alpha), bool(weighted)
        if self.n_bins < 1:
            raise ValueError("EncounterSearch needs at least one bin, got %d" % self.n_bins)
        self.p_floor = float(1.0 / (16 * self.n_bins) if p_floor is None else p_floor)
        self.level = float(2 * self.config.collision_radius if level is None else level)
        self.n_quantile = int(max(1, math.ceil(float(rho) * self.n_candidates)) if n_quantile is None else n_quantile)
        self.generation = 0
        K, L, N, B = self.n_policies, self.n_candidates, int(self.config.n_traffic), self.n_bins
        self.n_coord = NC = 4 * (N + 1)
        self.device = dev = torch.device(device)
        self._blocks = PolicyBlocks(policies, L, self.config.obs_dim, dev)
        self._env = ACAS2DVecEnv(K * self._blocks.EP, N, device=dev, dtype=dtype, seed=seed, env_offset=int(env_offset), auto_reset=True,
                                 config=self.config, keep_terminal_obs=False, double_buffer=False)
        self.active = records.search_active_coordinates(self.config)
        flat = np.full((K, NC, B), 1.0 / B, np.float64)
        up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        z = lambda *shape, dt=torch.float64: torch.zeros(*shape, dtype=dt, device=dev)  # noqa: E731
        self._buf = b = dict(zip(("p", "cdf", "log_ratio"), (up(t) for t in (flat,) + records.search_tables(flat))))
        self._drawn = {k: v.clone() for k, v in b.items()}       # the tables the last generation was drawn from
        b.update(active=up(self.active.astype(np.uint8)), bins=z(K, NC, L, dt=torch.uint8), log_w=z(K, L), elite_w=z(K, L),
                 outcome=z(K, L, dt=torch.uint8), steps=z(K, L, dt=torch.int32), total_reward=z(K, L, dt=dtype),
                 stats_f=z(4, K, L, dt=dtype), stats_i=z(2, K, L, dt=torch.int32),
                 best_score=torch.full((K,), float("inf"), dtype=dtype, device=dev), best_generation=z(K, dt=torch.int32),
                 best_candidate=torch.full((K,), -1, dtype=torch.int32, device=dev), best_own_psi=z(K, dt=dtype),
                 best_traffic=z(K, N, 4, dt=dtype))
        self._history = z(8, K, native.SEARCH_HISTORY_WIDTH)

    def _struct(self, generation, tables=None, history=None):
        b, t = self._buf, tables or self._buf
        return native.CEncounterSearch(
            t["p"].data_ptr(), t["cdf"].data_ptr(), t["log_ratio"].data_ptr(), b["active"].data_ptr(), b["bins"].data_ptr(),
            b["log_w"].data_ptr(), b["elite_w"].data_ptr(), b["outcome"].data_ptr(), b["stats_f"][0].data_ptr(),
            (self._history[0] if history is None else history).data_ptr(), b["best_score"].data_ptr(),
            b["best_generation"].data_ptr(), b["best_candidate"].data_ptr(), b["best_own_psi"].data_ptr(),
            b["best_traffic"].data_ptr(), self.n_bins, self.n_coord, self.n_quantile, int(self.weighted), self.alpha,
            self.p_floor, self.level, int(generation))

    def _sample(self, cs):
        v = self._env
        native.check(getattr(native.lib(), self.entries[0])(
            C.byref(v._ccfg), C.byref(v._cstate), v.num_envs, self.n_policies, self.n_candidates, v.seed_value, v.env_offset,
            v.n_traffic, C.byref(cs), v._stream()))

    def _generation(self, events=None):
        """One generation's five launches.  `events`: four pairs of torch.cuda.Events around the sample, evaluate, select and
        refit launches (tools/bench_encounter_search.py)."""
        v, b, g, lib = self._env, self._buf, self.generation, native.lib()
        K, L = self.n_policies, self.n_candidates
        mark = (lambda i, j: events[i][j].record()) if events else (lambda i, j: None)
        with torch.cuda.device(self.device):
            if g >= self._history.shape[0]:                      # (a device copy: nothing waits for it)
                self._history = torch.cat([self._history, torch.zeros_like(self._history)])
            cs = self._struct(g, history=self._history[g])
            mark(0, 0)
            self._sample(cs)                                     # the library refuses bad settings here, before any launch
            mark(0, 1)
            for k, t in self._drawn.items():
                t.copy_(b[k])
            v._launch_reset(None, do_init=0)                     # the first observation, as of an injected state
            cstats = self._blocks.c_eval_stats(b["stats_f"], b["stats_i"])
            mark(1, 0)
            self._blocks.call(self.entries[1], v, v._obs, self.config.max_steps + 1, b["outcome"].data_ptr(), b["steps"].data_ptr(),
                              b["total_reward"].data_ptr(), cstats)
            mark(1, 1)
            mark(2, 0)
            native.check(getattr(lib, self.entries[2])(C.byref(v._ccfg), K, L, v.seed_value, v.env_offset, v.n_traffic, C.byref(cs),
                                                       v._stream()))
            mark(2, 1)
            mark(3, 0)
            native.check(lib.acas2d_encounter_refit(C.byref(cs), K, L, v._stream()))
            mark(3, 1)
        self.generation = g + 1

    def run(self, generations):
        """`generations` more generations, queued without a host synchronisation or read-back in between.  run(a) then run(b)
        equals run(a + b), bit for bit."""
        n = int(generations)
        if n < 1:
            raise ValueError("run() needs at least one generation, got %d" % n)
        for _ in range(n):
            self._generation()
        return self

    def history(self):
        """The device log as a numpy array [generations, K, 16] (records.SEARCH_HISTORY_COLUMNS): one read-back."""
        return self._history[:self.generation].cpu().numpy()

    def estimate(self, first_generation=0):
        """records.search_estimate() of the log: per policy the probability of min_separation <= level under the reset
        distribution, per generation and averaged over the generations from first_generation on, with standard errors
        and effective sample sizes."""
        return records.search_estimate(self.history(), self.n_candidates, first_generation)

    def proposal(self):
        """The proposals the NEXT generation will be drawn from: p [K, n_coord, n_bins] float64."""
        return self._buf["p"].cpu().numpy()

    def buffers(self):
        """Every buffer of the search as numpy arrays (the tables, the last generation's bins, log_w, elite_w and evaluation
        results, the log, the archive): what two searches are compared by."""
        out = {k: v.cpu().numpy() for k, v in self._buf.items()}
        out["best_generation"] = out["best_generation"].view(np.uint32)
        out["history"] = self.history()
        return out

    def candidates(self):
        """The last generation as it was drawn: the tables it was drawn from (p, cdf, log_ratio), and per policy the
        candidates' states in the engine's dtype -- own [K, L, 4], traffic [K, L, N, 4], goal [K, L, 2], and the padding envs'
        under padding_* -- their bins [K, L, n_coord], log_w [K, L], outcome and score (min_separation) [K, L].  The states are
        drawn again from the kept tables by the sampler itself (the evaluation has stepped the arrays it wrote)."""
        if self.generation < 1:
            raise RuntimeError("candidates() before the first generation")
        K, L, EP, v = self.n_policies, self.n_candidates, self._blocks.EP, self._env
        with torch.cuda.device(self.device):
            self._sample(self._struct(self.generation - 1, tables=self._drawn))
        f = lambda t: t.detach().cpu().numpy()  # noqa: E731
        own = np.stack([f(v.own_x), f(v.own_y), f(v.own_psi), f(v.own_v)], axis=1).reshape(K, EP, 4)
        trf = np.stack([f(v.trf_x), f(v.trf_y), f(v.trf_psi), f(v.trf_v)], axis=2).reshape(K, EP, v.n_traffic, 4)
        goal = np.stack([f(v.goal_x), f(v.goal_y)], axis=1).reshape(K, EP, 2)
        b = self._buf
        out = {k: f(t) for k, t in self._drawn.items()}
        out.update(generation=self.generation - 1, own=own[:, :L], traffic=trf[:, :L], goal=goal[:, :L], padding_own=own[:, L:],
                   padding_traffic=trf[:, L:], padding_goal=goal[:, L:], steps=f(v.steps).reshape(K, EP),
                   total_reward=f(v.total_reward).reshape(K, EP), bins=f(b["bins"]).transpose(0, 2, 1), log_w=f(b["log_w"]),
                   outcome=f(b["outcome"]), score=f(b["stats_f"][0]), elite_w=f(b["elite_w"]))
        return out

    def best(self):
        """Per policy the closest encounter found so far as (generation, candidate, min_sep, own [1, 4], traffic [1, N, 4],
        goal [1, 2]) -- float64 arrays ready for evaluate_policies_fused() -- or None where no episode has finished yet.  The
        first occurrence wins: the lower generation, then the lower candidate."""
        b = self.buffers()
        cc = self.config.to_c()
        npdt = np.float32 if self.dtype == torch.float32 else np.float64
        out = []
        for k in range(self.n_policies):
            if b["best_candidate"][k] < 0:
                out.append(None)
                continue
            own = np.array([[npdt(cc.own_x0), npdt(cc.own_y0), b["best_own_psi"][k], npdt(cc.own_v)]], np.float64)
            goal = np.array([[npdt(cc.goal_x), npdt(cc.goal_y)]], np.float64)
            out.append((int(b["best_generation"][k]), int(b["best_candidate"][k]), b["best_score"][k], own,
                        b["best_traffic"][k][None].astype(np.float64), goal))
        return out

    _SAVED = ("p", "cdf", "log_ratio", "best_score", "best_generation", "best_candidate", "best_own_psi", "best_traffic")
    _SETTINGS = ("n_candidates", "n_policies", "n_bins", "n_coord", "n_quantile", "alpha", "p_floor", "level", "weighted", "seed")

    def state_dict(self):
        """The proposals, the log, the archive and the generation counter (numpy / numbers): a search survives its process."""
        b = self._buf
        sd = {k: b[k].cpu().numpy() for k in self._SAVED}
        sd.update(drawn={k: v.cpu().numpy() for k, v in self._drawn.items()}, history=self.history(), generation=int(self.generation))
        sd.update({k: getattr(self, k) for k in self._SETTINGS})
        return sd

    def load_state_dict(self, sd):
        for k in self._SETTINGS:
            if sd[k] != getattr(self, k):
                raise ValueError("state_dict of another search: %s = %r, this one has %r" % (k, sd[k], getattr(self, k)))
        for k in self._SAVED:
            self._buf[k].copy_(torch.as_tensor(np.ascontiguousarray(sd[k])))
        for k, t in self._drawn.items():
            t.copy_(torch.as_tensor(np.ascontiguousarray(sd["drawn"][k])))
        h = torch.as_tensor(np.ascontiguousarray(sd["history"])).to(self.device)
        rows = max(8, 2 * h.shape[0])
        self._history = torch.zeros(rows, *self._history.shape[1:], dtype=torch.float64, device=self.device)
        self._history[:h.shape[0]].copy_(h)
        self.generation = int(sd["generation"])
        return self


def read_state(venv):
    """The episodes a vec env holds as (own [E, 4], traffic [E, N, 4], goal [E, 2]) float64 arrays: set_state()'s and
    evaluate_policies_fused()'s arguments."""
    f = lambda t: t.detach().cpu().numpy().astype(np.float64)  # noqa: E731
    own = np.stack([f(venv.own_x), f(venv.own_y), f(venv.own_psi), f(venv.own_v)], axis=1)
    trf = np.stack([f(venv.trf_x), f(venv.trf_y), f(venv.trf_psi), f(venv.trf_v)], axis=2)
    return own, trf, np.stack([f(venv.goal_x), f(venv.goal_y)], axis=1)
