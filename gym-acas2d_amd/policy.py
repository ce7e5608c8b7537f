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
import io
import os
import zipfile

import numpy as np
import torch

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


def evaluate_policies_entry(dtype, group=False, safety=False):
    """The name of the C entry point evaluate_policies_fused() calls for (dtype, group, safety)."""
    if group and dtype != torch.float32:
        raise ValueError("evaluate_policies_fused(group=True) is float32 only, got %s" % (dtype,))
    return "acas2d_evaluate_policies%s%s_%s" % ("_stats" if safety else "", "_group" if group else "",
                                                "f32" if dtype == torch.float32 else "f64")


def evaluate_policies_fused(policies, own, traffic, goal=None, dtype=torch.float64, device="cuda:0", config=None,
                            max_steps=None, group=False, safety=False):
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
    |d_dev| over the steps - 1 rows; 0 where steps <= 1).  An unfinished episode has 0 in all of them."""
    from . import native
    from .vec_env import ACAS2DVecEnv
    if not policies:
        raise ValueError("evaluate_policies_fused needs at least one policy")
    entry = evaluate_policies_entry(dtype, group, safety)
    own, traffic = np.asarray(own), np.asarray(traffic)
    E, N = own.shape[0], traffic.shape[1]
    K, EP = len(policies), (own.shape[0] + 63) // 64 * 64
    idx = np.concatenate([np.arange(E), np.zeros(EP - E, np.int64)])
    idx = np.tile(idx, K)
    if goal is not None and np.asarray(goal).ndim == 2:
        goal = np.asarray(goal)[idx]
    v = ACAS2DVecEnv(K * EP, N, device=device, dtype=dtype, auto_reset=True, config=config)
    D, dev = v.obs_dim, v.device
    v.set_state(own[idx], traffic[idx], goal, np.zeros(K * EP, np.int32), observe=True)
    ws = []
    for pol in policies:
        if isinstance(pol, (str, os.PathLike)):
            pol = load_sb3_policy(pol)
        w = pol.actor_weights() if hasattr(pol, "actor_weights") else pol
        w1, b1, w2, b2, w3, b3 = (torch.as_tensor(t, dtype=torch.float32).to(dev) for t in w)
        if w1.shape != (64, D) or w2.shape != (64, 64) or w3.numel() != 64 or b3.numel() != 1:
            raise ValueError("policy must be the SB3 MlpPolicy actor %d -> 64 -> 64 -> 1, got %s %s %s"
                             % (D, tuple(w1.shape), tuple(w2.shape), tuple(w3.shape)))
        ws.append(kernel_layout(w1, b1, w2, b2, w3, b3))
    keep = [torch.stack(ts) for ts in zip(*ws)]                                  # [K][D][64], [K][64], ...
    T = (max_steps or v.config.max_steps) + 1
    outcome = torch.empty(K, E, dtype=torch.uint8, device=dev)
    steps = torch.empty(K, E, dtype=torch.int32, device=dev)
    ret = torch.empty(K, E, dtype=dtype, device=dev)
    pw = native.CPolicy(*[t.data_ptr() for t in keep], 64, 0)
    fn = getattr(native.lib(), entry)
    extra = ()
    if safety:
        st_f = torch.empty(4, K, E, dtype=dtype, device=dev)                    # min_sep, max_a_lat, max_dev, sum_dev
        st_i = torch.empty(2, K, E, dtype=torch.int32, device=dev)              # min_sep_step, los_steps
        cstats = native.CEvalStats(st_f[0].data_ptr(), st_i[0].data_ptr(), st_i[1].data_ptr(), st_f[1].data_ptr(),
                                   st_f[2].data_ptr(), st_f[3].data_ptr())
        extra = (C.byref(cstats),)
    with torch.cuda.device(dev):
        native.check(fn(C.byref(v._ccfg), C.byref(v._cstate), K * EP, C.byref(pw), K, E, v.outputs["obs"].data_ptr(), T,
                        v.seed_value, v.env_offset, N, outcome.data_ptr(), steps.data_ptr(), ret.data_ptr(),
                        *extra, v._stream()))
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
