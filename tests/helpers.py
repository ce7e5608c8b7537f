"""Shared test machinery: golden-vector loading, engine-agnostic replay loops and the one reader of kernel metadata.

An "engine" here is anything with the OracleEnvs interface (oracle/oracle.py): numpy float64
views  own_x, own_y, own_psi, trf_x, trf_y, steps, total_reward  plus
set_state(own, trf, goal, steps), observe(), step(actions) -> (obs, reward, done, outcome, n).
The CPU oracle implements it natively; tests/test_gpu_parity.py wraps the HIP path in the same
interface so that both are checked by the same code against the same fixtures.
"""
import os
import random
import re
import shlex
import shutil
import subprocess
from collections import namedtuple

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gym-acas2d_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def load(name):
    return np.load(os.path.join(GOLDEN, name))


def parity_reset_states(cfg, seed, skip, count):
    """Episodes number skip .. skip+count-1 of the reference's MT19937 stream after seed."""
    import gym_acas2d_amd as g
    rng = random.Random(seed)
    if skip:
        g.reset_parity.draw_episodes(cfg, skip, rng)
    return g.reset_parity.draw_episodes(cfg, count, rng)


def rollout_as_batch(fx):
    """Reference rollout fixture (one env, reset on done) -> one env per episode:
    acts [T, n_ep], valid [T, n_ep], rows [T] list of fixture row indices ordered by episode."""
    n_ep = len(fx["ep_own"])
    T = int(np.bincount(fx["ep"]).max())
    acts = np.zeros((T, n_ep))
    valid = np.zeros((T, n_ep), bool)
    acts[fx["k"], fx["ep"]] = fx["action"]
    valid[fx["k"], fx["ep"]] = True
    rows = []
    for k in range(T):
        r = np.nonzero(fx["k"] == k)[0]
        rows.append(r[np.argsort(fx["ep"][r])])
    return acts, valid, rows


def replay_rollout(engine, fx):
    """Step `engine` (already holding the fixture's initial states, observe() done) through the
    fixture's action streams.  Returns worst absolute errors and mask mismatch counts."""
    acts, valid, rows = rollout_as_batch(fx)
    res = dict(obs=0.0, reward=0.0, pos=0.0, psi=0.0, total_reward=0.0, done_mismatch=0,
               outcome_mismatch=0, steps_mismatch=0, n=0)
    for k in range(acts.shape[0]):
        obs, reward, done, outcome, _ = engine.step(acts[k])
        sel = np.nonzero(valid[k])[0]
        r = rows[k]
        assert np.array_equal(fx["ep"][r], sel)
        res["obs"] = max(res["obs"], float(np.nanmax(np.abs(obs[sel] - fx["obs"][r]))))
        assert np.array_equal(np.isnan(obs[sel]), np.isnan(fx["obs"][r]))
        res["reward"] = max(res["reward"], float(np.abs(reward[sel] - fx["reward"][r]).max()))
        own = np.stack([engine.own_x, engine.own_y], 1)[sel]
        res["pos"] = max(res["pos"], float(np.abs(own - fx["own"][r][:, :2]).max()),
                         float(np.abs(np.stack([engine.trf_x, engine.trf_y], -1)[sel] - fx["trf_xy"][r]).max()))
        res["psi"] = max(res["psi"], float(np.abs(engine.own_psi[sel] - fx["own"][r][:, 2]).max()))
        res["total_reward"] = max(res["total_reward"],
                                  float(np.abs(engine.total_reward[sel] - fx["total_reward"][r]).max()))
        res["done_mismatch"] += int((done[sel].astype(bool) != fx["done"][r].astype(bool)).sum())
        res["outcome_mismatch"] += int((outcome[sel] != fx["outcome"][r]).sum())
        res["steps_mismatch"] += int((engine.steps[sel] != fx["steps"][r]).sum())
        res["n"] += len(sel)
    return res


def replay_baseline(engine, digest, own, trf):
    """baseline_main.simulate() (baseline_main.py:32-61): constant action 0 until done, for the
    100 episodes of the reference's CSV as one batch of 100 envs.  `engine` must already hold
    the initial states (set_state + observe).  Returns what the CSV digest pins."""
    E = len(own)
    stride = int(digest["stride"])
    outcome = np.zeros(E, np.uint8)
    steps = np.zeros(E, np.int32)
    ret = np.zeros(E)
    last = np.zeros((E, 2))
    sub = np.full_like(digest["own_sub"], np.nan)
    tsub = np.full_like(digest["trf_sub"], np.nan)
    sub[:, 0] = own[:, :2]
    tsub[:, 0] = trf[:, 0, :2]
    first2 = np.zeros((E, 2, 2))
    first2[:, 0] = own[:, :2]
    prev_t = trf[:, 0, :2].copy()
    active = np.ones(E, bool)
    zeros = np.zeros(E)
    for k in range(1, 1001):
        _, _, done, oc, _ = engine.step(zeros)
        pos = np.stack([engine.own_x, engine.own_y], 1)
        if k == 1:
            first2[:, 1] = pos
        fin = active & (done != 0)
        if k % stride == 0:
            # Path[k] = player after k steps; Traffic Paths[k] = traffic BEFORE step k's move
            # (game.py:231-233 logs before :243-245 moves)
            sub[active, k // stride] = pos[active]
            tsub[active, k // stride] = prev_t[active]
        prev_t = np.stack([engine.trf_x[:, 0], engine.trf_y[:, 0]], 1)
        outcome[fin] = oc[fin]
        steps[fin] = engine.steps[fin]
        ret[fin] = engine.total_reward[fin]
        last[fin] = pos[fin]
        active &= ~fin
        if not active.any():
            break
    return dict(outcome=outcome, steps=steps, total_reward=ret, own_last=last, own_sub=sub,
                trf_sub=tsub, own_first2=first2, unfinished=int(active.sum()))


# notebooks/simulation_ACAS2D_PPO_1048576_11_100.ipynb cell 4: `simulation.describe()` of the
# reference's own 100-episode deterministic evaluation of best_model_1048576_11 (testing_main.py)
REF_POLICY_EVAL = {
    "Total Reward": dict(mean=1210.069219, std=69.336537, min=1099.788122, q25=1157.389870,
                         q50=1200.470752, q75=1245.515314, max=1370.264607),
    "Time Steps": dict(mean=704.35, std=73.826082, min=634, q25=656, q50=681, q75=721, max=927),
    "Path Length": dict(mean=1406.70, std=147.652164, min=1266, q25=1310, q50=1360, q75=1440, max=1852),
}


def describe(v):
    v = np.asarray(v, np.float64)
    return dict(mean=v.mean(), std=v.std(ddof=1), min=v.min(), q25=np.percentile(v, 25),
                q50=np.percentile(v, 50), q75=np.percentile(v, 75), max=v.max())


def assert_matches_reference_policy_eval(total_reward, steps, path_length, tol=2e-6):
    """Every printed digit of the reference's table (6 decimals) must be reproduced."""
    got = {"Total Reward": describe(total_reward), "Time Steps": describe(steps),
           "Path Length": describe(path_length)}
    for col, want in REF_POLICY_EVAL.items():
        for k, w in want.items():
            assert abs(got[col][k] - w) <= tol * max(1.0, abs(w)), (col, k, got[col][k], w)


# ---- code-object metadata -----------------------------------------------------------------------------------------------
needs_hipcc = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="needs hipcc")


class Kernel(namedtuple("Kernel", "name entry")):
    """One kernel of a code object: its mangled name and its whole entry of amdhsa.kernels (every field, the ones sorted
    before .name -- group_segment_fixed_size, max_flat_workgroup_size -- included)."""
    __slots__ = ()

    def field(self, key):
        return int(re.search(r"^    \.%s:\s+(\d+)$" % key, self.entry, re.M).group(1))


def kernel_metadata(tmp_path, unit):
    """csrc/<unit> (say "acas2d_ppo_set.hip") compiled to device assembly WITH THE FLAGS THE MAKEFILE GIVES IT: the compile
    command of <unit>.o is taken from a dry run of make (nothing is built, nothing is written into the tree) and its
    `-c <unit> -o <unit>.o` swapped for `-S --cuda-device-only -o <tmp_path>/<unit>.s`.  Returns the assembly text and one
    Kernel per kernel of the unit."""
    hipcc = HIPCC if os.path.exists(HIPCC) else "hipcc"
    obj = unit[:-len(".hip")] + ".o"
    dry = subprocess.run(["make", "-n", "-B", "HIPCC=" + hipcc, obj], cwd=CSRC, check=True, capture_output=True, text=True)
    cmd, = [shlex.split(ln) for ln in dry.stdout.splitlines() if ln.endswith(" -c %s -o %s" % (unit, obj))]
    asm = tmp_path / (unit + ".s")
    subprocess.run(cmd[:-4] + ["-S", "--cuda-device-only", "-o", str(asm), unit], cwd=CSRC, check=True, capture_output=True)
    text = asm.read_text()
    entries = ["    .agpr_count:" + e for e in re.split(r"\n  - \.agpr_count:", text.split("amdhsa.kernels:")[1])[1:]]
    return text, [Kernel(re.search(r"^    \.name:\s+(\S+)$", e, re.M).group(1), e) for e in entries]


# ---- work-shape coverage ------------------------------------------------------------------------------------------
# step_kernel is instantiated once per work shape: C traffic aircraft per lane as one vector, G lanes per env (the
# packed shapes of ACAS2D_PACKED_SHAPES in gym-acas2d_amd/csrc/acas2d_f32.hip / acas2d_f64.hip), or the generic
# strided walk with G in {1, 4, 16, 64} lanes per env (any N).  One row per shape and build -- float32 (FAST), and the
# float64 build in each of its formulations -- with the N that reaches it, through choose_shape() (override None) or
# ACAS2D_SHAPE.  C is None for the generic walk.  tests/test_host.py holds this table to the .hip lists; the GPU
# tests of tests/test_gpu_parity.py run every row.
class Shape(namedtuple("Shape", "dtype math n_traffic override C G")):
    """dtype "float32" / "float64"; math "fast" / "exact" (float32 has FAST only); override: ACAS2D_SHAPE, or None
    for the default choice."""
    __slots__ = ()
    packed = property(lambda s: s.C is not None)
    elem = property(lambda s: 4 if s.dtype == "float32" else 8)
    dtype_name = property(lambda s: "float64fast" if (s.dtype == "float64" and s.math == "fast") else s.dtype)

    @property
    def id(self):
        shape = "%d,%d" % (self.C, self.G) if self.packed else "generic,%d" % self.G
        return "%s-N%d-%s%s" % (self.dtype_name, self.n_traffic, shape, "" if self.override is None else "-override")

    @property
    def envs_per_wave(self):
        return 64 // self.G

    @property
    def reset_slots(self):
        """Envs one pass of the in-step reset takes (geometry_for() / ResetSlots in the kernels): a packed shape with
        N + 1 <= 32 has 64 / stride slots, stride the power of two >= max(2, N + 1); the others reset one env per pass."""
        if not self.packed or self.n_traffic + 1 > 32:
            return 1
        stride = 2
        while stride < self.n_traffic + 1:
            stride *= 2
        return 64 // stride


def _rows(dtype, math, rows):
    return [Shape(dtype, math, n, ov, c, gl) for n, ov, c, gl in rows]


_F32 = [(1, None, 1, 1), (2, None, 2, 1), (3, None, 3, 1), (4, None, 4, 1), (8, "8,1", 8, 1), (8, None, 4, 2),
        (8, "2,4", 2, 4), (16, None, 4, 4), (32, None, 4, 8), (64, None, 4, 16), (64, "8,8", 8, 8), (64, "2,32", 2, 32),
        (8, "generic,1", None, 1), (5, None, None, 4), (33, None, None, 16), (100, None, None, 64)]
_F64 = [(1, None, 1, 1), (2, None, 2, 1), (3, None, 3, 1), (4, None, 4, 1), (8, "2,4", 2, 4), (8, None, 4, 2),
        (16, None, 4, 4), (32, None, 4, 8), (64, "2,32", 2, 32), (64, None, 4, 16),
        (3, "generic,1", None, 1), (5, None, None, 4), (17, None, None, 16), (100, None, None, 64)]
SHAPES = _rows("float32", "fast", _F32) + _rows("float64", "exact", _F64) + _rows("float64", "fast", _F64)
GENERIC_G = (1, 4, 16, 64)


# ---- the fused collector ----------------------------------------------------------------------------------------------
def bits_equal(x, y):
    """torch.equal on the bit patterns (a NaN d_cpa -- exact parallel flight, kinematics.py:48 -- equals itself)."""
    import torch
    if x.is_floating_point():
        bits = torch.int32 if x.dtype == torch.float32 else torch.int64
        return x.shape == y.shape and torch.equal(x.contiguous().view(bits), y.contiguous().view(bits))
    return torch.equal(x, y)


def replay_collect_on_twin(env, twin, out):
    """A twin of `env` (same construction, same state before collect()) stepped with the clipped actions of the
    collect() dict `out` reproduces every observation, reward and mask bit for bit, some episodes end on the way, and
    both envs end in the same state.  Returns the number of finished episodes."""
    import torch
    T = out["actions"].shape[0]
    act = out["actions"].to(torch.float32)
    dones = 0
    for t in range(T):
        o, r, d, _ = twin.step(act[t].clamp(-1, 1).to(twin.dtype))
        assert bits_equal(o, out["obs"][t + 1]) and bits_equal(r, out["reward"][t]) and bits_equal(d, out["done"][t]), t
        dones += int(d.sum())
    assert dones > 0 and bits_equal(env.outputs["obs"], out["obs"][T])
    for name in ("own_x", "trf_x", "steps", "episode", "total_reward"):
        assert torch.equal(getattr(env, name), getattr(twin, name)), name
    return dones


# ---- non-default configurations ---------------------------------------------------------------------------------------
# ACAS2DConfig keyword sets in which every tunable differs from settings.py (tests/test_host.py checks that, field by
# field of to_c()).  "wide": a larger, slower-framed airspace with an airspeed-factor range and short episodes -- no goal
# is reachable within its 120 steps; "small": a small airspace in which goals, collisions and timeouts all occur within
# a few dozen steps after step 80, so the goal bonus and the step-reward decay are covered too.
NONDEFAULT_CONFIGS = {
    "wide": dict(max_steps=120, width=2000, height=1200, fps=50, aircraft_size=20, airspeed=180, airspeed_factor_min=0.8,
                 airspeed_factor_max=1.3, acc_lat_limit=150.0, player_initial_heading_lim=10,
                 traffic_initial_heading_lim=25, reward_goal=500, reward_collision=-750),
    "small": dict(max_steps=82, width=700, height=500, fps=40, aircraft_size=16, airspeed=240, airspeed_factor_min=0.7,
                  airspeed_factor_max=1.2, acc_lat_limit=120, player_initial_heading_lim=5,
                  traffic_initial_heading_lim=20, reward_goal=400, reward_collision=-600),
}


def oracle_config(O, cfg):
    """OracleConfig carrying the product configuration `cfg` (same field names)."""
    cc, oc = cfg.to_c(), O.OracleConfig()
    for name, _ in O.OracleConfig._fields_:
        if name != "_pad":                      # (the product's `math` selector: the oracle has one formulation)
            setattr(oc, name, getattr(cc, name))
    return oc


def f32_oracle_steps(O, E, N, T, seed=13, env_offset=0, warmup=None, config=None, episode=None):
    """The oracle side of a float32-vs-oracle window: a free-running float64 oracle trajectory `ref` with auto-reset and
    actions from default_rng(7), `warmup` steps first (None: 3 at N = 64, where episodes last ~8 steps, else 15..29 drawn
    from the same stream), then T steps.  For each of those it yields (t, own, trf, steps, episode, act, chk, stepped):
    ref's state rounded to float32 (the state both sides start the step from), the float32-representable action, and the
    oracle `chk` stepped once from that state -- stepped = chk.step()'s (o, r, d, oc).  `config`: an OracleConfig, None
    for the default one; `episode`: the episode counters [E] after reset() (None: 0)."""
    f32 = lambda a: a.astype(np.float32).astype(np.float64)  # noqa: E731
    ref = O.OracleEnvs(E, N, seed=seed, env_offset=env_offset, auto_reset=True, config=config)
    ref.reset()
    if episode is not None:
        ref.episode[:] = episode
    rng = np.random.default_rng(7)
    if warmup is None:
        warmup = 3 if N == 64 else int(rng.integers(15, 30))
    for _ in range(warmup):
        ref.step(rng.uniform(-1, 1, E))
    chk = O.OracleEnvs(E, N, seed=seed, env_offset=env_offset, auto_reset=True, config=config)
    for t in range(T):
        own = f32(np.stack([ref.own_x, ref.own_y, ref.own_psi, ref.own_v], 1))
        trf = f32(np.stack([ref.trf_x, ref.trf_y, ref.trf_psi, ref.trf_v], -1))
        steps, act = ref.steps.copy(), f32(rng.uniform(-1, 1, E))
        chk.set_state(own, trf, None, steps)
        chk.episode[:] = ref.episode
        o, r, d, oc, _ = chk.step(act)
        yield t, own, trf, steps, ref.episode.copy(), act, chk, (o, r, d, oc)
        ref.step(act)


# The float32 bounds of tests/test_gpu_parity.py (_check_f32_step_vs_oracle), derived from the configuration -- `cfgc`,
# an OracleConfig -- by the rules its docstring states.  For the default configuration each evaluates to the fixed number
# the tests used before it was derived (tests/test_host.py holds them to those numbers).
def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def f32_pos_bound(m):
    """Positions after one step, |coordinates| up to m: 1 float32 ulp -- 1.3e-4 below 2048 px (ulp 1.22e-4)."""
    return max(1.3e-4, ulp32(m))


def f32_bounds(cfgc, dflt):
    """dflt: the default OracleConfig (the reward bound scales with the configuration's d_cpa amplification over the
    default's).  speed None: the speed factor is a single value, the fresh speeds must be bit-equal."""
    extent = max(cfgc.t0_x, cfgc.tn_x_max, cfgc.t0_y_base + cfgc.t0_y_span, cfgc.tn_y_max)
    amp = (cfgc.d_cpa_max / cfgc.safe_distance) / (dflt.d_cpa_max / dflt.safe_distance)
    density = (cfgc.collision_dist / (cfgc.tn_x_max * cfgc.tn_y_max)) / (dflt.collision_dist / (dflt.tn_x_max * dflt.tn_y_max))
    fmin, fmax = cfgc.speed_factor_min, cfgc.speed_factor_max
    return dict(
        # the fraction of envs a step may leave inside the 1e-3 px band around the thresholds: the chance that an aircraft
        # lies in the band grows with the collision distance over the area the traffic is drawn in
        band=1e-3 * max(1.0, density),
        # terminal reward / episode return (total_reward starts each checked step at 0): 1 ulp of the bonus, + 1e-5 for
        # the shaped part
        ret=max(1.3e-4, ulp32(max(abs(cfgc.reward_goal), abs(cfgc.reward_collision)))) + 1e-5,
        # the non-terminal reward: (d_cpa / safe_distance)^4 amplifies the d_cpa entry's error (a fraction of d_cpa_max)
        # by up to 4 d_cpa_max / safe_distance -- 39x by default, where 5e-5 holds
        rew=5e-5 * max(1.0, amp),
        # fresh episode (float32 draws from 24 random bits): 2 ulp of the largest drawn coordinate, headings 2 ulp of 360
        reset_pos=max(2.5e-4, 2 * ulp32(extent)),
        reset_psi=6e-5,
        # fresh speeds: 24 random bits against 32 move the factor by < 2^-24 of the range, plus the float32 rounding
        speed=None if fmin == fmax else (fmax - fmin) * cfgc.airspeed * 2.0 ** -24 + 2 * ulp32(fmax * cfgc.airspeed))


# Where the non-default windows of tests/test_gpu_parity.py run (seed, env_offset, oracle warm-up steps, checked steps)
# and which outcomes the CPU oracle produces there -- the outcomes each test asserts it compared.  tests/test_host.py
# runs the oracle over every window and holds these sets to what really occurs.
GOAL, COLLISION, TIMEOUT = 1, 2, 3
NONDEFAULT_SHAPE_WINDOW = dict(wide=dict(seed=3, env_offset=37, warmup=100, T=30),
                               small=dict(seed=3, env_offset=37, warmup=75, T=40))
# (N, E, T) of the odd-traffic-count tests of tests/test_gpu_parity.py.  The float32 one runs "wide" in a window that starts
# at step 100, so the episodes that last reach their timeout at step 121 inside it
ODD_TRAFFIC = ((2, 1500, 80), (5, 777, 90), (6, 1024, 60), (7, 333, 60), (12, 640, 50), (33, 200, 30))
NONDEFAULT_ODD_WINDOW = dict(seed=3, env_offset=17, warmup=100)


def nondefault_outcomes(name, N):
    """The outcomes the CPU oracle produces at least 5 times in the shape window NONDEFAULT_SHAPE_WINDOW[name] at N
    traffic (measured; tests/test_host.py re-measures them): crowded airspaces end every episode in a collision before
    its goal or timeout, and "wide" with one aircraft collides nowhere."""
    if name == "wide":
        return {TIMEOUT} if N == 1 else {COLLISION, TIMEOUT}
    return {GOAL, COLLISION, TIMEOUT} if N <= 16 else {GOAL, COLLISION} if N <= 33 else {COLLISION}


# ---- wide reset keys --------------------------------------------------------------------------------------------------
# Every episode is the Philox4x32-7 block of counter (global env index lo, hi, episode, entity) under key (seed lo, hi).
# These keys make every one of those words matter: a seed whose halves are non-zero and distinct, an env_offset that puts
# the 2^32 crossing of the global env index inside a wave (and so inside a workgroup) of WIDE_E envs -- "mid" -- or in
# the last, partial wave of the shapes with >= 16 envs per wave -- "tail" --, and episode counters at 2^32 - 2 on the
# even envs (WIDE_PRESET), so that their second reset wraps the counter to 0.  tests/test_host.py holds every shape of
# SHAPES to these claims; the GPU tests of tests/test_gpu_parity.py run at these keys.
WIDE_SEED = 0x9E3779B97F4A7C15
WIDE_E = 1001
WIDE_CROSSING = dict(mid=501, tail=999)            # the local env whose global index is 2^32
WIDE_OFFSET = {k: 2 ** 32 - c for k, c in WIDE_CROSSING.items()}
WIDE_EPISODE = 2 ** 32 - 2


def wide_preset(E):
    """The envs whose episode counter starts at WIDE_EPISODE: the even ones (every wave holds both kinds)."""
    return np.arange(E) % 2 == 0


def wide_crossing_offset(E, wave):
    """An env_offset for a launch of E envs in waves of `wave` envs: the 2^32 crossing at the middle wave's lane
    max(1, wave / 2 - 1) -- inside it unless a wave holds one env (then at its lane 0)."""
    return 2 ** 32 - ((E // wave) // 2 * wave + (max(1, wave // 2 - 1) if wave > 1 else 0))


def wide_f32_window(N):
    """(oracle warm-up steps, checked steps) of the float32 wide-key windows (max_steps = 40): wraps of the preset
    counters happen inside them -- at the first collisions of crowded airspaces, at the second timeout (step 80) of one
    aircraft, at the first timeouts (step 40, the collisions before it took the first reset) of a few."""
    return (75, 8) if N == 1 else (36, 8) if N <= 5 else (0, 8)


# ---- 32-bit offset limits ---------------------------------------------------------------------------------------------
# The float32 "arena" step kernel addresses its state through 32-bit byte offsets (acas2d_launch.inl arena_layout):
# it takes E envs x N traffic only while 8 E N < 2^32 (the [2][E][N] traffic blocks) and 20 E < 2^32 (the [5][E] block).
# (N, largest admitted E, first rejected whole-workgroup E) at the bound -- N = 2: the 20 E term binds.
ARENA_BOUND = ((8, 67107840, 67108864), (64, 8388480, 8388608), (2, 214747136, 214749184))


def obs_row_crossing(D, elem):
    """The env whose observation row [E][D] of `elem`-byte elements straddles byte 2^32."""
    return (2 ** 32) // (D * elem)

