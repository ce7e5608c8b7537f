"""Shared by tests/test_safety_scenes.py (CPU) and tests/test_eval_stats_oracle.py (GPU): hand-placed scenes for the
per-episode safety statistics of the fused evaluator and their reference, WITH NO PROJECT KERNEL IN IT.

Reference.  The float64 CPU oracle (oracle.OracleEnvs, auto_reset=False) is stepped from set_state() + observe() with
given actions.  Per step row, in NumPy float64:
  d_sep   min over aircraft of hypot(player AFTER the oracle's step() - traffic copied BEFORE it) (game.py:236-237
          against :243-245); +inf where no distance is finite
  a_lat   action * acc_lat_limit
  d_dev   obs[:, 2] * d_dev_max of the observation that step returns (game.py:175-180)
Rows run up to and including each env's first non-zero outcome; records.episode_safety(dtype=float64) /
safety_summary() reduce them (held to the reference game's own record lists by tests/test_eval_stats_host.py).  They
drop list entry 0, so the row arrays here carry a dummy row 0.

Scenes.  scenes(cfg, O): see its docstring.  Every number of an initial state is representable in float32, so every
build starts from the same state as the reference.

Policies.  K = 4 per launch.  Three constant-action ActorCritics (action_net.weight zeroed, bias 0, 0.375, -3): the
action is the bias clipped to [-1, 1] for every finite observation and NaN after a NaN one, known without any kernel.
One random policy with its head scaled by 40: its actions come from ACAS2DVecEnv.rollout_policy() at the dtype under test
(GPU); the CPU test stands a seeded random walk in for it.

Bound B of the comparison (bound()):
  float64 exact   1e-9 px: what test_testing_main_record_columns_vs_reference holds whole-episode record columns to
  float64 FAST    rows x 1e-11: the asserted one-step position bound of that formulation (tests/test_gpu_parity.py) times
                  the number of step rows
  float32         4 x D, never below rows x helpers.f32_pos_bound(extent).  D (drift()) is measured on the oracle alone:
                  the same scenes and actions once plain and once with the state rounded to float32 after every step
                  (the rounding of helpers.f32_oracle_steps), D = the largest difference in d_sep and |d_dev| over the
                  rows both runs have.  The factor 4: the kernel also rounds its arithmetic (sincos, fma, rcp) in
                  float32, a handful of operations per coordinate and step on top of the storage rounding D captures.
Measured on an MI355X (the random policy's real actions; rows = max_steps; D comes from the 120-row timeout scenes, so the
CPU stand-in gives the same D except at N = 8 and small N = 16).  Floor: 120 x 1.3e-4 = 0.0156 px below 2048 px, 120 x
2.44e-4 = 0.0293 px where a scene's traffic flies beyond it, 82 x 1.3e-4 = 0.01066 px in "small".
  shape                     D        B         worst error of min_separation / max_abs_deviation / mean_abs_deviation
  float32 N = 1             3.53e-3  0.0156    8.8e-4 / 9.6e-4 / 8.5e-4 px
  float32 N = 2             5.40e-3  0.0216    8.8e-4 / 1.8e-3 / 8.1e-4
  float32 N = 3             7.94e-3  0.0318    8.8e-4 / 3.1e-3 / 1.6e-3
  float32 N = 4             5.37e-3  0.0293    6.1e-4 / 8.6e-4 / 5.9e-4
  float32 N = 8, 8 group    3.55e-3  0.0156    8.8e-4 / 7.9e-4 / 7.1e-4 (both entries)
  float32 N = 16 group      7.92e-3  0.0317    7.8e-4 / 1.6e-3 / 7.9e-4
  float32 N = 32 group      9.07e-3  0.0363    8.8e-4 / 1.3e-3 / 8.1e-4
  float32 N = 64 group      7.28e-3  0.0293    8.8e-4 / 7.9e-4 / 5.2e-4
  float32 small N = 3       1.46e-3  0.01066   2.3e-4 / 1.1e-3 / 5.4e-4
  float32 small N = 16 grp  2.06e-3  0.01066   2.6e-4 / 7.0e-4 / 3.5e-4
  float64 exact (all N)     -        1e-9      1.1e-13 / <= 1.4e-13 / <= 2.1e-14
  float64 FAST N = 1, 4     -        1.2e-9    1.3e-13 / 6.0e-13 / 3.4e-13
Of the 356 episodes of a launch, 329 .. 334 (float32) / 346 (float64) have a single candidate row and 349 .. 354 a single
loss-of-separation count: those are decided by equality.  Trace rows of the latching kernel (b = 0.375): d_sep / d_dev
within 2.7e-3 / 2.2e-4 px at float32 N = 8 (8,1), 7.3e-3 / 4.1e-4 px at N = 64 (4,16), 1.1e-13 / 5.0e-13 px at float64
N = 4; a_lat exact.  The exact scenes (tie, threshold, twin, nan) came out exactly in every build.
"""
import math
from collections import namedtuple

import numpy as np

MAX_STEPS = 120                                     # default config; "small" keeps its own 82
CONST_BIAS = (0.0, 0.375, -3.0)
K = len(CONST_BIAS) + 1
SMOOTH = 1                                          # index of the b = 0.375 policy (the trace comparison)
MARGIN = 0.25                                       # of a step length: how far every scene keeps the goal / collision thresholds
N_NEAR = 64                                         # nearest-at-slot scenes at least (N of them where N is larger)
TIE_ROW = 21

Scenes = namedtuple("Scenes", "own trf goal family slot")
Rows = namedtuple("Rows", "outcome steps d_sep a_lat d_dev margin extent")
Reference = namedtuple("Reference", "outcome steps d_sep a_lat d_dev stats margin extent actions")

f32 = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)  # noqa: E731


def config(g, N, name="default", fast=False):
    import helpers as H
    if name == "default":
        return g.ACAS2DConfig(n_traffic=N, max_steps=MAX_STEPS, fast_math=fast)
    return g.ACAS2DConfig(n_traffic=N, fast_math=fast, **H.NONDEFAULT_CONFIGS[name])


def step_len(cfg):
    return float(cfg.airspeed) * cfg.dt


def exact_scenes_hold(cfg):
    """The tie / threshold scenes need a step length, and half of it, that float32 reproduces exactly."""
    s = step_len(cfg)
    v, dt = np.float32(cfg.airspeed), np.float32(cfg.dt)
    return (s == round(s) and float(v * dt) == s and float(np.float32(0.5) * v * dt) == s / 2
            and float(cfg.safe_distance).is_integer())


# ---- the scenes ---------------------------------------------------------------------------------------------------------
def _plan(cfg):
    """(family, slot, variant) per scene."""
    N = cfg.n_traffic
    plan = [("nearest", i % N, i) for i in range(max(N, N_NEAR))]
    plan += [("goal", -1, i) for i in range(4)] + [("collision", (i * 5 + 1) % N, i) for i in range(4)]
    plan += [("timeout", -1, i) for i in range(3)] + [("receding", -1, i) for i in range(4)]
    plan += [("first_goal", -1, 0), ("first_collision", N - 1, 0)]
    if exact_scenes_hold(cfg):
        plan += [(fam, (0, N - 1)[i], i) for fam in ("tie", "threshold", "twin") for i in range(2)]
    plan += [("nan", (N - 1, 0)[i], i) for i in range(2)]
    return plan


def _scene(cfg, fam, slot, variant, rng):
    N = cfg.n_traffic
    gx, gy = (float(c) for c in cfg.goal)
    v, s = float(cfg.airspeed), step_len(cfg)
    cd, R, sd = 2.0 * cfg.collision_radius, float(cfg.goal_radius), float(cfg.safe_distance)
    y, psi = gy + rng.uniform(-20.0, 20.0), rng.uniform(-2.0, 2.0) % 360.0
    side = 1.0 if variant % 2 else -1.0
    if fam == "timeout":
        x = gx - R - s * (cfg.max_steps + 30) - rng.uniform(0.0, 50.0)
    elif fam in ("collision", "first_collision"):
        x = gx - R - 60.0 * s                           # the goal is out of reach before the intruder arrives
    elif fam in ("tie", "threshold", "twin"):
        # exactly representable rows: integer x and y, heading 0; the goal follows 24 .. 70 steps later
        x, y, psi = gx - R - s * rng.integers(24, 71) - s / 2, gy, 0.0
    elif fam == "first_goal":
        x, y, psi = gx - R - s / 2, gy, 0.0             # the first step ends s / 2 inside the goal radius
    else:
        # flown straight, step n = 5 .. 16 ends s / 2 inside the goal radius and step n - 1 s / 2 outside: in so few steps no
        # action sequence moves the crossing by more than 0.3 steps
        n, c, sn = int(rng.integers(5, 17)), math.cos(math.radians(psi)), math.sin(math.radians(psi))
        x = gx - n * s * c - math.sqrt((R - s / 2) ** 2 - (gy - y - n * s * sn) ** 2)
    trf = []
    for _ in range(N):                                   # everything not placed: 500 .. 800 px away, flying radially away
        th, r = rng.uniform(30.0, 330.0), rng.uniform(500.0, 800.0)
        trf.append([x + r * math.cos(math.radians(th)), y + r * math.sin(math.radians(th)),
                    (th + rng.uniform(-10.0, 10.0)) % 360.0, v])
    if fam == "nearest":
        # alongside, between collision and safe distance, off parallel by up to 25 degrees (15 .. 25 by default; at most
        # what closes a fifth of the band in 16 steps): diverging (minimum on row 1) or converging (minimum on the last
        # row) faster than a turning player bends the curve; well ahead or behind so that traffic-after-the-move shows
        conv = 1.0 if (variant // 2) % 2 else -1.0
        ahead = 1.0 if (variant // 4) % 2 else -1.0
        angle = min(25.0, 2.0 * math.degrees(math.asin(0.2 * (sd - cd) / (32.0 * s)))) * rng.uniform(0.6, 1.0)
        trf[slot] = [x + ahead * rng.uniform(0.25, 0.45) * sd, y + side * (cd + rng.uniform(0.3, 0.4) * (sd - cd)),
                     (side * conv * angle) % 360.0, v]
    elif fam == "collision":
        trf[slot] = [x + cd + rng.uniform(3.0, 20.0) * s, y + rng.uniform(-5.0, 5.0), 180.0 + rng.uniform(-3.0, 3.0), v]
    elif fam == "first_collision":
        psi = 0.0
        trf[slot] = [x + cd + 1.5 * s, y, 180.0, v]       # both move s: s / 2 inside the collision distance after row 1
    elif fam in ("tie", "threshold", "twin"):
        ahead = {"tie": 20.5, "threshold": 20.0, "twin": 20.0}[fam]
        dy = {"tie": sd + 7.0, "threshold": sd, "twin": sd - 2.0 ** -10}[fam]
        trf[slot] = [x + s + (s / 2) * ahead, y + side * dy, 0.0, v / 2]
    elif fam == "nan":
        psi = 1.5
        trf[slot][2:] = [psi, v]                          # exact parallel flight: d_cpa is NaN in the first observation
    return [x, y, psi, v], trf


def _draw(cfg, plan, seed, attempt, only=None):
    E, N = len(plan), cfg.n_traffic
    own, trf = np.zeros((E, 4)), np.zeros((E, N, 4))
    for i, (fam, slot, variant) in enumerate(plan):
        if only is None or only[i]:
            own[i], trf[i] = _scene(cfg, fam, slot, variant, np.random.default_rng([seed, N, i, attempt]))
    return f32(own), f32(trf)


_SCENES = {}


def scenes(cfg, O, seed=0):
    """One env per entry of _plan(): 89 at every N <= 64, a full wave of a thread-per-env launch and a partial one.
      nearest         for every slot j (several times at small N): aircraft j alongside the player between collision and
                      safe distance, never colliding; all others >= 500 px away and receding
      goal / receding a goal episode with far, receding traffic only: the minimum separation is on row 1
      collision       aircraft `slot` head-on: the minimum is on the last row
      timeout         the goal out of reach within max_steps
      first_goal / first_collision   done on the first step row (steps == 2), s / 2 inside the threshold
      tie             (b = 0 only) player at integer x, heading 0; aircraft `slot` at heading 0, half the airspeed,
                      x + s + 20.5 s/2, y +- (safe_distance + 7): rows 21 and 22 tie exactly, row 21 must win
      threshold       the same with x + s + 20 s/2 and y +- safe_distance: d_sep == safe_distance on row 21, los_steps 0
      twin            the threshold scene 2^-10 closer in y: los_steps 1
      nan             aircraft `slot` in exact parallel flight: NaN d_cpa, hence a NaN action from any policy
    tie / threshold / twin are left out where the step length, or half of it, is not exact in float32
    (exact_scenes_hold()).  Every scene keeps |d_goal - goal_radius| and |d - collision distance| (both after the move, as
    is_done() takes them) at least MARGIN step lengths away on every row, under the constant actions 0, 0.375, -1 and +1:
    scenes that do not are drawn again (the crossing of a threshold s px per step wide cannot be kept 1 px away in
    general: s / 2 is the most a straight flight allows)."""
    key = (cfg, seed)
    if key not in _SCENES:
        import helpers as H
        plan = _plan(cfg)
        E = len(plan)
        goal = np.tile(np.asarray(cfg.goal, np.float64), (E, 1))
        fam, slot = np.array([p[0] for p in plan]), np.array([p[1] for p in plan])
        own, trf = _draw(cfg, plan, seed, 0)
        bad = np.ones(E, bool)
        for attempt in range(1, 400):                                    # (only the scenes drawn anew are flown again)
            sub = Scenes(own[bad], trf[bad], goal[bad], fam[bad], slot[bad])
            margin = np.full(int(bad.sum()), np.inf)
            for a in (0.0, 0.375, -1.0, 1.0):
                margin = np.fmin(margin, run(O, H, cfg, sub, constant_actions(sub, a, cfg.max_steps + 1)).margin)
            bad[bad] = margin < MARGIN * step_len(cfg)
            if not bad.any():
                break
            o2, t2 = _draw(cfg, plan, seed, attempt, only=bad)
            own[bad], trf[bad] = o2[bad], t2[bad]
        else:
            raise AssertionError("no scene with the margin after 400 draws: %s" % fam[bad])
        sc = Scenes(own, trf, goal, fam, slot)
        for a in sc:
            a.setflags(write=False)
        _SCENES[key] = sc
    return _SCENES[key]


# ---- actions ------------------------------------------------------------------------------------------------------------
def constant_actions(sc, bias, T):
    """What a constant-action policy plays: clip(bias, -1, 1) on finite observations, NaN from the first step on in the
    `nan` scenes (their first observation holds a NaN, and a NaN action makes every later one NaN)."""
    a = np.full((T, len(sc.family)), float(np.clip(bias, -1.0, 1.0)))
    a[:, sc.family == "nan"] = np.nan
    return a


def walk_actions(sc, T, seed=5):
    """The CPU stand-in for the random policy: a clipped, seeded random walk, float32-representable."""
    rng = np.random.default_rng(seed)
    E = len(sc.family)
    a = f32(np.clip(rng.uniform(-1, 1, E) + np.cumsum(rng.normal(0.0, 0.25, (T, E)), 0), -1.0, 1.0))
    a[:, sc.family == "nan"] = np.nan
    return a


def cpu_actions(sc, T):
    return np.stack([constant_actions(sc, b, T) for b in CONST_BIAS] + [walk_actions(sc, T)])


def policies(g, N):
    """The K ActorCritics: the three constant ones and the random one (head x 40, as eval_stats_support.two_policies)."""
    import torch
    pols = []
    for i, b in enumerate(CONST_BIAS + (None,)):
        torch.manual_seed(11 + i)
        pol = g.ActorCritic(5 + 3 * N)
        with torch.no_grad():
            if b is None:
                pol.action_net.weight.mul_(40.0)
            else:
                pol.action_net.weight.zero_()
                pol.action_net.bias.fill_(b)
        pols.append(pol)
    return pols


# ---- the reference ------------------------------------------------------------------------------------------------------
def run(O, H, cfg, sc, actions, rounding=None, traffic="before"):
    """The oracle over `actions` [T, E] from the scenes: Rows of [E] / [T + 1, E] arrays (row 0 is the dummy row; rows
    after an env's first done hold NaN).  rounding: applied to the state after every step (the float32 drift probe).
    traffic="after": the deliberately wrong d_sep, from the traffic after its move.  margin: the least distance of
    d_goal from the goal radius and of any aircraft from the collision distance, after the move, over the env's rows;
    extent: the largest |coordinate| met."""
    T, E = actions.shape
    N = cfg.n_traffic
    env = O.OracleEnvs(E, N, auto_reset=False, config=H.oracle_config(O, cfg))
    env.set_state(sc.own, sc.trf, sc.goal)
    env.observe()
    d_sep, a_lat, d_dev = (np.full((T + 1, E), np.nan) for _ in range(3))
    outcome, steps = np.zeros(E, np.uint8), np.zeros(E, np.int32)
    margin, active, extent = np.full(E, np.inf), np.ones(E, bool), 0.0
    R, cd = float(cfg.goal_radius), 2.0 * cfg.collision_radius
    for t in range(T):
        tx, ty = env.trf_x.copy(), env.trf_y.copy()
        obs, _, done, oc, _ = env.step(actions[t])
        if traffic == "after":
            tx, ty = env.trf_x, env.trf_y
        d = np.hypot(env.own_x[:, None] - tx, env.own_y[:, None] - ty)
        d_sep[t + 1, active] = np.where(np.isnan(d), np.inf, d).min(1)[active]
        a_lat[t + 1, active] = (actions[t] * float(cfg.acc_lat_limit))[active]
        d_dev[t + 1, active] = (obs[:, 2] * env.cfg.d_dev_max)[active]
        after = np.hypot(env.own_x[:, None] - env.trf_x, env.own_y[:, None] - env.trf_y)
        m = np.minimum(np.abs(np.hypot(env.own_x - env.goal_x, env.own_y - env.goal_y) - R), np.abs(after - cd).min(1))
        margin[active] = np.fmin(margin, m)[active]
        for a in (env.own_x, env.own_y, env.trf_x, env.trf_y):
            if np.isfinite(a[active]).any():
                extent = max(extent, float(np.nanmax(np.abs(a[active]))))
        fin = active & (done != 0)
        outcome[fin], steps[fin] = oc[fin], env.steps[fin]
        active &= ~fin
        if not active.any():
            break
        if rounding is not None:
            for a in (env.own_x, env.own_y, env.own_psi, env.trf_x, env.trf_y, env.trf_psi):
                a[:] = rounding(a)
    margin[np.isinf(margin)] = np.nan                                    # (a NaN player has no margin)
    return Rows(outcome, steps, d_sep, a_lat, d_dev, margin, extent)


def reduce_rows(g, cfg, rows):
    """records.episode_safety / safety_summary in float64 per env: dict of [E] arrays under SAFETY_KEYS (zeros where the
    episode did not finish)."""
    E = len(rows.steps)
    out = {k: np.zeros(E, np.int32 if k in ("min_separation_step", "los_steps") else np.float64) for k in g.records.SAFETY_KEYS}
    for i in np.nonzero(rows.outcome)[0]:
        n = int(rows.steps[i])                                            # row 0 and steps - 1 step rows
        one = g.records.episode_safety(rows.d_sep[:n, i], rows.a_lat[:n, i], rows.d_dev[:n, i], cfg.safe_distance, np.float64)
        for k, val in g.records.safety_summary(one, n).items():
            out[k][i] = val
    return out


def reference(O, H, g, cfg, sc, actions):
    """The reference of K action streams `actions` [K, T, E] (float64 values representable in the dtype under test)."""
    runs = [run(O, H, cfg, sc, a) for a in actions]
    stats = [reduce_rows(g, cfg, r) for r in runs]
    stack = lambda name: np.stack([getattr(r, name) for r in runs])  # noqa: E731
    ref = Reference(stack("outcome"), stack("steps"), stack("d_sep"), stack("a_lat"), stack("d_dev"),
                    {k: np.stack([s[k] for s in stats]) for k in stats[0]}, stack("margin"),
                    max(r.extent for r in runs), np.array(actions))
    for a in (*ref[:5], *ref.stats.values(), ref.margin, ref.actions):
        a.setflags(write=False)
    return ref


def drift(O, H, cfg, sc, actions, ref):
    """D: the oracle with its state rounded to float32 after every step against the plain one, the largest difference in
    d_sep and in |d_dev| over the rows both have."""
    D = 0.0
    for k, a in enumerate(actions):
        r = run(O, H, cfg, sc, a, rounding=f32)
        for x, y in ((r.d_sep, ref.d_sep[k]), (np.abs(r.d_dev), np.abs(ref.d_dev[k]))):
            both = np.isfinite(x) & np.isfinite(y)
            D = max(D, float(np.abs(x[both] - y[both]).max()))
    return D


def bound(H, build, rows, extent=None, D=None):
    """B in px for build "float32" / "float64" / "float64fast" (module docstring)."""
    if build == "float64":
        return 1e-9
    if build == "float64fast":
        return rows * 1e-11
    return max(4.0 * D, rows * H.f32_pos_bound(extent))


# ---- the criteria -------------------------------------------------------------------------------------------------------
def step_rows(ref):
    """[K, T + 1, E] mask of each episode's step rows 1 .. steps - 1."""
    r = np.arange(ref.d_sep.shape[1])[None, :, None]
    return (r >= 1) & (r < ref.steps[:, None, :])


def candidates(ref, B):
    """[K, T + 1, E] mask: the step rows whose reference d_sep lies within 2 B of the episode's reference minimum."""
    valid = step_rows(ref) & np.isfinite(ref.d_sep)
    return valid & (ref.d_sep <= ref.stats["min_separation"][:, None, :] + 2 * B)


def los_range(ref, B, safe_distance):
    d = np.where(step_rows(ref) & np.isfinite(ref.d_sep), ref.d_sep, np.inf)
    return (d < safe_distance - B).sum(1), (d < safe_distance + B).sum(1)


def decided(ref, B, safe_distance):
    """(unique, same) [K, E]: episodes whose min_separation_step / los_steps the criteria pin to one value."""
    lo, hi = los_range(ref, B, safe_distance)
    return candidates(ref, B).sum(1) == 1, lo == hi


def expected_max_a_lat(ref, cfg, npdt):
    """max |T(action) * T(acc_lat_limit)| over the step rows in the build's dtype, from 0, a NaN never taken."""
    a = np.abs(ref.actions.astype(npdt) * npdt(cfg.acc_lat_limit))             # [K, T, E]: row t + 1 is action t
    a = np.where(step_rows(ref)[:, 1:], a, npdt(0))
    return np.fmax.reduce(a, 1, initial=npdt(0)).astype(npdt)


def compare(got, ref, cfg, B, npdt):
    """Every assertion of the comparison with the reference; returns the worst errors and the counts of episodes decided by
    equality.  `got`: evaluate_policies_fused(safety=True)'s dict ([K, E] arrays)."""
    assert np.array_equal(got["outcome"], ref.outcome), np.argwhere(got["outcome"] != ref.outcome)
    assert np.array_equal(got["steps"], ref.steps), np.argwhere(got["steps"] != ref.steps)
    assert (ref.outcome != 0).all()
    s, eps = ref.stats, float(np.finfo(npdt).eps)
    want = expected_max_a_lat(ref, cfg, npdt)
    assert got["max_abs_a_lat"].dtype == want.dtype and np.array_equal(got["max_abs_a_lat"].view(np.uint8), want.view(np.uint8))
    err = {}
    for key in ("min_separation", "max_abs_deviation", "mean_abs_deviation"):
        x, y = got[key].astype(np.float64), s[key]
        same = (np.isnan(x) & np.isnan(y)) | (x == y)                          # NaN and +inf compare exactly
        fin = np.isfinite(x) & np.isfinite(y)
        assert (same | fin).all(), (key, np.argwhere(~(same | fin)))
        x, y = np.where(fin, x, 0.0), np.where(fin, y, 0.0)
        tol = B + ((ref.steps - 1) * eps * np.abs(y) if key == "mean_abs_deviation" else 0.0)
        d = np.abs(x - y)
        err[key] = float(d.max())
        assert (d <= tol).all(), (key, err[key], B, np.argwhere(d > tol))
    cand = candidates(ref, B)
    row = got["min_separation_step"]
    none = ~cand.any(1)                                                        # no finite row: the index stays 0
    k, e = np.indices(row.shape)
    assert ((row >= 0) & (row < cand.shape[1])).all()
    assert np.where(none, row == 0, cand[k, np.clip(row, 0, cand.shape[1] - 1), e]).all(), \
        np.argwhere(~np.where(none, row == 0, cand[k, np.clip(row, 0, cand.shape[1] - 1), e]))
    lo, hi = los_range(ref, B, float(cfg.safe_distance))
    assert ((got["los_steps"] >= lo) & (got["los_steps"] <= hi)).all(), np.argwhere((got["los_steps"] < lo) | (got["los_steps"] > hi))
    unique, same = decided(ref, B, float(cfg.safe_distance))
    err.update(unique=int(unique.sum()), same_los=int(same.sum()), episodes=int(row.size))
    return err


def assert_exact_scenes(got, sc, cfg, npdt):
    """tie / threshold / twin under the b = 0 policy (row 0 of the launch) and nan under every policy: exactly."""
    fam, sd = sc.family, npdt(cfg.safe_distance)
    z = got["min_separation_step"][0]
    if exact_scenes_hold(cfg):
        for f in ("tie", "threshold", "twin"):
            assert (fam == f).sum() == 2
            assert (z[fam == f] == TIE_ROW).all(), (f, z[fam == f])
            assert (got["max_abs_a_lat"][0][fam == f] == 0).all() and (got["max_abs_deviation"][0][fam == f] == 0).all()
        assert (got["los_steps"][0][np.isin(fam, ("tie", "threshold"))] == 0).all()
        assert (got["los_steps"][0][fam == "twin"] == 1).all()
        m = got["min_separation"][0][fam == "threshold"]
        assert m.dtype == np.dtype(npdt) and (m == sd).all(), m
        assert (got["min_separation"][0][fam == "twin"] < sd).all()
    nan = fam == "nan"
    assert nan.sum() == 2
    for k in range(got["outcome"].shape[0]):
        assert (got["outcome"][k][nan] == 3).all() and (got["steps"][k][nan] == cfg.max_steps + 1).all()
        assert np.isposinf(got["min_separation"][k][nan]).all()
        for key in ("min_separation_step", "los_steps", "max_abs_a_lat", "max_abs_deviation"):
            assert (got[key][k][nan] == 0).all(), (key, got[key][k][nan])
        assert np.isnan(got["mean_abs_deviation"][k][nan]).all()
