"""Hand-placed edge states for every work shape: the batch of tests/test_gpu_edge_states.py, checked against the CPU
oracle by tests/test_edge_states.py.

edge_cases(N, cfg, seed) lists single-step cases that each hit one edge of the game at a chosen traffic slot, every
threshold placed relative to `cfg` (an OracleConfig: collision_dist, goal_radius, max_steps, goal, dt, speeds), so the
same families run under helpers.NONDEFAULT_CONFIGS.  Families (oracle/refharness/capture_golden.py edge_cases widened
to every slot):

  collision   traffic `slot` alone ends the step at collision_dist + offset, crossing in; every other aircraft stays
              >= 300 px away.  |offset| >= 1e-8 is decided exactly; 0 and +-1e-10 lie inside the 1e-9 band.
  parallel    traffic `slot` alone flies the player's heading and speed: the reference's relative velocity is 0 / 0, so
              d_cpa (column 5 + 3 slot + 1) is NaN (kinematics.py:48).  The reward stays finite: the closing speed is 0,
              and min(1, nan ** 4) is 1 (rewards.py:16) -- also at slot 0, where the reward reads that d_cpa.
  parallel+timeout  the same on the last step of the episode: the NaN reaches the terminal observation.
  mirror      traffic `slot` flies the mirror-image heading (360 - psi) at the player's speed: v12x is an exact 0 or
              +-1 ulp, a coin toss of cos that decides the SIGN of d_cpa (test_f64_edge_vectors).
  injected    traffic `slot` starts from an injected heading (INJECTED_HEADINGS) that the step wraps.
  goal        the player ends the step at goal_radius + offset from the goal (offsets as for collisions).
  goal+collision  inside the goal radius and colliding with the last slot in the same step.
  timeout     steps max_steps - 2 .. max_steps + 1 before the step, alone, with a goal, with a collision (last slot),
              with both (is_done(): timeout > collision > goal, game.py:294-314).
  own-wrap    the player's heading across 0 / 360 with saturated actions, injected 360, a hair below 0 and 719.
  off-plan    far off the planned path (|d_dev| > rw_d_dev_max), behind the start.
  speeds      player and traffic at speeds other than the configuration's (the v_1 quirk of kinematics.py:74).

edge_batch() lays the cases out for the kernels: each case at the first env of a wave and at the last env of a wave of
every work shape of N (helpers.SHAPES), calm filler envs between them, the batch padded to whole eight-workgroup groups
of the float32 packed shapes (the consecutive-layout "arena" kernel's sizes), and a partial last wave of 17 envs behind
that which repeats the first and the last case of every family (the general kernel's sizes).
"""
import math
from collections import namedtuple

import numpy as np

import helpers as H

# offsets of the collision / goal placements: decided exactly, and inside the float64 1e-9 band
EXACT_OFFSETS = (-1e-8, 1e-8, -1e-2, 1e-2, -5.0, 5.0)
BAND_OFFSETS = (0.0, -1e-10, 1e-10)
OFFSETS = EXACT_OFFSETS + BAND_OFFSETS
F64_BAND = 1e-9
F32_BAND = 1e-3             # _check_f32_step_vs_oracle's band around the thresholds
# injected traffic headings: 360, the largest float64 and float32 values below 360, -0.0, a hair below 0 (-2^-40:
# float64 wraps it to 360 - 2^-40, which rounds to 360.0f -- the float32 step's own result), 719 (the float32 window)
INJECTED_HEADINGS = (360.0, float(np.nextafter(360.0, 0.0)), float(np.nextafter(np.float32(360), np.float32(0))), -0.0,
                     -2.0 ** -40, 719.0)
TAIL = 17                   # envs of the partial last wave
MIN_SEP = 300.0             # every aircraft not placed on purpose

Case = namedtuple("Case", "family slot offset own trf goal steps action coll_slot coll_off goal_off nan_slot mirror_slot")


def rad(deg):
    """(deg / 360.0) * 2 * math.pi, as aircraft.py:23 evaluates it."""
    return ((deg / 360.0) * 2.0) * math.pi


def py_mod360(a):
    return float(np.mod(a, 360.0)) if a != 0 else 0.0


def wave_unit(N):
    """The largest number of envs per wave among the work shapes of N: a multiple of it starts a wave of every shape."""
    return max(s.envs_per_wave for s in H.SHAPES if s.n_traffic == N)


def arena_unit(N):
    """Whole eight-workgroup groups (4 waves each) of every float32 packed shape of N (1: none is packed)."""
    eps = [s.envs_per_wave for s in H.SHAPES if s.n_traffic == N and s.dtype == "float32" and s.packed]
    return 32 * max(eps) if eps else 1


def _post_own(cfg, own, action):
    """The player after aircraft.py:16-26 (float64, the oracle's operation order)."""
    x, y, psi, v = own
    psi2 = py_mod360(psi + ((action * cfg.acc_lat_limit) / (v * cfg.dt)) * cfg.dt)
    return x + (v * math.cos(rad(psi2))) * cfg.dt, y + (v * math.sin(rad(psi2))) * cfg.dt, psi2


def _pre_traffic(cfg, px, py, psi, v):
    """The traffic state that ends the step (straight flight) at (px, py)."""
    return [px - (v * math.cos(rad(psi))) * cfg.dt, py - (v * math.sin(rad(psi))) * cfg.dt, psi, v]


class _Gen:
    def __init__(self, N, cfg, seed):
        self.N, self.cfg = N, cfg
        self.rng = np.random.default_rng(seed)
        self.v = float(cfg.own_v)
        self.goal = (float(cfg.goal_x), float(cfg.goal_y))
        self.span = self.goal[0] - float(cfg.own_x0)

    def heading_apart(self, psi):
        """A traffic heading at least 5 degrees from psi and from its mirror image (no parallel / near-0 v12x)."""
        while True:
            h = float(self.rng.uniform(0, 360))
            if all(min(abs(h - p) % 360, 360 - abs(h - p) % 360) > 5 for p in (psi, 360 - psi)):
                return h

    def calm_own(self):
        """Mid-plan, heading roughly to the goal, far from the goal radius."""
        gx, gy = self.goal
        x = float(self.cfg.own_x0) + self.span * self.rng.uniform(0.2, 0.6)
        y = gy + self.rng.uniform(-0.2, 0.2) * float(self.cfg.rw_d_dev_max)
        return [x, y, float(self.rng.uniform(-20, 20)) % 360, self.v]

    def calm_steps(self):
        return int(self.rng.integers(1, max(2, self.cfg.max_steps - 10)))

    def far_traffic(self, cx, cy, psi_own, n):
        """n aircraft on a ring 300 .. 600 px around (cx, cy) -- post-step distance >= MIN_SEP -- none parallel."""
        out = []
        for _ in range(n):
            r, a = self.rng.uniform(MIN_SEP + 10, 2 * MIN_SEP), self.rng.uniform(0, 2 * math.pi)
            h = self.heading_apart(psi_own)
            out.append(_pre_traffic(self.cfg, cx + r * math.cos(a), cy + r * math.sin(a), h, self.v))
        return out

    def ring_except(self, own, action, placed):
        """A traffic block: far aircraft everywhere, `placed` {slot: state} on top."""
        px, py, psi = _post_own(self.cfg, own, action)
        trf = self.far_traffic(px, py, psi, self.N)
        for j, t in placed.items():
            trf[j] = t
        return trf

    def at_distance(self, own, action, d, psi_t=None, v_t=None):
        """A traffic aircraft that ends the step d px from the player, crossing in."""
        px, py, psi = _post_own(self.cfg, own, action)
        a = self.rng.uniform(0, 2 * math.pi)
        h = self.heading_apart(psi) if psi_t is None else psi_t
        return _pre_traffic(self.cfg, px + d * math.cos(a), py + d * math.sin(a), h, self.v if v_t is None else v_t)

    def at_goal(self, d, psi=None):
        """A player state that ends the step (action 0) d px from the goal, flying at it."""
        gx, gy = self.goal
        th = float(self.rng.uniform(-30, 30)) if psi is None else psi
        px, py = gx - d * math.cos(rad(th)), gy - d * math.sin(rad(th))
        return [px - (self.v * math.cos(rad(th))) * self.cfg.dt, py - (self.v * math.sin(rad(th))) * self.cfg.dt, th % 360, self.v]


def edge_cases(N, cfg, seed=0):
    """The list of Case tuples for N traffic under the OracleConfig `cfg` (see the module docstring)."""
    G = _Gen(N, cfg, seed)
    cd, R, M = float(cfg.collision_dist), float(cfg.goal_radius), int(cfg.max_steps)
    cases = []

    def add(family, slot, offset, own, trf, steps, action, coll_slot=-1, coll_off=np.nan, goal_off=np.nan, nan_slot=-1,
            mirror_slot=-1):
        assert len(trf) == N
        cases.append(Case(family, slot, offset, list(map(float, own)), [list(map(float, t)) for t in trf],
                          list(G.goal), int(steps), float(action), coll_slot, coll_off, goal_off, nan_slot, mirror_slot))

    for j in range(N):
        for off in OFFSETS:
            own = G.calm_own()
            add("collision", j, off, own, G.ring_except(own, 0.0, {j: G.at_distance(own, 0.0, cd + off)}), G.calm_steps(), 0.0,
                coll_slot=j, coll_off=off)
        own = G.calm_own()
        par = G.at_distance(own, 0.0, float(G.rng.uniform(2 * cd, MIN_SEP)), psi_t=own[2], v_t=own[3])
        add("parallel", j, np.nan, own, G.ring_except(own, 0.0, {j: par}), G.calm_steps(), 0.0, nan_slot=j)
        own = G.calm_own()
        mir = G.at_distance(own, 0.0, float(G.rng.uniform(2 * cd, MIN_SEP)), psi_t=(360.0 - own[2]) % 360, v_t=own[3])
        add("mirror", j, np.nan, own, G.ring_except(own, 0.0, {j: mir}), G.calm_steps(), 0.0, mirror_slot=j)
        for h in INJECTED_HEADINGS:
            own = G.calm_own()
            own[2] = 37.0                # clear of every wrapped value and its mirror image
            trf = G.ring_except(own, 0.0, {})
            trf[j][2] = h
            add("injected", j, h, own, trf, G.calm_steps(), float(G.rng.uniform(-1, 1)))
    for j in sorted({0, N - 1}):
        own = G.calm_own()
        par = G.at_distance(own, 0.0, float(G.rng.uniform(2 * cd, MIN_SEP)), psi_t=own[2], v_t=own[3])
        add("parallel+timeout", j, np.nan, own, G.ring_except(own, 0.0, {j: par}), M, 0.0, nan_slot=j)
    for off in OFFSETS:
        own = G.at_goal(R + off)
        add("goal", -1, off, own, G.ring_except(own, 0.0, {}), G.calm_steps(), 0.0, goal_off=off)
    own = G.at_goal(R - 4.0)
    add("goal+collision", N - 1, -4.0, own, G.ring_except(own, 0.0, {N - 1: G.at_distance(own, 0.0, cd - 4.0)}),
        G.calm_steps(), 0.0, coll_slot=N - 1, coll_off=-4.0, goal_off=-4.0)
    for s in range(M - 2, M + 2):
        for goal in (False, True):
            for coll in (False, True):
                own = G.at_goal(R - 4.0) if goal else G.calm_own()
                placed = {N - 1: G.at_distance(own, 0.0, cd - 4.0)} if coll else {}
                add("timeout", N - 1 if coll else -1, float(s), own, G.ring_except(own, 0.0, placed), s, 0.0,
                    coll_slot=N - 1 if coll else -1, coll_off=-4.0 if coll else np.nan, goal_off=-4.0 if goal else np.nan)
    for psi, a in ((0.2, -1.0), (359.8, 1.0), (0.0, -1.0), (0.0, 1.0), (360.0, 0.0), (359.99999999, 1.0), (-2.0 ** -40, 0.0),
                   (-2.0 ** -40, -1.0), (719.0, 0.3), (180.0, 1.0), (90.0, -1.0), (270.0, 0.5)):
        own = G.calm_own()
        own[2] = psi
        add("own-wrap", -1, psi, own, G.ring_except(own, a, {}), G.calm_steps(), a)
    gx, gy = G.goal
    dev = 1.3 * float(cfg.rw_d_dev_max)
    for own in ([gx - 0.5 * G.span, gy + dev, 300.0, G.v], [gx - 0.5 * G.span, gy - dev, 60.0, G.v],
                [float(cfg.own_x0) - 0.1 * G.span, gy + 20.0, 180.0, G.v]):
        add("off-plan", -1, np.nan, own, G.ring_except(own, 0.1, {}), G.calm_steps(), 0.1)
    for fo, ft in ((1.0, 1.3), (0.9, 0.7), (1.2, 1.0)):
        own = G.calm_own()
        own[3] = fo * G.v
        t = G.at_distance(own, 0.25, float(G.rng.uniform(2 * cd, MIN_SEP)), v_t=ft * G.v)
        add("speeds", 0, ft, own, G.ring_except(own, 0.25, {0: t}), G.calm_steps(), 0.25)
    return cases


Batch = namedtuple("Batch", "N own trf goal steps action case whole cases")


def _tail_cases(cases):
    """TAIL cases: the first case of every family, then the last ones (the last slot) of as many as fit."""
    first, last = {}, {}
    for i, c in enumerate(cases):
        first.setdefault(c.family, i)
        last[c.family] = i
    pick = list(first.values())
    for i in last.values():
        if len(pick) < TAIL and i not in pick:
            pick.append(i)
    return pick + [pick[k % len(pick)] for k in range(TAIL - len(pick))]


def edge_batch(N, cfg, seed=0):
    """The edge cases of edge_cases(N, cfg, seed) as one batch: own [E, 4], trf [E, N, 4], goal [E, 2], steps [E],
    action [E], case [E] (the index into `cases`, -1 for a filler env).  Envs 0 .. whole - 1 are whole eight-workgroup
    groups of every float32 packed shape of N; the TAIL envs behind them are a partial last wave."""
    cases = edge_cases(N, cfg, seed)
    W, U = wave_unit(N), arena_unit(N)
    K = len(cases)
    main = W * K if W > 1 else K
    whole = -(-main // U) * U
    E = whole + TAIL
    case = np.full(E, -1, np.int64)
    if W > 1:
        case[np.arange(K) * W] = np.arange(K)              # the first env of a wave
        case[np.arange(K) * W + W - 1] = np.arange(K)      # the last env of a wave
    else:
        case[:K] = np.arange(K)
    case[whole:] = _tail_cases(cases)
    G = _Gen(N, cfg, seed + 1)
    own = np.zeros((E, 4))
    trf = np.zeros((E, N, 4))
    goal = np.tile(np.array(G.goal), (E, 1))
    steps = np.zeros(E, np.int32)
    action = np.zeros(E)
    for e in range(E):
        if case[e] >= 0:
            c = cases[case[e]]
            own[e], trf[e], goal[e], steps[e], action[e] = c.own, c.trf, c.goal, c.steps, c.action
        else:                                              # calm mid-episode filler
            o = G.calm_own()
            a = float(G.rng.uniform(-1, 1))
            own[e], trf[e], steps[e], action[e] = o, G.ring_except(o, a, {}), G.calm_steps(), a
    return Batch(N, own, trf, goal, steps, action, case, whole, cases)


def labels(batch, field):
    """Per-env value of a Case field (NaN / -1 / None for filler envs)."""
    fill = {"family": None, "slot": -1, "coll_slot": -1, "nan_slot": -1, "mirror_slot": -1}.get(field, np.nan)
    vals = [fill if k < 0 else getattr(batch.cases[k], field) for k in batch.case]
    return np.array(vals, dtype=object if field == "family" else None)


def placed_in_band(batch, band):
    """Envs whose placed collision / goal offset lies within `band` of its threshold."""
    co, go = labels(batch, "coll_off").astype(float), labels(batch, "goal_off").astype(float)
    with np.errstate(invalid="ignore"):
        return (np.abs(co) < band) | (np.abs(go) < band)


def expected_nan_columns(batch):
    """Bool [E, 5 + 3N]: where the observation holds NaN (slot j's d_cpa of the parallel-flight cases)."""
    E, N = len(batch.case), batch.N
    want = np.zeros((E, 5 + 3 * N), bool)
    j = labels(batch, "nan_slot").astype(int)
    rows = np.nonzero(j >= 0)[0]
    want[rows, 5 + 3 * j[rows] + 1] = True
    return want


def post_step_geometry(O, batch, config=None, rounding=None):
    """The latching oracle stepped once on the batch (inputs passed through `rounding`, e.g. float32): returns (d [E, N]
    traffic distances, d_goal [E]) after the step -- what game.py:185-192 compares with the thresholds -- and the oracle."""
    f = (lambda a: a) if rounding is None else rounding
    E, N = len(batch.case), batch.N
    ref = O.OracleEnvs(E, N, config=config)
    ref.set_state(f(batch.own), f(batch.trf), f(batch.goal), batch.steps)
    ref.step(f(batch.action))
    d = np.sqrt((ref.trf_x - ref.own_x[:, None]) ** 2 + (ref.trf_y - ref.own_y[:, None]) ** 2)
    d_goal = np.sqrt((ref.goal_x - ref.own_x) ** 2 + (ref.goal_y - ref.own_y) ** 2)
    return d, d_goal, ref


def in_band(cfg, d, d_goal, band):
    return (np.abs(d - cfg.collision_dist) < band).any(1) | (np.abs(d_goal - cfg.goal_radius) < band)
