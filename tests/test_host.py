"""CPU tests (-m "not gpu") of the host side: config vs the reference's constants, the host
parity reset, the C-ABI library (loads, exports every declared symbol, validates arguments --
no compute without a GPU), spaces, sharding arithmetic, and the no-fallback rule."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g():
    import gym_acas2d_amd as g
    return g


def test_config_matches_reference_constants(g, oracle_mod):
    c = g.ACAS2DConfig()
    assert (c.max_steps, c.width, c.height, c.fps) == (1000, 1600, 1000, 100)        # settings.py:9,15-17
    assert (c.aircraft_size, c.collision_radius, c.goal_radius, c.safe_distance) == (24, 48, 144, 192)
    assert c.acc_lat_limit == pytest.approx(196.133) and c.airspeed == 200
    cc = c.to_c()
    assert cc.d_goal_max == 3408 and cc.d_dev_max == 2000 and cc.v_closing_max == 400
    assert cc.d_sep_max == pytest.approx(5886.796, abs=1e-3) and cc.d_cpa_max == pytest.approx(1886.796, abs=1e-3)
    assert cc.rw_d_goal_max == 3408 and cc.rw_d_dev_max == 704 and cc.collision_dist == 96
    # field-for-field against the oracle's independent restatement of settings.py
    oc = oracle_mod.default_config()
    for name, _ in oracle_mod.OracleConfig._fields_:
        if name != "_pad":
            assert getattr(cc, name) == getattr(oc, name), name
    assert c.obs_dim == 8 and g.ACAS2DConfig(n_traffic=8).obs_dim == 29
    lo, hi = g.ACAS2DConfig(n_traffic=2).obs_low_high()                                # environment.py:19-20
    assert lo == [0, 0, -1, 0, 0, 0, -1, -1, 0, -1, -1] and hi == [1] * 11
    with pytest.raises(ValueError):
        g.ACAS2DConfig(n_traffic=0)
    assert g.ACAS2DConfig.algorithmic_bytes_per_env_step(8, 4) == 361
    assert g.ACAS2DConfig.algorithmic_bytes_per_env_step(3, 4) == 181
    assert g.ACAS2DConfig.algorithmic_bytes_per_env_step(64, 8) == 4745


def test_parity_reset_reproduces_reference_draws(g):
    """random.seed(13) -> 2nd game is (48, 500, psi=358.1242450086868),
    traffic (1552, 48, 136.41722591475224); also the captured initial states for N = 1..64."""
    cfg = g.ACAS2DConfig()
    rng = random.Random(13)
    g.reset_parity.draw_episode(cfg, rng)
    own, trf, goal = g.reset_parity.draw_episode(cfg, rng)
    assert list(own) == [48, 500.0, 358.1242450086868, 200]
    assert list(trf[0]) == [1552, 48, 136.41722591475224, 200.0]
    assert list(goal) == [1456, 500.0]
    for N in (1, 3, 8, 64):
        fx = H.load("ref_rollout_n%d.npz" % N)
        o, t, gl = H.parity_reset_states(g.ACAS2DConfig(n_traffic=N), int(fx["seed_py"]), 1, len(fx["ep_own"]))
        assert np.array_equal(o, fx["ep_own"]) and np.array_equal(t, fx["ep_trf"]) and np.array_equal(gl, fx["ep_goal"])
    # the module-level default draws from the global `random`, like the reference
    random.seed(13)
    g.reset_parity.draw_episode(cfg)
    own2, _, _ = g.reset_parity.draw_episode(cfg)
    assert own2[2] == 358.1242450086868


def test_c_abi_library_loads_and_exports_every_declared_symbol(g):
    header = open(os.path.join(ROOT, "include", "acas2d.h")).read()
    declared = set(re.findall(r"\b(acas2d_[a-z0-9_]+)\s*\(", header))
    assert {"acas2d_step_f32", "acas2d_step_f64", "acas2d_rollout_f32", "acas2d_rollout_f64",
            "acas2d_rollout_policy_f32", "acas2d_rollout_policy_f64",
            "acas2d_reset_f32", "acas2d_reset_f64", "acas2d_last_error", "acas2d_abi_version"} <= declared
    L = g.native.lib()
    for name in declared:
        assert hasattr(L, name), name
    assert set(g.native.EXPORTS) == declared
    assert L.acas2d_abi_version() == g.native.ABI_VERSION == 7 and L.acas2d_config_size() == C.sizeof(g.config.CConfig)
    assert int(re.search(r"#define ACAS2D_ABI_VERSION (\d+)", header).group(1)) == g.native.ABI_VERSION


def test_c_abi_argument_validation_needs_no_gpu(g):
    L = g.native.lib()
    cfg = g.ACAS2DConfig().to_c()
    st, io = g.native.CState(), g.native.CStepIO()
    assert L.acas2d_step_f32(None, C.byref(st), None, C.byref(io), 0, 0, 0, 4, 1, None) == -22
    assert b"NULL cfg" in L.acas2d_last_error()
    assert L.acas2d_step_f64(C.byref(cfg), C.byref(st), None, C.byref(io), 0, 0, 0, 4, 1, None) == -22
    assert b"state" in L.acas2d_last_error()
    dummy = (C.c_double * 4096)()
    base = C.addressof(dummy)
    full = g.native.CState(*([base] * 14))        # trace stays NULL
    assert L.acas2d_step_f64(C.byref(cfg), C.byref(full), None, C.byref(io), 0, 0, 0, 4, 1, None) == -22
    assert b"required" in L.acas2d_last_error()
    io_ok = g.native.CStepIO(*([base] * 5 + [None] * 3))
    assert L.acas2d_step_f64(C.byref(cfg), C.byref(full), None, C.byref(io_ok), 0, 0, 0, 4, 0, None) == -22
    assert b"n_traffic" in L.acas2d_last_error()
    assert L.acas2d_step_f64(C.byref(cfg), C.byref(full), None, C.byref(io_ok), 0, 0, 0, -1, 1, None) == -22
    assert L.acas2d_step_f64(C.byref(cfg), C.byref(full), None, C.byref(io_ok), 0, 0, 0, 0, 1, None) == 0   # no-op
    # state_out (double-buffered state, ABI 6): the layout contract of include/acas2d.h is checked before any launch
    E, N, AR = 4, 2, g.native.AUTO_RESET

    def gen2(**over):
        """A second generation E (per-env arrays) / E * N (traffic arrays) elements behind `full`'s, in doubles."""
        f = {n: getattr(full, n) for n, _ in g.native.CState._fields_}
        for n in ("own_x", "own_y", "own_psi", "total_reward"):
            f[n] = base + 8 * E
        f["steps"] = base + 4 * E
        f["trf_x"] = f["trf_y"] = base + 8 * E * N
        f.update(over)
        return g.native.CState(*[f[n] for n, _ in g.native.CState._fields_])

    def step(out, flags=AR):
        return L.acas2d_step_f64(C.byref(cfg), C.byref(full), None if out is None else C.byref(out), C.byref(io_ok), flags,
                                 0, 0, E, N, None)

    assert step(gen2(own_v=base + 64)) == -22 and b"must share" in L.acas2d_last_error()
    assert step(gen2(own_y=base + 8 * (E + 1))) == -22 and b"ONE element offset" in L.acas2d_last_error()
    assert step(gen2(steps=base + 8 * E)) == -22 and b"ONE element offset" in L.acas2d_last_error()
    assert step(gen2(trf_y=base + 8 * E * N + 8)) == -22 and b"ONE element offset" in L.acas2d_last_error()
    assert step(gen2(), flags=0) == -22 and b"ACAS2D_AUTO_RESET" in L.acas2d_last_error()
    near = {n: base + 8 * (E - 1) for n in ("own_x", "own_y", "own_psi", "total_reward")}
    assert step(gen2(steps=base + 4 * (E - 1), **near)) == -22 and b"overlaps" in L.acas2d_last_error()
    assert L.acas2d_reset_f32(C.byref(cfg), C.byref(st), None, None, 1, 0, 0, 4, 1, None) == -22
    assert L.acas2d_reset_f32(C.byref(cfg), C.byref(full), None, None, 1, 0, 0, 0, 1, None) == 0
    reset = lambda do_init=1, off=0, n=4, N=1: L.acas2d_reset_f64(C.byref(cfg), C.byref(full), None, None, do_init, 0, off,  # noqa: E731
                                                                 n, N, None)
    assert reset(N=0) == -22 and L.acas2d_last_error() == b"acas2d_reset: n_traffic = 0"
    assert reset(off=-1) == -22 and L.acas2d_last_error() == b"acas2d_reset: negative n_envs / env_offset"
    assert reset(do_init=-1) == -22 and L.acas2d_last_error() == b"acas2d_reset: do_init = -1"
    assert reset(do_init=-1, n=0) == 0                         # no envs: done before do_init is looked at
    # acas2d_rollout_*: the shared rejections in its own words, and the packed-only work shape
    roll = lambda T=4, N=8, n=4, off=0, io=C.byref(io_ok), c=C.byref(cfg): L.acas2d_rollout_f32(c, C.byref(full), io, T, 0,  # noqa: E731
                                                                                               off, n, N, None)
    assert roll(c=None) == -22 and L.acas2d_last_error() == b"acas2d_rollout: NULL cfg / io"
    assert roll(io=None) == -22 and L.acas2d_last_error() == b"acas2d_rollout: NULL cfg / io"
    assert roll(io=C.byref(g.native.CStepIO(*([base] * 4)))) == -22 and b"outcome are required" in L.acas2d_last_error()
    assert roll(T=0) == -22 and L.acas2d_last_error() == b"acas2d_rollout: n_traffic = 8, n_steps = 0"
    assert roll(N=0) == -22 and L.acas2d_last_error() == b"acas2d_rollout: n_traffic = 0, n_steps = 4"
    assert roll(n=-1) == -22 and L.acas2d_last_error() == b"acas2d_rollout: negative n_envs / env_offset"
    assert roll(n=0) == 0
    assert roll(N=5) == -22 and b"acas2d_rollout: n_traffic = 5 has no packed work shape" in L.acas2d_last_error()
    # acas2d_rollout_policy_* / acas2d_collect_* (which words these as the former): NULL pointers and obs_in
    pol = g.native.CPolicy(*([base] * 6), 64, 0)
    ac = g.native.CActorCritic(pol, *([base] * 9), 7, 0)
    policy = lambda p=C.byref(pol), io=C.byref(io_ok), obs=base: L.acas2d_rollout_policy_f64(C.byref(cfg), C.byref(full), io,  # noqa: E731
                                                                                              p, obs, 4, 0, 0, 4, 4, None)
    assert policy(p=None) == -22 and L.acas2d_last_error() == b"acas2d_rollout_policy: NULL cfg / io / policy"
    assert policy(io=None) == -22 and L.acas2d_last_error() == b"acas2d_rollout_policy: NULL cfg / io / policy"
    assert policy(obs=None) == -22 and b"rollout_policy: obs_in, actions (output), obs" in L.acas2d_last_error()
    assert L.acas2d_collect_f32(None, C.byref(full), C.byref(io_ok), C.byref(ac), base, 4, 0, 0, 4, 4, None) == -22
    assert L.acas2d_last_error() == b"acas2d_rollout_policy: NULL cfg / io / policy"
    assert L.acas2d_collect_f32(C.byref(cfg), C.byref(full), C.byref(io_ok), C.byref(ac), None, 4, 0, 0, 4, 4, None) == -22
    assert b"acas2d_rollout_policy: obs_in, actions (output)" in L.acas2d_last_error()
    with pytest.raises(RuntimeError, match="acas2d: error -22"):
        g.native.check(L.acas2d_launch_geometry(-1, 1, 4, None, None, None, None))
    # headline config: 4 traffic per lane as one 16-byte vector, 2 lanes per env, 32 envs per wave
    assert g.native.launch_geometry(65536, 8) == {"lanes_per_env": 2, "traffic_per_lane": 4,
                                                  "block_threads": 256, "grid_blocks": 512}
    assert g.native.launch_geometry(65536, 8, 8)["traffic_per_lane"] == 4         # float64: 4 per lane (2 x 16 B)
    assert g.native.launch_geometry(4096, 3)["lanes_per_env"] == 1
    assert g.native.launch_geometry(10, 1)["lanes_per_env"] == 1
    assert g.native.launch_geometry(65536, 64)["lanes_per_env"] == 16
    assert L.acas2d_state_size() == C.sizeof(g.native.CState)
    # consecutive ("arena") layout, include/acas2d.h: pointer arithmetic only, so synthetic addresses do
    E, N, b = 2048, 8, 1 << 20

    def arena(elem=4, **over):
        f = {n: 0 for n, _ in g.native.CState._fields_}
        for k, n in enumerate(("own_x", "own_y", "own_psi", "total_reward", "steps")):
            f[n] = b + k * E * elem
        for k, n in enumerate(("own_v", "goal_x", "goal_y", "episode")):
            f[n] = 2 * b + k * E * elem
        f["trf_x"], f["trf_y"] = 3 * b, 3 * b + E * N * elem
        f["trf_psi"], f["trf_v"] = 4 * b, 4 * b + E * N * elem
        f["status"], f["trace"] = 5 * b, None
        f.update(over)
        return g.native.CState(*[f[n] for n, _ in g.native.CState._fields_])

    yes = lambda st, n=N, elem=4, e=E: L.acas2d_state_is_consecutive(C.byref(st), e, n, elem)  # noqa: E731
    assert yes(arena()) == 1
    assert yes(arena(own_y=b + 4 * E + 4)) == 0 and yes(arena(trf_v=4 * b)) == 0 and yes(arena(episode=6 * b)) == 0
    assert yes(arena(), e=E - 1) == 0 and yes(arena(), e=E - 1024) == 0      # rows are E apart for THIS env count only
    assert yes(arena(elem=8), elem=8) == 0                     # float32 only
    assert yes(arena(), n=5) == 0                              # no packed work shape for 5 traffic aircraft
    E = 2048 + 512                                             # whole multiples of eight workgroups only (1 024 envs at N = 8)
    assert yes(arena(), e=E) == 0
    E = 3072
    assert yes(arena(), e=E) == 1
    assert yes(arena(own_x=None)) == 0 and L.acas2d_state_is_consecutive(None, E, N, 4) == 0
    geo = g.native.launch_geometry(7, 200)                                          # generic walk
    assert geo["lanes_per_env"] == 64 and geo["traffic_per_lane"] == -1
    with pytest.raises(RuntimeError, match="LDS"):
        g.native.launch_geometry(16, 5000)


_READ_ARRAYS = ("own_x", "own_y", "own_psi", "own_v", "goal_x", "goal_y", "trf_x", "trf_y", "trf_psi", "trf_v", "steps",
                "total_reward", "status", "episode")


class _SyntheticF64State:
    """A float64 state of E envs x N traffic on host memory: array k of _READ_ARRAYS in slot k (SLOT bytes apart).
    Every case built from it must be rejected by acas2d_step's validation BEFORE any launch: the addresses are not
    device memory."""
    E, N, SLOT = 4, 2, 1024

    def __init__(self, g):
        self.g, self.L = g, g.native.lib()
        self.buf = (C.c_char * (self.SLOT * 64))()
        self.base = C.addressof(self.buf) + 16 * self.SLOT          # room below for negative offsets
        self.cfg = g.ACAS2DConfig(n_traffic=self.N).to_c()
        self.at = {n: self.base + k * self.SLOT for k, n in enumerate(_READ_ARRAYS)}
        self.st = g.native.CState(*[self.at.get(n) for n, _ in g.native.CState._fields_])      # trace stays NULL
        self.io = g.native.CStepIO(*([self.base + 40 * self.SLOT] * 5 + [None] * 3))
        E, N = self.E, self.N
        self.bytes = {n: E * N * 8 if n.startswith("trf") else E * {"steps": 4, "status": 1, "episode": 4}.get(n, 8)
                      for n in _READ_ARRAYS}

    def out(self, d=0, dt=0):
        """state_out: own_x, own_y, own_psi, total_reward (float64) and steps (int32) d ELEMENTS from state's, trf_x and
        trf_y dt elements; everything else shared."""
        f = dict(self.at)
        for n in ("own_x", "own_y", "own_psi", "total_reward"):
            f[n] += 8 * d
        f["steps"] += 4 * d
        for n in ("trf_x", "trf_y"):
            f[n] += 8 * dt
        return self.g.native.CState(*[f.get(n) for n, _ in self.g.native.CState._fields_])

    def step(self, out):
        return self.L.acas2d_step_f64(C.byref(self.cfg), C.byref(self.st), C.byref(out), C.byref(self.io),
                                      self.g.native.AUTO_RESET, 0, 0, self.E, self.N, None)


def test_state_out_writing_into_another_array_of_state_is_rejected(g):
    """write_offsets(): each double-buffered array only clearing ITSELF is not enough -- state_out.own_x == state.own_y
    (one element offset of E, as far as own_x alone can tell a clean second generation) would stream one env's stores
    over rows other wavefronts are still reading."""
    s = _SyntheticF64State(g)
    d = s.SLOT // 8                                                  # out.own_x == st.own_y, out.own_y == st.own_psi ...
    assert s.out(d=d).own_x == s.st.own_y
    assert s.step(s.out(d=d)) == -22
    assert b"state_out's own_x overlaps state's own_y" in s.L.acas2d_last_error()
    # the same for the traffic pair: out.trf_x == st.trf_y
    dt = s.SLOT // 8
    assert s.step(s.out(dt=dt)) == -22 and b"state_out's trf_x overlaps state's trf_y" in s.L.acas2d_last_error()


@pytest.mark.parametrize("group", ("env", "trf"))
@pytest.mark.parametrize("target", _READ_ARRAYS)
def test_state_out_overlap_with_each_array_of_state_is_rejected(g, group, target):
    """One written group (own_x .. steps, or trf_x / trf_y) moved so that its first array's first element lies on the
    LAST element of one array the step reads -- a one-element overlap, from above or below -- for every array of state:
    the double-buffered ones and the ones shared between the two structs (written in place at a reset)."""
    s = _SyntheticF64State(g)
    first = "own_x" if group == "env" else "trf_x"
    last = s.at[target] + (s.bytes[target] - 1) // 8 * 8             # the float64-aligned word holding its last byte
    off = (last - s.at[first]) // 8
    out = s.out(d=off) if group == "env" else s.out(dt=off)
    assert s.step(out) == -22, target
    assert (b"state_out's %s overlaps state's %s" % (first.encode(), target.encode())) in s.L.acas2d_last_error()


def test_state_out_overlap_is_checked_in_bytes(g):
    """steps is int32 while the float64 arrays are 8 bytes wide: one element offset d moves steps by 4 d bytes and the
    others by 8 d.  Here only the written steps row lands inside state's total_reward -- in its SECOND half, which a
    check that counted every array as E 4-byte elements would not see."""
    s = _SyntheticF64State(g)
    d = (s.at["total_reward"] + 4 * s.E - s.at["steps"]) // 4
    out = s.out(d=d)
    assert out.steps == s.at["total_reward"] + 4 * s.E
    for n in ("own_x", "own_y", "own_psi", "total_reward"):          # the float64 rows land right behind other arrays
        w0 = getattr(out, n)
        assert all(w0 >= s.at[r] + s.bytes[r] or w0 + 8 * s.E <= s.at[r] for r in _READ_ARRAYS), n
    assert s.step(out) == -22
    assert b"state_out's steps overlaps state's total_reward" in s.L.acas2d_last_error()


def _packed_shapes(build):
    src = open(os.path.join(ROOT, "gym-acas2d_amd", "csrc", "acas2d_%s.hip" % build)).read()
    line = re.search(r"^#define ACAS2D_PACKED_SHAPES\(X\)(.*)$", src, re.M).group(1)
    return {(int(c), int(gl)) for c, gl in re.findall(r"X\(\s*(\d+)\s*,\s*(\d+)\s*\)", line)}


def test_shape_table_is_exactly_the_compiled_set():
    """helpers.SHAPES (the rows the GPU tests run) against the instantiations: a shape added to ACAS2D_PACKED_SHAPES
    without a row, or a row whose shape is no longer compiled, fails here -- for float32 and for each float64
    formulation (one instantiation per formulation)."""
    builds = {"float32": _packed_shapes("f32"), "float64": _packed_shapes("f64")}
    assert (4, 2) in builds["float32"] and (4, 2) in builds["float64"] and len(builds["float32"]) >= 10
    for dtype, math in (("float32", "fast"), ("float64", "exact"), ("float64", "fast")):
        rows = [s for s in H.SHAPES if (s.dtype, s.math) == (dtype, math)]
        assert {(s.C, s.G) for s in rows if s.packed} == builds[dtype], (dtype, math)
        assert {s.G for s in rows if not s.packed} == set(H.GENERIC_G), (dtype, math)
        assert len(rows) == len(builds[dtype]) + len(H.GENERIC_G), (dtype, math)        # one row per shape
    assert all(s.math == "fast" for s in H.SHAPES if s.dtype == "float32")


@pytest.mark.parametrize("shape", H.SHAPES, ids=[s.id for s in H.SHAPES])
def test_shape_table_rows_resolve_to_their_shape(g, monkeypatch, shape):
    """Each row's N (and ACAS2D_SHAPE, where it has one) resolves to the row's (C, G) in launch_geometry() -- the
    same resolve_shape() the step / reset / rollout launches call -- so a GPU test run on that row runs that kernel.
    (An override that named a shape no longer compiled would fall back to the generic walk and fail here.)"""
    if shape.override is None:
        monkeypatch.delenv("ACAS2D_SHAPE", raising=False)
    else:
        monkeypatch.setenv("ACAS2D_SHAPE", shape.override)
    geo = g.native.launch_geometry(1000, shape.n_traffic, shape.elem)
    assert geo["lanes_per_env"] == shape.G
    assert geo["traffic_per_lane"] == (shape.C if shape.packed else -1)
    if shape.packed:
        assert shape.C * shape.G == shape.n_traffic


def test_no_cpu_fallback(g, monkeypatch):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError, match="no CPU fallback|no GPU"):
        g.ACAS2DVecEnv(4, 1)
    with pytest.raises(RuntimeError):
        g.ACAS2DVecEnv(4, 1, device="cpu")
    monkeypatch.setattr(g.native, "LIB_PATH", "/nonexistent/libacas2d_hip.so")
    monkeypatch.setattr(g.native, "_lib", None)
    with pytest.raises(g.native.NativeLibraryError, match="no CPU fallback"):
        g.native.lib()


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "gym-acas2d_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".inl", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in src.replace("oracle-state", "").replace("oracle vectors", "") \
                    .replace("Oracle", ""), os.path.join(dirpath, f)


def test_spaces_and_sharding(g):
    b = g.Box(low=-1, high=1, shape=(1,), dtype=np.float64)
    assert b.shape == (1,) and b.contains(np.array([0.5])) and not b.contains(np.array([1.5]))
    tot = 1048576
    blocks = [g.shard_range(tot, r, 8) for r in range(8)]
    assert blocks[0] == (0, 131072) and blocks[7] == (917504, 131072)          # BASELINE configs[3]
    for world in (1, 2, 3, 7, 8):
        bl = [g.shard_range(1000, r, world) for r in range(world)]
        assert bl[0][0] == 0 and sum(c for _, c in bl) == 1000
        assert all(bl[i][0] + bl[i][1] == bl[i + 1][0] for i in range(world - 1))
        assert max(c for _, c in bl) - min(c for _, c in bl) <= 1


# ---- the learner's kernels: compiled sets, workspace layout, argument validation ------------------------------------
def _ppo_widths():
    src = open(os.path.join(ROOT, "gym-acas2d_amd", "csrc", "acas2d_ppo.hip")).read()
    body = re.search(r"switch \(D\) \{(.*?)default:", src, re.S).group(1)
    return [int(d) for d in re.findall(r"case (\d+): rc = launch_grad<\1>", body)]


def test_learner_kernel_lists_are_exactly_the_compiled_set():
    """learner_ref.UPDATE_WIDTHS (the widths tests/test_learner_kernels.py runs acas2d_ppo_update_f32 at) against the
    obs_dim switch of acas2d_ppo.hip, and learner_ref.POLICY_KERNELS (the collector / rollout-policy instantiations it
    runs) against the G = 1 packed shapes of each build -- float32 FAST, float64 EXACT and FAST.  An instantiation added
    or removed on either side fails here."""
    import learner_ref as R
    widths = _ppo_widths()
    assert len(widths) == len(set(widths)) and 8 in widths
    assert tuple(sorted(widths)) == tuple(R.UPDATE_WIDTHS)
    want = [("float32", True, c) for c, gl in sorted(_packed_shapes("f32")) if gl == 1]
    want += [("float64", fast, c) for fast in (False, True) for c, gl in sorted(_packed_shapes("f64")) if gl == 1]
    assert len(want) >= 13 and sorted(want) == sorted(R.POLICY_KERNELS) and len(set(R.POLICY_KERNELS)) == len(R.POLICY_KERNELS)


def test_ppo_workspace_is_the_13_parameter_tensors(g):
    """acas2d_ppo_workspace_floats(D) == the total numel of FusedUpdate's 13 parameter tensors of ActorCritic(D), in
    learner_ref.PARAM_NAMES order (the flat layout the float64 references unflatten)."""
    import torch

    import learner_ref as R
    L = g.native.lib()
    for D in _ppo_widths():
        pol = g.ActorCritic(D)
        z = lambda *s: torch.zeros(*s)  # noqa: E731
        fu = g.FusedUpdate(pol, g.PPOConfig(), z(4, D), z(4), z(4), z(4), z(4))      # host only: nothing is launched
        assert len(fu._params) == 13 and all(p is pol.get_parameter(n) for p, n in zip(fu._params, R.PARAM_NAMES))
        total = sum(p.numel() for p in fu._params)
        assert L.acas2d_ppo_workspace_floats(D) == total == fu.grad.numel() == R.segments(pol)[-1][2], D


def test_ppo_update_validation_needs_no_gpu(g):
    import learner_support as LS
    L = g.native.lib()
    assert L.acas2d_ppo_update_f32(None, None) == -22 and b"NULL argument" in L.acas2d_last_error()
    pointers = [n for n, t in g.native.CPpoUpdate._fields_ if t is C.c_void_p]
    assert len(pointers) == 24
    for name in pointers:
        u, _keep = LS.host_update(g, **{name: None})
        assert L.acas2d_ppo_update_f32(C.byref(u), None) == -22, name
        assert b"every pointer is required" in L.acas2d_last_error(), name
    for n_rows in (1, 0, -5):
        u, _keep = LS.host_update(g, n_rows=n_rows)
        assert L.acas2d_ppo_update_f32(C.byref(u), None) == -22
        assert (b"n_rows = %d" % n_rows) in L.acas2d_last_error()
    for D in (0, 5, 7, 9, 20, 30, -8, 53):
        u, _keep = LS.host_update(g, obs_dim=D)
        assert L.acas2d_ppo_update_f32(C.byref(u), None) == -22
        assert (b"obs_dim = %d" % D) in L.acas2d_last_error()


def test_collect_and_rollout_policy_validation_needs_no_gpu(g):
    """acas2d_collect_* / acas2d_rollout_policy_* reject, before any launch: a traffic count with no thread-per-env
    shape (float32 N = 5, float64 N = 8), hidden != 64, and (collect) a missing value net, log_std or output."""
    L = g.native.lib()
    buf = (C.c_double * 4096)()
    a = C.addressof(buf)
    st = g.native.CState(*([a] * 14))
    io = g.native.CStepIO(*([a] * 5 + [None] * 3))

    def pol(hidden=64):
        return g.native.CPolicy(*([a] * 6), hidden, 0)

    def ac(hidden=64, **none):
        f = {n: a for n, _ in g.native.CActorCritic._fields_[1:10]}
        f.update(none)
        return g.native.CActorCritic(pol(hidden), **f, noise_seed=7, noise_step=0)

    for dt, N in (("f32", 5), ("f64", 8)):
        cfg = g.ACAS2DConfig(n_traffic=N).to_c()
        rp, cl = getattr(L, "acas2d_rollout_policy_" + dt), getattr(L, "acas2d_collect_" + dt)
        assert rp(C.byref(cfg), C.byref(st), C.byref(io), C.byref(pol()), a, 4, 13, 0, 64, N, None) == -22
        assert b"no thread-per-env shape" in L.acas2d_last_error()
        assert cl(C.byref(cfg), C.byref(st), C.byref(io), C.byref(ac()), a, 4, 13, 0, 64, N, None) == -22
        assert b"no thread-per-env shape" in L.acas2d_last_error()
    for dt, N in (("f32", 8), ("f64", 4), ("f32", 1)):
        cfg = g.ACAS2DConfig(n_traffic=N).to_c()
        rp, cl = getattr(L, "acas2d_rollout_policy_" + dt), getattr(L, "acas2d_collect_" + dt)
        for hidden in (32, 0, 65):
            assert rp(C.byref(cfg), C.byref(st), C.byref(io), C.byref(pol(hidden)), a, 4, 13, 0, 64, N, None) == -22
            assert (b"got hidden = %d" % hidden) in L.acas2d_last_error()
            assert cl(C.byref(cfg), C.byref(st), C.byref(io), C.byref(ac(hidden)), a, 4, 13, 0, 64, N, None) == -22
            assert (b"got hidden = %d" % hidden) in L.acas2d_last_error()
        for name in ("v1t", "vb1", "v2t", "vb2", "v3", "vb3", "log_std", "values", "logp"):
            assert cl(C.byref(cfg), C.byref(st), C.byref(io), C.byref(ac(**{name: None})), a, 4, 13, 0, 64, N, None) == -22, name
            assert b"the value net, log_std, values and logp are required" in L.acas2d_last_error(), name
        assert cl(C.byref(cfg), C.byref(st), C.byref(io), None, a, 4, 13, 0, 64, N, None) == -22
        assert b"NULL actor-critic" in L.acas2d_last_error()


# ---- the non-default configurations of the GPU tests (helpers.NONDEFAULT_CONFIGS) ------------------------------------
# to_c() fields no ACAS2DConfig can move: the first traffic aircraft's heading base and step are constants of game.py:105,
# and the player starts at the goal's height (own_y0 == goal_y == height / 2, game.py:80-87), so the heading from start
# to goal is always 0.  `math` selects the float64 build's formulation and is not part of the environment.
_FIXED_BY_CONSTRUCTION = ("t0_heading_base", "t0_heading_step", "own_heading0", "math")


def _window_outcomes(O, cfg, E, N, T, seed, env_offset, warmup):
    """Occurrences of each outcome, and the distinct traffic speeds, in the oracle side of a float32 window."""
    counts, speeds = {}, set()
    for _, _, _, _, _, _, chk, (_, _, d, oc) in H.f32_oracle_steps(O, E, N, T, seed, env_offset, warmup,
                                                                   H.oracle_config(O, cfg)):
        for k in oc[d != 0]:
            counts[int(k)] = counts.get(int(k), 0) + 1
        speeds |= set(np.unique(chk.trf_v).tolist())
    return counts, len(speeds)


@pytest.mark.parametrize("name", tuple(H.NONDEFAULT_CONFIGS))
def test_nondefault_configs_move_every_tunable_and_cover_the_outcomes_the_gpu_tests_claim(g, oracle_mod, name):
    """Each non-default configuration differs from the default in every to_c() field that a configuration can move, and
    the CPU oracle, run over the windows of the GPU tests that use it (same seed, env_offset, warm-up and actions),
    produces there the outcomes those tests assert they compared (at least 5 times each: helpers.nondefault_outcomes
    lists exactly these) with more than 10 distinct traffic speeds.  A later edit of a configuration or a window that
    drops goals or timeouts from a GPU test fails here, without a GPU."""
    O = oracle_mod
    kw = H.NONDEFAULT_CONFIGS[name]
    c, d = g.ACAS2DConfig(**kw).to_c(), g.ACAS2DConfig().to_c()
    for field, _ in type(c)._fields_:
        if field in _FIXED_BY_CONSTRUCTION:
            assert getattr(c, field) == getattr(d, field), field
        else:
            assert getattr(c, field) != getattr(d, field), field
    assert c.own_y0 == c.goal_y and c.own_heading0 == 0
    w = H.NONDEFAULT_SHAPE_WINDOW[name]
    for N in sorted({s.n_traffic for s in H.SHAPES if s.dtype == "float32"}):
        counts, speeds = _window_outcomes(O, g.ACAS2DConfig(n_traffic=N, **kw), 1001, N, w["T"], w["seed"],
                                          w["env_offset"], w["warmup"])
        assert {k for k, n in counts.items() if n >= 5} == H.nondefault_outcomes(name, N), (N, counts)
        assert speeds > 10, (N, speeds)
    if name == "wide":
        for N, E, T in H.ODD_TRAFFIC:
            counts, speeds = _window_outcomes(O, g.ACAS2DConfig(n_traffic=N, **kw), E, N, T, **H.NONDEFAULT_ODD_WINDOW)
            assert min(counts.get(H.COLLISION, 0), counts.get(H.TIMEOUT, 0)) >= 5 and speeds > 10, (N, counts, speeds)
    # test_f32_reset_names_the_same_episodes_nondefault: 40 steps from reset() (seed 5) end enough episodes
    E, N = 4096, 8
    ref = O.OracleEnvs(E, N, seed=5, auto_reset=True, config=H.oracle_config(O, g.ACAS2DConfig(n_traffic=N, **kw)))
    ref.reset()
    rng = np.random.default_rng(3)
    assert sum(int(ref.step(rng.uniform(-1, 1, E).astype(np.float32).astype(np.float64))[4]) for _ in range(40)) > 200


def test_f32_bounds_of_the_default_configuration_are_the_fixed_ones(oracle_mod):
    """helpers.f32_bounds / f32_pos_bound evaluate, for the default configuration, to exactly the numbers the float32
    tests held before the bounds were derived from the configuration; the non-default ones are at least as large."""
    dflt = oracle_mod.default_config()
    assert H.f32_bounds(dflt, dflt) == dict(band=1e-3, ret=1.3e-4 + 1e-5, rew=5e-5, reset_pos=2.5e-4,
                                                reset_psi=6e-5, speed=None)
    assert 1 - H.f32_bounds(dflt, dflt)["band"] == 0.999
    assert H.f32_pos_bound(1600) == H.f32_pos_bound(2047.9) == 1.3e-4 and H.f32_pos_bound(2514) == 2 ** -12
    import gym_acas2d_amd as g
    for kw in H.NONDEFAULT_CONFIGS.values():
        b = H.f32_bounds(H.oracle_config(oracle_mod, g.ACAS2DConfig(**kw)), dflt)
        assert all(b[k] >= v for k, v in H.f32_bounds(dflt, dflt).items() if v is not None) and b["speed"] > 0


def test_wide_keys_cross_2_to_the_32_where_the_gpu_tests_claim(g, oracle_mod):
    """helpers.WIDE_*: the seed's halves are non-zero and distinct; for every work shape of helpers.SHAPES the global
    env index crosses 2^32 inside a wave and a workgroup at both env_offsets ("tail": inside the last, partial wave
    wherever it holds more than one env), every wave holds preset and plain episode counters, and the GPU tests' runs
    really wrap preset counters through 2^32 - 1 to 0: the float64 shape runs (90 steps, max_steps 40) and the float32
    windows of helpers.wide_f32_window -- re-measured on the oracle here."""
    O = oracle_mod
    lo, hi = H.WIDE_SEED & 0xFFFFFFFF, H.WIDE_SEED >> 32
    assert 0 < lo != hi > 0 and hi < 2 ** 32
    E, block = H.WIDE_E, 256 // 64                       # waves per workgroup (kWavesPerBlock)
    pre = H.wide_preset(E)
    for shape in H.SHAPES:
        wave = shape.envs_per_wave
        for key, off in H.WIDE_OFFSET.items():
            c = 2 ** 32 - off
            assert 0 < c < E and off + c == 2 ** 32 and (off + c - 1) >> 32 == 0, (shape.id, key)
            if wave > 1:
                assert c % wave != 0 and c % (wave * block) != 0, (shape.id, key)     # not on a wave / workgroup start
                w0 = c - c % wave
                assert pre[w0:w0 + wave].any() and (~pre[w0:w0 + wave]).any(), shape.id
            if key == "tail" and E % wave > 1:
                assert c >= E - E % wave, shape.id                                   # the last, partial wave
        # test_waves_finishing_together_vs_oracle's wide cases: E = 32 waves, the crossing inside the middle one
        c = 2 ** 32 - H.wide_crossing_offset(32 * wave, wave)
        assert c // wave == 16 and (wave == 1 or c % wave != 0), shape.id
    assert sum(s.envs_per_wave > 1 and E % s.envs_per_wave > 1 for s in H.SHAPES) >= 10
    for N in sorted({s.n_traffic for s in H.SHAPES}):
        cfg = g.ACAS2DConfig(n_traffic=N, max_steps=40)
        ocfg = H.oracle_config(O, cfg)
        for key, off in H.WIDE_OFFSET.items():
            ref = O.OracleEnvs(E, N, seed=H.WIDE_SEED, env_offset=off, auto_reset=True, config=ocfg)
            ref.reset()
            ref.episode[pre] = H.WIDE_EPISODE
            rng = np.random.default_rng(1)
            wrapped = 0
            for _ in range(90):
                _, _, d, _, _ = ref.step(rng.uniform(-1, 1, E))
                wrapped += int(((d != 0) & (ref.episode == 0)).sum())
            assert wrapped >= 50 and (ref.episode[pre] < 2 ** 31).sum() >= 50, (N, key, wrapped)
            warmup, T = H.wide_f32_window(N)
            episode = np.where(pre, H.WIDE_EPISODE, 0).astype(np.uint32)
            wrapped = 0
            for _, _, _, _, _, _, chk, (_, _, d, _) in H.f32_oracle_steps(O, E, N, T, H.WIDE_SEED, off, warmup, ocfg,
                                                                         episode):
                wrapped += int(((d != 0) & (chk.episode == 0)).sum())
            assert wrapped >= 5, (N, key, wrapped)


def test_arena_layout_size_bound_at_the_32_bit_limit(g):
    """acas2d_state_is_consecutive at its size bound (helpers.ARENA_BOUND): the largest whole-workgroup env count with
    8 E N < 2^32 and 20 E < 2^32 is admitted, the next one is not (N = 8 and 64: the traffic term; N = 2: the [5][E]
    term).  Synthetic addresses, as in test_c_abi_argument_validation_needs_no_gpu."""
    L = g.native.lib()

    def arena(E, N):
        b = 1 << 40
        f = {n: 0 for n, _ in g.native.CState._fields_}
        for k, n in enumerate(("own_x", "own_y", "own_psi", "total_reward", "steps")):
            f[n] = b + k * E * 4
        for k, n in enumerate(("own_v", "goal_x", "goal_y", "episode")):
            f[n] = 2 * b + k * E * 4
        f["trf_x"], f["trf_y"] = 3 * b, 3 * b + E * N * 4
        f["trf_psi"], f["trf_v"] = 4 * b, 4 * b + E * N * 4
        f["status"], f["trace"] = 5 * b, None
        return g.native.CState(*[f[n] for n, _ in g.native.CState._fields_])

    for N, e_yes, e_no in H.ARENA_BOUND:
        geo = g.native.launch_geometry(e_yes, N, 4)
        unit = (64 // geo["lanes_per_env"]) * 4 * 8                # whole multiples of eight workgroups
        assert e_yes % unit == 0 and e_no == e_yes + unit, N
        assert 8 * e_yes * N < 2 ** 32 and 20 * e_yes < 2 ** 32, N
        assert 8 * e_no * N >= 2 ** 32 or 20 * e_no >= 2 ** 32, N
        assert (20 * e_no >= 2 ** 32) == (N <= 2) and (8 * e_no * N < 2 ** 32) == (N <= 2), N   # which term binds
        assert L.acas2d_state_is_consecutive(C.byref(arena(e_yes, N)), e_yes, N, 4) == 1, N
        assert L.acas2d_state_is_consecutive(C.byref(arena(e_no, N)), e_no, N, 4) == 0, N
        assert L.acas2d_state_is_consecutive(C.byref(arena(e_yes - unit, N)), e_yes - unit, N, 4) == 1, N
