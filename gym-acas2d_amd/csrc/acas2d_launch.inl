// acas2d_launch.inl -- host-side launchers, included by acas2d_f32.hip and acas2d_f64.hip which
// define ACAS2D_PACKED_SHAPES(X) (the (C, G) pairs to instantiate for their element type), Elem (that
// type) and kFast (its own formulation); the launchers are instantiated for Elem at the end.  (Two
// translation units: each element type is compiled with its own flags.  Both use -ffp-contract=off
// today, so only the fma()s written in the source fuse.)
#include <stdlib.h>
#include <cmath>
#include <initializer_list>
#include <type_traits>

#include "acas2d_kernels.hpp"

namespace acas2d {

template <typename T>
static Params<T> make_params(const Acas2dConfig& c) {
    Params<T> p;
    p.dt = (T)c.dt; p.acc_lat_limit = (T)c.acc_lat_limit; p.collision_dist = (T)c.collision_dist;
    p.goal_radius = (T)c.goal_radius; p.safe_distance = (T)c.safe_distance;
    p.d_goal_max = (T)c.d_goal_max; p.d_dev_max = (T)c.d_dev_max; p.d_sep_max = (T)c.d_sep_max;
    p.d_cpa_max = (T)c.d_cpa_max; p.v_closing_max = (T)c.v_closing_max;
    p.rw_d_goal_max = (T)c.rw_d_goal_max; p.rw_d_dev_max = (T)c.rw_d_dev_max;
    p.reward_goal = (T)c.reward_goal; p.reward_collision = (T)c.reward_collision;
    p.inv_dt = (T)(1.0 / c.dt); p.inv_d_goal_max = (T)(1.0 / c.d_goal_max);
    p.inv_d_dev_max = (T)(1.0 / c.d_dev_max); p.inv_d_sep_max = (T)(1.0 / c.d_sep_max);
    p.inv_d_cpa_max = (T)(1.0 / c.d_cpa_max); p.inv_v_closing_max = (T)(1.0 / c.v_closing_max);
    p.inv_rw_d_goal_max = (T)(1.0 / c.rw_d_goal_max); p.inv_rw_d_dev_max = (T)(1.0 / c.rw_d_dev_max);
    p.inv_safe_distance = (T)(1.0 / c.safe_distance); p.inv_max_steps = (T)(1.0 / (double)c.max_steps);
    p.max_steps = c.max_steps;
    return p;
}

template <typename T, bool ROLLOUT>
static StepResetParams<T, ROLLOUT> make_reset_params(const Acas2dConfig& c) {
    using R = typename std::conditional<ROLLOUT, double, T>::type;
    // the goal terms of a fresh episode (own_context_fresh()): game.py:168-180 at the start position
    const double gdx = c.goal_x - c.own_x0, gdy = c.goal_y - c.own_y0;
    double bearing = std::atan2(gdy, gdx);
    if (bearing < 0) bearing += 6.283185307179586476925;
    else if (bearing == 0) bearing = 0;
    return StepResetParams<T, ROLLOUT>{(R)c.own_x0, (R)c.own_y0, (R)c.own_v, (R)c.own_heading0, (R)c.own_heading_jitter,
                                       (R)c.goal_x, (R)c.goal_y, (R)c.t0_x, (R)c.t0_y_base, (R)c.t0_y_span,
                                       (R)c.t0_heading_base, (R)c.t0_heading_step, (R)c.t0_heading_jitter, (R)c.tn_x_max,
                                       (R)c.tn_y_max, (R)c.speed_factor_min, (R)c.speed_factor_max, (R)c.airspeed,
                                       (T)std::sqrt(std::fma(gdy, gdy, gdx * gdx)), (T)(bearing * 57.29577951308232087680), (T)gdy};
}

template <typename T>
static State<T> make_state(const Acas2dState& s) {
    return State<T>{(T*)s.own_x, (T*)s.own_y, (T*)s.own_psi, (T*)s.own_v, (T*)s.goal_x, (T*)s.goal_y,
                    (T*)s.trf_x, (T*)s.trf_y, (T*)s.trf_psi, (T*)s.trf_v, s.steps,
                    (T*)s.total_reward, s.status, s.episode, (T*)s.trace, 0, 0};
}

static bool state_complete(const Acas2dState* s) {
    return s && s->own_x && s->own_y && s->own_psi && s->own_v && s->goal_x && s->goal_y && s->trf_x &&
           s->trf_y && s->trf_psi && s->trf_v && s->steps && s->total_reward && s->status && s->episode;
}

// Double-buffered state (acas2d_step_* with a state_out): the element offsets of `out`'s per-step arrays from
// `st`'s -- own_x, own_y, own_psi, steps, total_reward share one (w_env), trf_x and trf_y another (w_trf); e.g.
// every such array allocated as [2][E] / [2][E][N] and the two structs pointing at its two halves.  Everything
// else must be the same buffer in both structs (those arrays change at a reset only, in place).
template <typename T>
static int write_offsets(const Acas2dState* st, const Acas2dState* out, bool auto_reset, int64_t n_envs, int n_traffic,
                         int32_t* w_env, int32_t* w_trf) {
    *w_env = 0; *w_trf = 0;
    if (!out || out == st) return ACAS2D_OK;
    if (!state_complete(out)) { set_error("acas2d_step: state_out has a NULL buffer"); return ACAS2D_EINVAL; }
    if (out->own_v != st->own_v || out->goal_x != st->goal_x || out->goal_y != st->goal_y || out->trf_psi != st->trf_psi ||
        out->trf_v != st->trf_v || out->status != st->status || out->episode != st->episode || out->trace != st->trace) {
        set_error("acas2d_step: state_out must share own_v, goal_x, goal_y, trf_psi, trf_v, status, episode and trace with state "
                  "(only own_x, own_y, own_psi, steps, total_reward, trf_x, trf_y are double-buffered)");
        return ACAS2D_EINVAL;
    }
    const int64_t d = (const T*)out->own_x - (const T*)st->own_x, dt = (const T*)out->trf_x - (const T*)st->trf_x;
    if ((const T*)out->own_y - (const T*)st->own_y != d || (const T*)out->own_psi - (const T*)st->own_psi != d ||
        (const T*)out->total_reward - (const T*)st->total_reward != d || out->steps - st->steps != d ||
        (const T*)out->trf_y - (const T*)st->trf_y != dt) {
        set_error("acas2d_step: state_out's own_x, own_y, own_psi, steps, total_reward must lie at ONE element offset from "
                  "state's, trf_x and trf_y at one (e.g. each array allocated [2][E] / [2][E][N])");
        return ACAS2D_EINVAL;
    }
    if (d == 0 && dt == 0) return ACAS2D_OK;
    if (!auto_reset) {
        set_error("acas2d_step: a separate state_out needs ACAS2D_AUTO_RESET (the latching step leaves frozen traffic unwritten)");
        return ACAS2D_EINVAL;
    }
    const int64_t lim = 0x7fffffffLL - n_envs * (int64_t)n_traffic - 64;
    const int64_t ad = d < 0 ? -d : d, adt = dt < 0 ? -dt : dt;
    if (ad > lim || adt > lim) {
        set_error("acas2d_step: state_out lies more than 2^31 elements away from state");
        return ACAS2D_EINVAL;
    }
    // No byte a moved group writes may be one the step reads: any array of `st` (trace aside), the shared ones
    // written in place at a reset included.  (A group at offset 0 is stepped in place, as without a state_out.)
    // Compared in bytes: steps is int32 while T may be 8 bytes wide.
    const int64_t E = n_envs, EN = n_envs * (int64_t)n_traffic, sT = (int64_t)sizeof(T);
    struct Range { const char* name; const void* p; int64_t bytes; };
    const Range reads[] = {{"own_x", st->own_x, E * sT}, {"own_y", st->own_y, E * sT}, {"own_psi", st->own_psi, E * sT},
                           {"own_v", st->own_v, E * sT}, {"goal_x", st->goal_x, E * sT}, {"goal_y", st->goal_y, E * sT},
                           {"trf_x", st->trf_x, EN * sT}, {"trf_y", st->trf_y, EN * sT}, {"trf_psi", st->trf_psi, EN * sT},
                           {"trf_v", st->trf_v, EN * sT}, {"steps", st->steps, E * 4}, {"total_reward", st->total_reward, E * sT},
                           {"status", st->status, E}, {"episode", st->episode, E * 4}};
    const Range env_writes[] = {{"own_x", out->own_x, E * sT}, {"own_y", out->own_y, E * sT}, {"own_psi", out->own_psi, E * sT},
                                {"total_reward", out->total_reward, E * sT}, {"steps", out->steps, E * 4}};
    const Range trf_writes[] = {{"trf_x", out->trf_x, EN * sT}, {"trf_y", out->trf_y, EN * sT}};
    const auto overlap = [&](const Range& w) -> bool {
        const uintptr_t w0 = (uintptr_t)w.p, w1 = w0 + (uintptr_t)w.bytes;
        for (const Range& r : reads) {
            const uintptr_t r0 = (uintptr_t)r.p, r1 = r0 + (uintptr_t)r.bytes;
            if (w0 < r1 && r0 < w1) {
                set_error("acas2d_step: state_out's %s overlaps state's %s (a double-buffered array must not share a byte "
                          "with any array the step reads)", w.name, r.name);
                return true;
            }
        }
        return false;
    };
    if (d != 0)
        for (const Range& w : env_writes) if (overlap(w)) return ACAS2D_EINVAL;
    if (dt != 0)
        for (const Range& w : trf_writes) if (overlap(w)) return ACAS2D_EINVAL;
    *w_env = (int32_t)d; *w_trf = (int32_t)dt;
    return ACAS2D_OK;
}

static int check_launch(const char* name) {
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) { set_error("%s launch: %s", name, hipGetErrorString(err)); return ACAS2D_EHIP; }
    return ACAS2D_OK;
}

// Launch geometry for a shape: one env per G lanes, 64 / G envs per wavefront, 4 wavefronts per
// workgroup, one LDS observation tile per wavefront.  `group_policy`: the launch evaluates the in-kernel policy
// with the G lanes of an env together and keeps each env's 64 hidden activations behind the wave's tile and reset
// slots (policy_mlp_group(); the kernel finds them at the END of the wave's tile_elems).  `held`: values the launch keeps
// per LANE behind all of that (the correlated flavours' error state, CorrW, and the delayed flavours' lag state behind it, RespW;
// the hidden vectors then end where it begins).
struct Geometry { unsigned grid, block; int tile_elems; size_t lds_bytes; };

template <typename T>
static int geometry_for(const Shape& sh, int64_t n_envs, int n_traffic, Geometry* g, bool group_policy = false, int held = 0) {
    const int64_t epw = 64 / sh.G, envs_per_block = epw * kWavesPerBlock;
    const int64_t blocks = (n_envs + envs_per_block - 1) / envs_per_block;
    if (blocks > 0x7fffffffLL || n_envs > 0x7fffffffLL) { set_error("n_envs = %lld exceeds the launch limit", (long long)n_envs); return ACAS2D_EINVAL; }
    const int W = 16 / (int)sizeof(T);
    // per wave: the observation tile, then the reset slots (SlotLayout<T, N> in the kernels; packed shapes with
    // N + 1 <= 32) or one 4N+1-value hand-off scratch (the other packed shapes), everything 16-byte aligned
    const int64_t tile = (epw * (5 + 3 * (int64_t)n_traffic) + 3) / 4 * 4;
    int64_t scratch = 0;
    if (sh.packed && n_traffic + 1 <= 32) {
        int stride = 2; while (stride < n_traffic + 1) stride *= 2;
        scratch = (64 / stride) * ((4 * (int64_t)n_traffic + 1 + W - 1) / W * W);
    } else if (sh.packed) {
        scratch = 4 * (int64_t)n_traffic + 1;
    }
    const int64_t hidden = group_policy ? epw * kPolicyHidden : 0;
    const int64_t elems = ((tile + scratch + 3) / 4) * 4 + hidden + 64 * (int64_t)held;
    const int64_t bytes = elems * kWavesPerBlock * (int64_t)sizeof(T);
    if (bytes > 64 * 1024) {
        set_error("n_traffic = %d needs a %lld-byte LDS observation tile%s%s per workgroup (limit 65536)", n_traffic, (long long)bytes,
                  group_policy ? " and hidden vectors" : "", held ? " and error state" : "");
        return ACAS2D_EINVAL;
    }
    g->grid = (unsigned)blocks; g->block = (unsigned)kBlock; g->tile_elems = (int)elems; g->lds_bytes = (size_t)bytes;
    return ACAS2D_OK;
}

// "Arena" layout of a float32 state: the per-env arrays a step reads are consecutive [k][E] rows -- own_x, own_y,
// own_psi, total_reward, steps / own_v, goal_x, goal_y, episode -- and so are the traffic arrays -- trf_x, trf_y /
// trf_psi, trf_v ([k][E][N]).  Five preloaded base pointers (the four blocks and the actions) then name every input of
// the step, and ALL of a wavefront's loads leave before its first scalar-load round trip (Mode::Arena).
// `ACAS2DVecEnv` allocates its float32 state this way.  The kernel also assumes full waves in whole multiples of eight
// workgroups (n_envs a multiple of 1 024 at n_traffic = 8); any other layout or size takes the general kernel, same results.
template <typename T>
static bool arena_layout(const State<T>& s, int64_t E, int N, int G) {
    if (sizeof(T) != 4 || getenv("ACAS2D_NO_ARENA")) return false;
    if (E % ((64 / G) * kWavesPerBlock * 8) != 0) return false;            // whole multiples of eight workgroups (full waves)
    const int64_t EN = E * N;
    if (8 * EN >= (1LL << 32) || 20 * E >= (1LL << 32)) return false;      // the kernel's 32-bit byte offsets
    return s.own_y == s.own_x + E && s.own_psi == s.own_x + 2 * E && s.total_reward == s.own_x + 3 * E &&
           (const void*)s.steps == (const void*)(s.own_x + 4 * E) &&
           s.goal_x == s.own_v + E && s.goal_y == s.own_v + 2 * E && (const void*)s.episode == (const void*)(s.own_v + 3 * E) &&
           s.trf_y == s.trf_x + EN && s.trf_v == s.trf_psi + EN;
}

// The one map from a runtime Shape to an instantiation: calls f(C, G, PACKED), as integral_constants, for the shape of
// ACAS2D_PACKED_SHAPES or of the generic walk (C = 1, G lanes per env) that sh names; false when none does.
template <typename F>
static bool visit_shape(const Shape& sh, F f) {
    bool found = false;
    const auto at = [&](auto C, auto G, auto packed) {
        if (sh.packed == packed && sh.C == C && sh.G == G) { f(C, G, packed); found = true; }
    };
#define X(C_, G_) at(std::integral_constant<int, C_>{}, std::integral_constant<int, G_>{}, std::true_type{});
    ACAS2D_PACKED_SHAPES(X)
#undef X
#define X(G_) at(std::integral_constant<int, 1>{}, std::integral_constant<int, G_>{}, std::false_type{});
    X(1) X(4) X(16) X(64)                                   // the generic walk
#undef X
    return found;
}

static bool shape_instantiated(const Shape& sh) { return visit_shape(sh, [](auto, auto, auto) {}); }

// Formulation: the element type's own -- FAST for float32, EXACT for float64 -- unless the
// configuration asks for ACAS2D_MATH_FAST, which gives the float64 entry points the algebraic formulation in
// float64 arithmetic (float32 has no other).  Chosen per call; nothing is cached between calls.  Calls
// f(FAST, C, G, PACKED) for that formulation and the instantiated shape sh.
template <typename F>
static void dispatch(const Acas2dConfig& cfg, const Shape& sh, F f) {
    const auto with = [&](auto fast) { visit_shape(sh, [&](auto C, auto G, auto packed) { f(fast, C, G, packed); }); };
    if (kFast || cfg.math == ACAS2D_MATH_FAST) with(std::true_type{});
    else with(std::integral_constant<bool, kFast>{});
}

// Shape for (n_traffic, element type): the tuned default of choose_shape(), or the override
// ACAS2D_SHAPE="C,G" (packed, needs C*G == n_traffic) / "generic,G" from the environment.
template <typename T>
static int resolve_shape(int n_traffic, Shape* out) {
    Shape sh = choose_shape(n_traffic, (int)sizeof(T));
    if (const char* ov = getenv("ACAS2D_SHAPE")) {
        int a = 0, b = 0;
        if (sscanf(ov, "generic,%d", &b) == 1) sh = Shape{1, b, false};
        else if (sscanf(ov, "%d,%d", &a, &b) == 2) sh = Shape{a, b, true};
        if (sh.packed && sh.C * sh.G != n_traffic) { set_error("ACAS2D_SHAPE=%s does not tile n_traffic=%d", ov, n_traffic); return ACAS2D_EINVAL; }
    }
    if (!shape_instantiated(sh)) {
        if (sh.packed) sh = Shape{1, n_traffic >= 64 ? 64 : (n_traffic >= 16 ? 16 : (n_traffic >= 4 ? 4 : 1)), false};
        if (!shape_instantiated(sh)) { set_error("no kernel for shape C=%d G=%d", sh.C, sh.G); return ACAS2D_EINVAL; }
    }
    *out = sh;
    return ACAS2D_OK;
}

template <typename... A>
static int fail(const char* fmt, A... a) {
    set_error(fmt, a...);
    return ACAS2D_EINVAL;
}

// One entry point's launch: its arguments (the first block, set by the entry point), then what prepare() derives.
template <typename T>
struct Launch {
    const char* name;                         // the entry point, as its messages name it
    const Acas2dConfig* cfg;
    const Acas2dState* st;
    const Acas2dStepIO* step_io;              // NULL where the entry point takes no StepIO
    uint64_t seed;
    int64_t env_offset, n_envs;
    int32_t N, n_steps;                       // n_steps = 1 for the per-step entry points
    hipStream_t stream;
    Shape sh;
    Geometry g;
    Params<T> p;
    State<T> s;
    StepIO<T> io;
    uint32_t k0, k1;
    bool group_policy;                        // the *_group entry points: geometry_for()'s hidden vectors
    bool correlated;                          // the *_correlated entry points: geometry_for()'s error state, 3 C + 1 per lane
    bool delayed;                             // the *_delayed entry points: one value more per lane, the lag's state
};

// The entry points' words for the rejections they share (each has always said them its own way)
struct Words {
    const char* nulls;                        // the pointers the first check names next to cfg
    const char* sizes;                        // n_traffic or n_steps < 1 (printf: name, n_traffic, n_steps)
    const char* negative;                     // a negative n_envs / env_offset
};
static const char kSizes[] = "%s: n_traffic = %d, n_steps = %d", kNegative[] = "%s: negative n_envs / env_offset";

// The checks every entry point shares, in the order each one runs them, and the launch arguments they share.  The
// entry point's own parts: `given` (the pointers of words.nulls are there), inputs() (its buffers), shape() (its work
// shape; its own shape checks) and go() (its checks that need the launch arguments, then the launch).
template <typename T, typename Inputs, typename PickShape, typename Go>
static int prepare(Launch<T>& L, const Words& words, bool given, Inputs inputs, PickShape shape, Go go) {
    if (!L.cfg || !given) return fail("%s: NULL %s", L.name, words.nulls);
    if (!state_complete(L.st)) return fail("%s: NULL state or a NULL state buffer", L.name);
    if (int rc = inputs()) return rc;
    if (L.N < 1 || L.n_steps < 1) return fail(words.sizes, L.name, L.N, L.n_steps);
    if (L.n_envs < 0 || L.env_offset < 0) return fail(words.negative, L.name);
    if (L.n_envs == 0) return ACAS2D_OK;
    if (int rc = shape(&L.sh)) return rc;
    if (int rc = geometry_for<T>(L.sh, L.n_envs, L.N, &L.g, L.group_policy, L.correlated ? kCorrSlots(L.sh.C) + (L.delayed ? 1 : 0) : 0)) return rc;
    L.p = make_params<T>(*L.cfg);
    L.s = make_state<T>(*L.st);
    if (const Acas2dStepIO* io = L.step_io)
        L.io = StepIO<T>{(const T*)io->actions, (T*)io->obs, (T*)io->reward, io->done, io->outcome, (T*)io->term_obs,
                         (T*)io->ep_return, io->ep_steps};
    L.k0 = (uint32_t)L.seed; L.k1 = (uint32_t)(L.seed >> 32);
    if (int rc = go()) return rc;
    return check_launch(L.name);
}

static int require_io(const char* name, const Acas2dStepIO* io) {
    if (io->actions && io->obs && io->reward && io->done && io->outcome) return ACAS2D_OK;
    return fail("%s: actions, obs, reward, done and outcome are required", name);
}
static int require_actor(const char* name, const Acas2dPolicy* pol) {
    if (pol->w1t && pol->b1 && pol->w2t && pol->b2 && pol->w3 && pol->b3 && pol->hidden == kPolicyHidden) return ACAS2D_OK;
    return fail("%s: six weight buffers and hidden == %d are required (got hidden = %d)", name, kPolicyHidden, pol->hidden);
}
// the in-kernel policy's work shape: one lane per env, its traffic as one vector
static int thread_per_env(const char* name, int n_traffic, Shape* sh) {
    *sh = Shape{n_traffic, 1, true};
    if (shape_instantiated(*sh)) return ACAS2D_OK;
    return fail("%s: n_traffic = %d has no thread-per-env shape for this element type", name, n_traffic);
}
// the *_group entry points' work shape: the default of resolve_shape(), which must be one of the four shapes the
// group-cooperative policy is built for.  `sibling`: the entry point that serves the thread-per-env counts.
template <typename T>
static int group_shape(const char* name, const char* sibling, int n_traffic, Shape* sh) {
    static const char kBuilt[] = "the group-cooperative policy is built for n_traffic in {8, 16, 32, 64}, float32 "
                                 "(work shapes (4,2) (4,4) (4,8) (4,16))";
    if (int rc = resolve_shape<T>(n_traffic, sh)) return rc;
    if (sizeof(T) == 4 && sh->packed && group_policy_shape(sh->C, sh->G)) return ACAS2D_OK;
    if (sizeof(T) == 4 && sh->packed && sh->G == 1)
        return fail("%s: n_traffic = %d takes the thread-per-env shape C=%d G=1: use %s; %s", name, n_traffic, sh->C, sibling, kBuilt);
    if (!sh->packed) return fail("%s: n_traffic = %d has no packed work shape; %s", name, n_traffic, kBuilt);
    return fail("%s: n_traffic = %d takes the work shape C=%d G=%d; %s", name, n_traffic, sh->C, sh->G, kBuilt);
}
// ... and its weights: a lane reads its slice of a weight row as 16-byte vectors
static int require_aligned(const char* name, std::initializer_list<const void*> ptrs) {
    for (const void* q : ptrs)
        if (reinterpret_cast<uintptr_t>(q) & 15u)
            return fail("%s: the first two layers' weights and biases must be 16-byte aligned", name);
    return ACAS2D_OK;
}

// The kernel of a launch: step_kernel in mode M, unless the launch's policy argument is one of the ten that have a kernel
// of their own (Mode::Eval with statistics, the Monte Carlo campaign, the disturbed, the correlated and the delayed flavour of
// each, the disturbed and the correlated set collector; packed shapes)
template <typename PW, typename T, int C, int G, bool PACKED, bool FAST, Mode M>
static constexpr auto kernel_for() {
    if constexpr (std::is_same<PW, PolicyCollectCorrW>::value) return &collect_set_correlated_kernel<T, C, G, FAST>;
    else if constexpr (std::is_same<PW, PolicyCollectDistW>::value) return &collect_set_disturbed_kernel<T, C, G, FAST>;
    else if constexpr (std::is_same<PW, PolicyMonteCarloRespW>::value) return &monte_carlo_delayed_kernel<T, C, G, FAST>;
    else if constexpr (std::is_same<PW, PolicyEvalStatsRespW>::value) return &eval_stats_delayed_kernel<T, C, G, FAST>;
    else if constexpr (std::is_same<PW, PolicyMonteCarloCorrW>::value) return &monte_carlo_correlated_kernel<T, C, G, FAST>;
    else if constexpr (std::is_same<PW, PolicyEvalStatsCorrW>::value) return &eval_stats_correlated_kernel<T, C, G, FAST>;
    else if constexpr (std::is_same<PW, PolicyMonteCarloDistW>::value) return &monte_carlo_disturbed_kernel<T, C, G, FAST>;
    else if constexpr (std::is_same<PW, PolicyEvalStatsDistW>::value) return &eval_stats_disturbed_kernel<T, C, G, FAST>;
    else if constexpr (std::is_same<PW, PolicyMonteCarloW>::value) return &monte_carlo_kernel<T, C, G, FAST>;
    else if constexpr (std::is_same<PW, PolicyEvalStatsW>::value) return &eval_stats_kernel<T, C, G, FAST>;
    else return &step_kernel<T, C, G, PACKED, FAST, M>;
}

// One launch in mode M for L's shape and formulation.  The six preloaded pointers (see step_kernel): the
// arena mode's four state blocks and the actions, else the traffic arrays, own_x and own_y.
template <Mode M, typename T, typename PW>
static int launch_mode(const Launch<T>& L, const PW& pw) {
    const StepResetParams<T, rollout_mode(M)> rp = make_reset_params<T, rollout_mode(M)>(*L.cfg);
    const State<T>& s = L.s;
    const T* const general[6] = {s.trf_x, s.trf_y, s.trf_psi, s.trf_v, s.own_x, s.own_y};
    const T* const arena[6] = {s.own_x, s.own_v, s.trf_x, s.trf_psi, L.io.actions, nullptr};
    const T* const* a = M == Mode::Arena ? arena : general;
    dispatch(*L.cfg, L.sh, [&](auto fast, auto C, auto G, auto packed) {
        if constexpr ((M != Mode::Arena || (packed && sizeof(T) == 4)) && (!rollout_mode(M) || packed) &&
                      (!policy_mode(M) || G == 1 || (sizeof(T) == 4 && packed && group_policy_shape(C, G))) &&
                      (M != Mode::CollectSet || sizeof(T) == 4)) {
            hipLaunchKernelGGL((kernel_for<PW, T, C, G, packed, fast, M>()), dim3(L.g.grid), dim3(L.g.block), L.g.lds_bytes,
                               L.stream, a[0], a[1], a[2], a[3], a[4], a[5], (int32_t)L.n_envs, (int32_t)L.g.tile_elems,
                               L.p, rp, s, L.io, L.k0, L.k1, L.env_offset, L.N, L.n_steps, pw);
        }
    });
    return ACAS2D_OK;
}

template <typename T>
int launch_step(const Acas2dConfig* cfg, const Acas2dState* st, const Acas2dState* st_out, const Acas2dStepIO* io, uint32_t flags,
                uint64_t seed, int64_t env_offset, int64_t n_envs, int32_t n_traffic, hipStream_t stream) {
    Launch<T> L{"acas2d_step", cfg, st, io, seed, env_offset, n_envs, n_traffic, 1, stream};
    const auto go = [&] {
        const bool ar = (flags & ACAS2D_AUTO_RESET) != 0;
        if (int rc = write_offsets<T>(st, st_out, ar, n_envs, n_traffic, &L.s.w_env, &L.s.w_trf)) return rc;
        if (!ar) return launch_mode<Mode::Latch>(L, PolicyW{});
        if (L.sh.packed && arena_layout<T>(L.s, n_envs, n_traffic, L.sh.G)) return launch_mode<Mode::Arena>(L, PolicyW{});
        return launch_mode<Mode::Step>(L, PolicyW{});
    };
    return prepare(L, Words{"cfg / io", "%s: n_traffic = %d (the reference needs traffic[0], game.py:254)", kNegative},
                   io != nullptr, [&] { return require_io(L.name, io); },
                   [&](Shape* sh) { return resolve_shape<T>(n_traffic, sh); }, go);
}

template <typename T>
int launch_rollout(const Acas2dConfig* cfg, const Acas2dState* st, const Acas2dStepIO* io, int32_t n_steps,
                   uint64_t seed, int64_t env_offset, int64_t n_envs, int32_t n_traffic, hipStream_t stream) {
    Launch<T> L{"acas2d_rollout", cfg, st, io, seed, env_offset, n_envs, n_traffic, n_steps, stream};
    const auto shape = [&](Shape* sh) {
        if (int rc = resolve_shape<T>(n_traffic, sh)) return rc;
        if (sh->packed) return ACAS2D_OK;
        return fail("acas2d_rollout: n_traffic = %d has no packed work shape for this element type "
                    "(needs n_traffic in {1,2,3} or a multiple of %d tiling a wave); use acas2d_step", n_traffic,
                    16 / (int)sizeof(T));
    };
    return prepare(L, Words{"cfg / io", kSizes, kNegative}, io != nullptr, [&] { return require_io(L.name, io); }, shape,
                   [&] { return launch_mode<Mode::Rollout>(L, PolicyW{}); });
}

// the actor's weights and the observation its first action is taken on (policy and evaluation launches)
template <typename PW>
static PW actor(const Acas2dPolicy* pol, const void* obs_in) {
    PW pw{};
    pw.w1t = (const float*)pol->w1t; pw.b1 = (const float*)pol->b1; pw.w2t = (const float*)pol->w2t;
    pw.b2 = (const float*)pol->b2; pw.w3 = (const float*)pol->w3; pw.b3 = (const float*)pol->b3;
    pw.obs_in = obs_in;
    return pw;
}

// ... and what the collectors add: the value net, log_std, the per-step value / log-probability outputs and the noise stream,
// `key` its 64-bit key (acas2d_collect_*) or the address of the members' keys (acas2d_collect_set_*)
static void sample_with(PolicyW& pw, const Acas2dActorCritic* ac, uint64_t key) {
    pw.v1t = (const float*)ac->v1t; pw.vb1 = (const float*)ac->vb1; pw.v2t = (const float*)ac->v2t;
    pw.vb2 = (const float*)ac->vb2; pw.v3 = (const float*)ac->v3; pw.vb3 = (const float*)ac->vb3;
    pw.log_std = (const float*)ac->log_std; pw.values_out = ac->values; pw.logp_out = ac->logp;
    pw.nk0 = (uint32_t)key; pw.nk1 = (uint32_t)(key >> 32); pw.noise_step = ac->noise_step;
}

// acas2d_rollout_policy_* and, with the actor-critic, acas2d_collect_* (which words most rejections as the former)
template <typename T>
static int launch_policy(const Acas2dConfig* cfg, const Acas2dState* st, const Acas2dStepIO* io, const Acas2dPolicy* pol,
                         const void* obs_in, int32_t n_steps, uint64_t seed, int64_t env_offset, int64_t n_envs,
                         int32_t n_traffic, hipStream_t stream, const Acas2dActorCritic* ac, bool group = false) {
    Launch<T> L{group ? "acas2d_rollout_policy_group" : "acas2d_rollout_policy", cfg, st, io, seed, env_offset, n_envs, n_traffic,
                n_steps, stream};
    L.group_policy = group;
    const auto inputs = [&] {
        if (!io->actions || !io->obs || !io->reward || !io->done || !io->outcome || !obs_in)
            return fail("%s: obs_in, actions (output), obs, reward, done and outcome are required", L.name);
        return require_actor(L.name, pol);
    };
    const auto go = [&] {
        PolicyW pw = actor<PolicyW>(pol, obs_in);
        pw.actions_out = const_cast<void*>(io->actions);
        if (group)
            if (int rc = require_aligned(L.name, {pol->w1t, pol->b1, pol->w2t, pol->b2})) return rc;
        if (!ac) return launch_mode<Mode::Policy>(L, pw);
        if (!ac->v1t || !ac->vb1 || !ac->v2t || !ac->vb2 || !ac->v3 || !ac->vb3 || !ac->log_std || !ac->values || !ac->logp)
            return fail("acas2d_collect: the value net, log_std, values and logp are required");
        if (group)
            if (int rc = require_aligned(L.name, {ac->v1t, ac->vb1, ac->v2t, ac->vb2})) return rc;
        sample_with(pw, ac, ac->noise_seed);
        return launch_mode<Mode::Collect>(L, pw);
    };
    const auto shape = [&](Shape* sh) {
        if (group) return group_shape<T>(L.name, ac ? "acas2d_collect_f32" : "acas2d_rollout_policy_f32", n_traffic, sh);
        return thread_per_env(L.name, n_traffic, sh);
    };
    return prepare(L, Words{"cfg / io / policy", kSizes, kNegative}, io && pol, inputs, shape, go);
}
template <typename T>
int launch_rollout_policy(const Acas2dConfig* cfg, const Acas2dState* st, const Acas2dStepIO* io,
                          const Acas2dPolicy* pol, const void* obs_in, int32_t n_steps, uint64_t seed,
                          int64_t env_offset, int64_t n_envs, int32_t n_traffic, hipStream_t stream) {
    return launch_policy<T>(cfg, st, io, pol, obs_in, n_steps, seed, env_offset, n_envs, n_traffic, stream, nullptr);
}
template <typename T>
int launch_collect(const Acas2dConfig* cfg, const Acas2dState* st, const Acas2dStepIO* io, const Acas2dActorCritic* ac,
                   const void* obs_in, int32_t n_steps, uint64_t seed, int64_t env_offset, int64_t n_envs,
                   int32_t n_traffic, hipStream_t stream) {
    if (!ac) return fail("acas2d_collect: NULL actor-critic");
    return launch_policy<T>(cfg, st, io, &ac->actor, obs_in, n_steps, seed, env_offset, n_envs, n_traffic, stream, ac);
}
// the *_group entry points: the same launches at the shapes whose G lanes evaluate an env's policy together
template <typename T>
int launch_rollout_policy_group(const Acas2dConfig* cfg, const Acas2dState* st, const Acas2dStepIO* io,
                                const Acas2dPolicy* pol, const void* obs_in, int32_t n_steps, uint64_t seed,
                                int64_t env_offset, int64_t n_envs, int32_t n_traffic, hipStream_t stream) {
    return launch_policy<T>(cfg, st, io, pol, obs_in, n_steps, seed, env_offset, n_envs, n_traffic, stream, nullptr, true);
}
template <typename T>
int launch_collect_group(const Acas2dConfig* cfg, const Acas2dState* st, const Acas2dStepIO* io, const Acas2dActorCritic* ac,
                         const void* obs_in, int32_t n_steps, uint64_t seed, int64_t env_offset, int64_t n_envs,
                         int32_t n_traffic, hipStream_t stream) {
    if (!ac) return fail("acas2d_collect: NULL actor-critic");
    return launch_policy<T>(cfg, st, io, &ac->actor, obs_in, n_steps, seed, env_offset, n_envs, n_traffic, stream, ac, true);
}

// acas2d_collect_set_f32: acas2d_collect_* for K stacked actor-critics, member k on the envs [k EM, (k + 1) EM) with
// EM = n_envs / K a multiple of the wave, so that the member is wave-uniform.  float32, one lane per env -- or, `group`
// (acas2d_collect_set_group_f32), the env's G lanes together at the shapes of group_shape(): a wave then holds 64 / G envs,
// and the same rule for EM keeps them one member's.
// DIST (acas2d_collect_set_disturbed_f32, acas2d_collect_set_disturbed_group_f32; collect_set_disturbed_kernel): the same launch
// under sensor and actuator noise, `cd` its three arguments.  One member then takes any n_envs >= 1: it is the solo collector.
// CORR on top (acas2d_collect_set_correlated_f32, acas2d_collect_set_correlated_group_f32; collect_set_correlated_kernel): the
// noise a Gauss-Markov error whose state lives in `held` between launches, `cd`'s last two arguments; its rejections stand
// behind everything the disturbed entry rejects: in go(), after the shape, geometry_for() and the alignment.
struct CollectDisturbance { const float* sigmas; uint64_t seed; void* obs_read; const float* correlations; float* held; };
template <typename T, bool DIST, bool CORR = false>
static int collect_set(const Acas2dConfig* cfg, const Acas2dState* st, const Acas2dStepIO* io, const Acas2dActorCritic* ac,
                       int32_t n_members, const uint64_t* noise_seeds, const void* obs_in, int32_t n_steps, uint64_t seed,
                       int64_t env_offset, int64_t n_envs, int32_t n_traffic, hipStream_t stream, bool group,
                       const CollectDisturbance& cd = CollectDisturbance{}) {
    static_assert(sizeof(T) == 4, "acas2d_collect_set: float32 only");
    static_assert(!CORR || DIST, "the correlated collector: on top of the disturbed one");
    static const char kScope[] = "float32, n_traffic in {1, 2, 3, 4, 8}; n_traffic 16 / 32 / 64 is acas2d_collect_set_group_f32, "
                                 "float64 collects one learner per call";
    Launch<T> L{CORR ? (group ? "acas2d_collect_set_correlated_group" : "acas2d_collect_set_correlated")
                : DIST ? (group ? "acas2d_collect_set_disturbed_group" : "acas2d_collect_set_disturbed")
                       : (group ? "acas2d_collect_set_group" : "acas2d_collect_set"), cfg, st, io, seed, env_offset, n_envs, n_traffic,
                n_steps, stream};
    L.group_policy = group;
    L.correlated = CORR;
    const auto inputs = [&] {
        if (!io->actions || !io->obs || !io->reward || !io->done || !io->outcome || !obs_in)
            return fail("%s: obs_in, actions (output), obs, reward, done and outcome are required", L.name);
        if (int rc = require_actor(L.name, &ac->actor)) return rc;
        if (!ac->v1t || !ac->vb1 || !ac->v2t || !ac->vb2 || !ac->v3 || !ac->vb3 || !ac->log_std || !ac->values || !ac->logp)
            return fail("%s: the value net's stacks, log_std, values and logp are required", L.name);
        if (!noise_seeds) return fail("%s: NULL noise_seeds (one 64-bit key per member, on the device)", L.name);
        if (n_members < 1) return fail("%s: n_members = %d (at least 1)", L.name, n_members);
        if (n_envs >= 0 && !(DIST && n_members == 1) && (n_envs % n_members != 0 || (n_envs / n_members) % 64 != 0))
            return fail("%s: n_envs = %lld is not n_members = %d x a multiple of 64 (a wavefront's envs belong to ONE member)",
                        L.name, (long long)n_envs, n_members);
        if constexpr (DIST) {
            if (!cd.sigmas || !cd.obs_read)
                return fail("%s: NULL sigmas (float[n_members][4], on the device) or obs_read", L.name);
            if (n_envs > 0 && n_steps >= 1 && n_traffic >= 1) {      // (else: rejected or empty below)
                const uint64_t row = (uint64_t)n_envs * (uint64_t)(5 + 3 * (int64_t)n_traffic) * sizeof(T);
                const uintptr_t w0 = (uintptr_t)cd.obs_read, w1 = w0 + (uintptr_t)(row * ((uint64_t)n_steps + 1u));
                const auto meets = [&](const void* q, uint64_t bytes) { return w0 < (uintptr_t)q + (uintptr_t)bytes && (uintptr_t)q < w1; };
                if (meets(io->obs, row * (uint64_t)n_steps) || meets(obs_in, row))
                    return fail("%s: obs_read overlaps io->obs or obs_in (the true observations stay what they are)", L.name);
            }
            if ((int64_t)cfg->max_steps + 1 >= (1ll << kDisturbanceSlotShift))
                return fail("%s: max_steps = %d (max_steps + 1 must stay below 2^%d, the step field of the noise counter)", L.name,
                            cfg->max_steps, kDisturbanceSlotShift);
        }
        return ACAS2D_OK;
    };
    const auto shape = [&](Shape* sh) {
        if (group) return group_shape<T>(L.name, "acas2d_collect_set_f32", n_traffic, sh);
        *sh = Shape{n_traffic, 1, true};
        if (shape_instantiated(*sh)) return ACAS2D_OK;
        return fail("%s: n_traffic = %d has no thread-per-env shape (%s)", L.name, n_traffic, kScope);
    };
    const auto go = [&] {
        PolicyW pw = actor<PolicyW>(&ac->actor, obs_in);
        pw.actions_out = const_cast<void*>(io->actions);
        if (group)      // (a member's slice lies a multiple of 256 bytes behind the stack's base: the base decides)
            if (int rc = require_aligned(L.name, {ac->actor.w1t, ac->actor.b1, ac->actor.w2t, ac->actor.b2, ac->v1t, ac->vb1,
                                                  ac->v2t, ac->vb2})) return rc;
        if constexpr (CORR) {
            // its own rejections, behind EVERYTHING the disturbed sibling rejects (the work shape, the launch and LDS limits and
            // the group entries' alignment included), as the correlated evaluator checks its correlation last of all
            if (!cd.correlations) return fail("%s: NULL correlations (float[n_members][8], on the device)", L.name);
            if (!cd.held) return fail("%s: NULL held (float[3 n_traffic + 1][n_envs], on the device)", L.name);
            const uint64_t row = (uint64_t)n_envs * (uint64_t)(5 + 3 * (int64_t)n_traffic) * sizeof(T);
            const uintptr_t w0 = (uintptr_t)cd.held,
                            w1 = w0 + (uintptr_t)((uint64_t)n_envs * (uint64_t)(3 * (int64_t)n_traffic + 1) * sizeof(float));
            const auto meets = [&](const void* q, uint64_t bytes) { return w0 < (uintptr_t)q + (uintptr_t)bytes && (uintptr_t)q < w1; };
            if (meets(cd.obs_read, row * ((uint64_t)n_steps + 1u)) || meets(io->obs, row * (uint64_t)n_steps) || meets(obs_in, row))
                return fail("%s: held overlaps obs_read, io->obs or obs_in", L.name);
        }
        sample_with(pw, ac, (uint64_t)reinterpret_cast<uintptr_t>(noise_seeds));       // the kernel loads its member's key
        pw.member_stride = (uint32_t)(n_envs / n_members);
        if constexpr (CORR) {
            PolicyCollectCorrW pc{};
            static_cast<PolicyW&>(pc) = pw;
            pc.dist = CollectDistW{cd.sigmas, cd.obs_read, (uint32_t)cd.seed, (uint32_t)(cd.seed >> 32)};
            pc.corr = CollectCorrW{cd.correlations, cd.held};
            return launch_mode<Mode::CollectSet>(L, pc);
        } else if constexpr (DIST) {
            PolicyCollectDistW pd{};
            static_cast<PolicyW&>(pd) = pw;
            pd.dist = CollectDistW{cd.sigmas, cd.obs_read, (uint32_t)cd.seed, (uint32_t)(cd.seed >> 32)};
            return launch_mode<Mode::CollectSet>(L, pd);
        } else {
            return launch_mode<Mode::CollectSet>(L, pw);
        }
    };
    return prepare(L, Words{"cfg / io / actor-critic", kSizes, kNegative}, io && ac, inputs, shape, go);
}
template <typename T>
int launch_collect_set(const Acas2dConfig* cfg, const Acas2dState* st, const Acas2dStepIO* io, const Acas2dActorCritic* ac,
                       int32_t n_members, const uint64_t* noise_seeds, const void* obs_in, int32_t n_steps, uint64_t seed,
                       int64_t env_offset, int64_t n_envs, int32_t n_traffic, hipStream_t stream) {
    return collect_set<T, false>(cfg, st, io, ac, n_members, noise_seeds, obs_in, n_steps, seed, env_offset, n_envs, n_traffic, stream,
                                 false);
}
template <typename T>
int launch_collect_set_group(const Acas2dConfig* cfg, const Acas2dState* st, const Acas2dStepIO* io, const Acas2dActorCritic* ac,
                             int32_t n_members, const uint64_t* noise_seeds, const void* obs_in, int32_t n_steps, uint64_t seed,
                             int64_t env_offset, int64_t n_envs, int32_t n_traffic, hipStream_t stream) {
    return collect_set<T, false>(cfg, st, io, ac, n_members, noise_seeds, obs_in, n_steps, seed, env_offset, n_envs, n_traffic, stream,
                                 true);
}
template <typename T>
int launch_collect_set_disturbed(const Acas2dConfig* cfg, const Acas2dState* st, const Acas2dStepIO* io, const Acas2dActorCritic* ac,
                                 int32_t n_members, const uint64_t* noise_seeds, const void* obs_in, int32_t n_steps, uint64_t seed,
                                 int64_t env_offset, int64_t n_envs, int32_t n_traffic, const float* sigmas, uint64_t dist_seed,
                                 void* obs_read, hipStream_t stream, bool group) {
    return collect_set<T, true>(cfg, st, io, ac, n_members, noise_seeds, obs_in, n_steps, seed, env_offset, n_envs, n_traffic, stream,
                                group, CollectDisturbance{sigmas, dist_seed, obs_read});
}
template <typename T>
int launch_collect_set_correlated(const Acas2dConfig* cfg, const Acas2dState* st, const Acas2dStepIO* io, const Acas2dActorCritic* ac,
                                  int32_t n_members, const uint64_t* noise_seeds, const void* obs_in, int32_t n_steps, uint64_t seed,
                                  int64_t env_offset, int64_t n_envs, int32_t n_traffic, const float* sigmas, uint64_t dist_seed,
                                  void* obs_read, const float* correlations, float* held, hipStream_t stream, bool group) {
    return collect_set<T, true, true>(cfg, st, io, ac, n_members, noise_seeds, obs_in, n_steps, seed, env_offset, n_envs, n_traffic,
                                      stream, group, CollectDisturbance{sigmas, dist_seed, obs_read, correlations, held});
}

// what the disturbed entries check on top of their siblings (after them: cfg is there), and the kernels' view of the struct
static int check_disturbance(const char* name, const Acas2dConfig* cfg, const Acas2dDisturbance* d) {
    if (!d) return fail("%s: NULL disturbance", name);
    const float sd[4] = {d->s_sep, d->s_cpa, d->s_closing, d->s_action};
    for (float v : sd)
        if (!(v >= 0.0f) || !(v < __builtin_inff()))
            return fail("%s: s_sep = %g, s_cpa = %g, s_closing = %g, s_action = %g (each finite and at least 0)", name,
                        (double)sd[0], (double)sd[1], (double)sd[2], (double)sd[3]);
    if ((int64_t)cfg->max_steps + 1 >= (1ll << kDisturbanceSlotShift))
        return fail("%s: max_steps = %d (max_steps + 1 must stay below 2^%d, the step field of the noise counter)", name,
                    cfg->max_steps, kDisturbanceSlotShift);
    return ACAS2D_OK;
}
static DisturbW disturbance_words(const Acas2dDisturbance& d) {
    return DisturbW{d.s_sep, d.s_cpa, d.s_closing, d.s_action, (uint32_t)d.noise_seed, (uint32_t)(d.noise_seed >> 32), d.noise_episode};
}
// ... and the correlated entries on top of the disturbed ones (behind EVERYTHING those reject), with the gains
static int check_correlation(const char* name, const Acas2dCorrelation* c) {
    if (!c) return fail("%s: NULL correlation", name);
    const float rho[4] = {c->rho_sep, c->rho_cpa, c->rho_closing, c->rho_action};
    for (float v : rho)
        if (!(v >= 0.0f) || !(v <= 1.0f))
            return fail("%s: rho_sep = %g, rho_cpa = %g, rho_closing = %g, rho_action = %g (each in [0, 1])", name,
                        (double)rho[0], (double)rho[1], (double)rho[2], (double)rho[3]);
    return ACAS2D_OK;
}
// ... and the delayed entries on top of the correlated ones, last of all: `total` is the launch's env count, n_policies x EP
static int check_response(const char* name, const Acas2dResponse* r, int64_t total) {
    if (!r) return fail("%s: NULL response", name);
    if (r->delay_steps < 0 || r->delay_steps > 32767)
        return fail("%s: delay_steps = %d (0 to 32767)", name, r->delay_steps);
    if (!(r->lag >= 0.0f) || !(r->lag <= 1.0f)) return fail("%s: lag = %g (in [0, 1])", name, (double)r->lag);
    if (r->delay_steps > 0 && !r->ring)
        return fail("%s: NULL ring with delay_steps = %d (float[delay_steps][ring_envs], on the device)", name, r->delay_steps);
    if (r->delay_steps > 0 && r->ring_envs < total)
        return fail("%s: ring_envs = %lld, the launch covers %lld envs", name, (long long)r->ring_envs, (long long)total);
    return ACAS2D_OK;
}
static RespW response_words(const Acas2dResponse& r) {
    return RespW{r.delay_steps, r.lag, (float)(1.0 - (double)r.lag), r.ring, r.ring_envs};
}
static CorrW correlation_words(const Acas2dCorrelation& c) {
    const auto gain = [](float rho) { return (float)std::sqrt(1.0 - (double)rho * (double)rho); };
    return CorrW{c.rho_sep, c.rho_cpa, c.rho_closing, c.rho_action,
                 gain(c.rho_sep), gain(c.rho_cpa), gain(c.rho_closing), gain(c.rho_action)};
}

// ---- the policy-scoring family: acas2d_evaluate_policies_* and acas2d_monte_carlo_* ------------------------------------------
// K stacked policies on shared work: policy k plays envs [k EP, (k + 1) EP) of the state, EP = n_per_policy (the evaluator's
// n_episodes, the campaign's n_lanes) rounded up to a whole wave; the launch covers those n_policies x EP envs in Mode::Eval.
// An entry's words: what its messages call it (alone / as the *_group entry), the thread-per-env entry its *_group one sends
// the small traffic counts to, what its family calls n_per_policy, and who says "the state holds" (NULL: the entry itself;
// the evaluator's entries have always said that one under the plain entry's name).
struct ScoringWords { const char *name, *group_name, *sibling, *count, *holds; };
static const ScoringWords kEvaluateWords[] = {             // [Scoring]
    {"acas2d_evaluate_policies", "acas2d_evaluate_policies_group", "acas2d_evaluate_policies_f32", "n_episodes",
     "acas2d_evaluate_policies"},
    {"acas2d_evaluate_policies_stats", "acas2d_evaluate_policies_stats_group", "acas2d_evaluate_policies_stats_f32", "n_episodes",
     "acas2d_evaluate_policies"},
    {"acas2d_evaluate_policies_disturbed", "acas2d_evaluate_policies_disturbed_group", "acas2d_evaluate_policies_disturbed_f32",
     "n_episodes", "acas2d_evaluate_policies"},
    {"acas2d_evaluate_policies_correlated", "acas2d_evaluate_policies_correlated_group", "acas2d_evaluate_policies_correlated_f32",
     "n_episodes", "acas2d_evaluate_policies"},
    {"acas2d_evaluate_policies_delayed", "acas2d_evaluate_policies_delayed_group", "acas2d_evaluate_policies_delayed_f32",
     "n_episodes", "acas2d_evaluate_policies"}};
static const ScoringWords kMonteCarloWords[] = {           // [plain, disturbed, correlated, delayed]
    {"acas2d_monte_carlo", "acas2d_monte_carlo_group", "acas2d_monte_carlo_f32", "n_lanes", nullptr},
    {"acas2d_monte_carlo_disturbed", "acas2d_monte_carlo_disturbed_group", "acas2d_monte_carlo_disturbed_f32", "n_lanes", nullptr},
    {"acas2d_monte_carlo_correlated", "acas2d_monte_carlo_correlated_group", "acas2d_monte_carlo_correlated_f32", "n_lanes", nullptr},
    {"acas2d_monte_carlo_delayed", "acas2d_monte_carlo_delayed_group", "acas2d_monte_carlo_delayed_f32", "n_lanes", nullptr}};

// Everything the two share, around their own parts: nulls(name), the family's required pointers; own(name), its checks
// behind the counts' and in front of the disturbance's; fill(pw), its fields of the kernel's last argument PW -- which
// picks the kernel (kernel_for()).  A PW with a CorrW is a correlated entry's: `corr` is checked last of all -- but for `resp`,
// which a PW with a RespW (a delayed entry's) checks behind it.
template <typename T, typename PW, bool DIST, typename Nulls, typename Own, typename Fill>
static int score(const ScoringArgs& a, const ScoringWords& w, const Acas2dDisturbance* dist, const Acas2dCorrelation* corr,
                 const Acas2dResponse* resp, Nulls nulls, Own own, Fill fill) {
    static_assert(!DIST || sizeof(T) == 4, "the disturbed flavours: float32");
    constexpr bool CORR = std::is_base_of<PolicyEvalStatsCorrW, PW>::value || std::is_base_of<PolicyMonteCarloCorrW, PW>::value;
    static_assert(!CORR || DIST, "the correlated flavours: on top of the disturbed ones");
    constexpr bool RESP = std::is_base_of<PolicyEvalStatsRespW, PW>::value || std::is_base_of<PolicyMonteCarloRespW, PW>::value;
    const int64_t ep = ((int64_t)a.n_per_policy + 63) / 64 * 64, total = (int64_t)a.n_policies * ep;
    Launch<T> L{a.group ? w.group_name : w.name, a.cfg, a.st, nullptr, a.seed, a.env_offset, total, a.n_traffic, a.n_steps,
                a.stream};
    L.group_policy = a.group;
    L.correlated = CORR;
    L.delayed = RESP;
    const auto inputs = [&] {
        if (int rc = nulls(L.name)) return rc;
        if (int rc = require_actor(L.name, a.pol)) return rc;
        if (a.n_policies < 1 || a.n_per_policy < 1)
            return fail("%s: n_policies = %d, %s = %d (at least 1 each)", L.name, a.n_policies, w.count, a.n_per_policy);
        if (int rc = own(L.name)) return rc;
        if constexpr (DIST) return check_disturbance(L.name, a.cfg, dist);
        return ACAS2D_OK;
    };
    const auto shape = [&](Shape* sh) {
        if (int rc = a.group ? group_shape<T>(L.name, w.sibling, a.n_traffic, sh) : thread_per_env(L.name, a.n_traffic, sh)) return rc;
        if (a.n_envs >= total) return ACAS2D_OK;
        return fail("%s: the state holds n_envs = %lld envs, %d policies x %lld (%s = %d rounded up to 64) need %lld",
                    w.holds ? w.holds : L.name, (long long)a.n_envs, a.n_policies, (long long)ep, w.count, a.n_per_policy,
                    (long long)total);
    };
    const auto go = [&] {
        if (a.group)
            if (int rc = require_aligned(L.name, {a.pol->w1t, a.pol->b1, a.pol->w2t, a.pol->b2})) return rc;
        if constexpr (CORR)
            if (int rc = check_correlation(L.name, corr)) return rc;
        if constexpr (RESP)
            if (int rc = check_response(L.name, resp, total)) return rc;
        PW pw = actor<PW>(a.pol, a.obs_in);
        if constexpr (DIST) pw.dist = disturbance_words(*dist);
        if constexpr (CORR) pw.corr = correlation_words(*corr);
        if constexpr (RESP) pw.resp = response_words(*resp);
        pw.n_episodes = a.n_per_policy; pw.ep_stride = (int32_t)ep;
        fill(pw);
        return launch_mode<Mode::Eval>(L, pw);
    };
    return prepare(L, Words{"cfg / policies", kSizes, "%s: negative env_offset"}, a.pol != nullptr, inputs, shape, go);
}

// acas2d_evaluate_policies_*: each lane's first episode, scored.  Scoring::Stats adds the per-episode safety statistics
// (eval_stats_kernel instead of step_kernel<..., Mode::Eval>), Scoring::Disturbed sensor noise and actuator disturbance on
// top (eval_stats_disturbed_kernel; float32), Scoring::Correlated a Gauss-Markov error in the white noise's place
// (eval_stats_correlated_kernel; float32, instantiated by acas2d_scoring_correlated.hip), Scoring::Delayed a dead time and a lag
// between the actor and the actuator on top of that (eval_stats_delayed_kernel; float32, acas2d_scoring_delayed.hip).
// (The units instantiate Stats and Disturbed LAST -- ACAS2D_INSTANTIATE_SCORING at their ends -- so that their kernels follow
//  every other kernel of the unit, and those keep the local labels of their assembly too.)
template <typename T, Scoring V>
int launch_evaluate_policies(const ScoringArgs& a, uint8_t* outcome, int32_t* steps, void* total_reward,
                             const Acas2dEvalStats* stats, const Acas2dDisturbance* dist, const Acas2dCorrelation* corr,
                             const Acas2dResponse* resp) {
    constexpr bool STATS = V != Scoring::Plain, RESP = V == Scoring::Delayed, CORR = V == Scoring::Correlated || RESP;
    constexpr bool DIST = V == Scoring::Disturbed || CORR;
    using PW = typename std::conditional<RESP, PolicyEvalStatsRespW, typename std::conditional<CORR, PolicyEvalStatsCorrW, typename std::conditional<DIST, PolicyEvalStatsDistW,
                                         typename std::conditional<STATS, PolicyEvalStatsW, PolicyEvalW>::type>::type>::type>::type;
    const auto nulls = [&](const char* name) {
        if (!a.obs_in || !outcome || !steps || !total_reward)
            return fail("%s: obs_in and the outcome, steps and total_reward outputs are required", name);
        if (STATS && !stats) return fail("%s: NULL stats", name);
        if (STATS && (!stats->min_sep || !stats->min_sep_step || !stats->los_steps || !stats->max_a_lat || !stats->max_dev ||
                      !stats->sum_dev))
            return fail("%s: the min_sep, min_sep_step, los_steps, max_a_lat, max_dev and sum_dev outputs of stats are required",
                        name);
        return ACAS2D_OK;
    };
    const auto fill = [&](PW& pw) {
        pw.res_outcome = outcome; pw.res_steps = steps; pw.res_return = total_reward;
        if constexpr (STATS) {
            pw.st_min_sep = stats->min_sep; pw.st_min_sep_step = stats->min_sep_step; pw.st_los_steps = stats->los_steps;
            pw.st_max_a_lat = stats->max_a_lat; pw.st_max_dev = stats->max_dev; pw.st_sum_dev = stats->sum_dev;
        }
    };
    return score<T, PW, DIST>(a, kEvaluateWords[(int)V], dist, corr, resp, nulls, [](const char*) { return ACAS2D_OK; }, fill);
}

// acas2d_monte_carlo_*: the same blocks of lanes, each lane playing mc->episodes_per_lane drawn episodes and folding them
// into mc's accumulators (monte_carlo_kernel; V = 1: monte_carlo_disturbed_kernel, V = 2: monte_carlo_correlated_kernel, V = 3:
// monte_carlo_delayed_kernel, all three float32).  Instantiated after the stats evaluator, for the same reason.
template <typename T, int V>
int launch_monte_carlo(const ScoringArgs& a, const Acas2dMonteCarlo* mc, const Acas2dDisturbance* dist, const Acas2dCorrelation* corr,
                       const Acas2dResponse* resp) {
    constexpr bool DIST = V >= 1, CORR = V >= 2, RESP = V == 3;
    using PW = typename std::conditional<RESP, PolicyMonteCarloRespW, typename std::conditional<CORR, PolicyMonteCarloCorrW,
                                         typename std::conditional<DIST, PolicyMonteCarloDistW, PolicyMonteCarloW>::type>::type>::type;
    const auto nulls = [&](const char* name) {
        if (!a.obs_in) return fail("%s: obs_in is required", name);
        if (!mc) return fail("%s: NULL mc", name);
        if (!mc->outcome_count || !mc->sum_steps || !mc->los_episodes || !mc->sum_los_steps || !mc->sep_hist ||
            !mc->lane_return_sum || !mc->lane_return_sq || !mc->lane_worst_sep || !mc->lane_worst_episode)
            return fail("%s: the nine accumulators of mc are required", name);
        return ACAS2D_OK;
    };
    const auto own = [&](const char* name) {
        if (mc->episodes_per_lane < 1) return fail("%s: episodes_per_lane = %d (at least 1)", name, mc->episodes_per_lane);
        if (mc->n_bins < 1) return fail("%s: n_bins = %d (at least 1)", name, mc->n_bins);
        if ((uint64_t)mc->first_episode + (uint64_t)mc->episodes_per_lane > (1ull << 32))
            return fail("%s: first_episode = %u + episodes_per_lane = %d exceeds the 32-bit episode counter", name,
                        mc->first_episode, mc->episodes_per_lane);
        const int64_t need = (int64_t)mc->episodes_per_lane * a.cfg->max_steps;
        if (a.cfg->max_steps < 1 || need + mc->episodes_per_lane > 0x7fffffffLL || mc->episodes_per_lane > (1 << 24) ||
            a.n_steps < need)
            return fail("%s: n_steps = %d does not cover episodes_per_lane = %d episodes of max_steps = %d steps (%lld needed; "
                        "episodes_per_lane x (max_steps + 1) must fit an int32, episodes_per_lane <= 2^24)", name, a.n_steps,
                        mc->episodes_per_lane, a.cfg->max_steps, (long long)need);
        return ACAS2D_OK;
    };
    const auto fill = [&](PW& pw) {
        const auto u64 = [](int64_t* q) { return reinterpret_cast<unsigned long long*>(q); };
        pw.mc_outcome_count = u64(mc->outcome_count); pw.mc_sum_steps = u64(mc->sum_steps);
        pw.mc_los_episodes = u64(mc->los_episodes); pw.mc_sum_los_steps = u64(mc->sum_los_steps); pw.mc_sep_hist = u64(mc->sep_hist);
        pw.mc_return_sum = mc->lane_return_sum; pw.mc_return_sq = mc->lane_return_sq;
        pw.mc_worst_sep = mc->lane_worst_sep; pw.mc_worst_episode = mc->lane_worst_episode;
        pw.mc_n_bins = mc->n_bins; pw.mc_episodes = mc->episodes_per_lane; pw.mc_first = mc->first_episode;
        pw.mc_inv_bin_f = (float)mc->inv_bin_width; pw.mc_inv_bin_d = mc->inv_bin_width;
    };
    return score<T, PW, DIST>(a, kMonteCarloWords[V], dist, corr, resp, nulls, own, fill);
}

// acas2d_disturbance_draw_f32: the normals the disturbed kernels draw (float32; instantiated with them)
template <typename T>
int launch_disturbance_draw(uint64_t seed, int64_t first_lane, int32_t n_lanes, uint32_t episode, int32_t first_step,
                            int32_t n_steps, int32_t n_slots, T* out, hipStream_t stream) {
    const char* name = "acas2d_disturbance_draw";
    if (!out) return fail("%s: NULL out", name);
    if (n_lanes < 1 || n_steps < 1 || n_slots < 1)
        return fail("%s: n_lanes = %d, n_steps = %d, n_slots = %d (at least 1 each)", name, n_lanes, n_steps, n_slots);
    if (first_lane < 0 || first_step < 0) return fail("%s: negative first_lane / first_step", name);
    if ((int64_t)first_step + n_steps > (1ll << kDisturbanceSlotShift))
        return fail("%s: first_step = %d + n_steps = %d exceeds the step field of the noise counter (2^%d)", name, first_step,
                    n_steps, kDisturbanceSlotShift);
    if (n_slots > 65) return fail("%s: n_slots = %d (at most 65: the actuator and 64 traffic aircraft)", name, n_slots);
    const uint64_t total = (uint64_t)n_steps * (uint64_t)n_lanes * (uint64_t)n_slots;
    if (total > (1ull << 38)) return fail("%s: %llu blocks (at most 2^38 per call)", name, (unsigned long long)total);
    hipLaunchKernelGGL((disturbance_draw_kernel<T>), dim3((unsigned)((total + 255u) / 256u)), dim3(256), 0, stream, (uint32_t)seed,
                       (uint32_t)(seed >> 32), (uint64_t)first_lane, (uint32_t)n_lanes, episode, (uint32_t)first_step,
                       (uint32_t)n_slots, total, out);
    return check_launch(name);
}
// The family's instantiations behind everything else of a unit, in the order their kernels have always been emitted: the
// stats evaluator, the campaign, and -- the float32 unit's tail -- the disturbed evaluator, the disturbed campaign, the draw.
// (The plain evaluator's kernels are step_kernel's: it is instantiated with the other launchers, below.)
#define ACAS2D_INSTANTIATE_SCORING \
    namespace acas2d { \
    template decltype(launch_evaluate_policies<Elem, Scoring::Stats>) launch_evaluate_policies<Elem, Scoring::Stats>; \
    template decltype(launch_monte_carlo<Elem, 0>) launch_monte_carlo<Elem, 0>; }
#define ACAS2D_INSTANTIATE_SCORING_DISTURBED \
    namespace acas2d { \
    template decltype(launch_evaluate_policies<Elem, Scoring::Disturbed>) launch_evaluate_policies<Elem, Scoring::Disturbed>; \
    template decltype(launch_monte_carlo<Elem, 1>) launch_monte_carlo<Elem, 1>; \
    template decltype(launch_disturbance_draw<Elem>) launch_disturbance_draw<Elem>; }
// the correlated evaluator and campaign: the instantiations of acas2d_scoring_correlated.hip, a unit of its own for the reason
// the disturbed set collector's is one
#define ACAS2D_INSTANTIATE_SCORING_CORRELATED \
    namespace acas2d { \
    template decltype(launch_evaluate_policies<Elem, Scoring::Correlated>) launch_evaluate_policies<Elem, Scoring::Correlated>; \
    template decltype(launch_monte_carlo<Elem, 2>) launch_monte_carlo<Elem, 2>; }
// the delayed evaluator and campaign: the instantiations of acas2d_scoring_delayed.hip, a unit of its own likewise
#define ACAS2D_INSTANTIATE_SCORING_DELAYED \
    namespace acas2d { \
    template decltype(launch_evaluate_policies<Elem, Scoring::Delayed>) launch_evaluate_policies<Elem, Scoring::Delayed>; \
    template decltype(launch_monte_carlo<Elem, 3>) launch_monte_carlo<Elem, 3>; }
// the disturbed set collector: the ONE instantiation of acas2d_collect_disturbed.hip, a unit of its own -- the float32 unit
// ends with the kernels above, and every kernel of it keeps its place, its name and the local labels of its assembly
#define ACAS2D_INSTANTIATE_COLLECT_DISTURBED \
    namespace acas2d { template decltype(launch_collect_set_disturbed<Elem>) launch_collect_set_disturbed<Elem>; }
// ... and the correlated one: the ONE instantiation of acas2d_collect_correlated.hip, a unit of its own likewise
#define ACAS2D_INSTANTIATE_COLLECT_CORRELATED \
    namespace acas2d { template decltype(launch_collect_set_correlated<Elem>) launch_collect_set_correlated<Elem>; }

template <typename T>
int launch_reset(const Acas2dConfig* cfg, const Acas2dState* st, const uint8_t* mask, void* obs,
                 int32_t do_init, uint64_t seed, int64_t env_offset, int64_t n_envs, int32_t n_traffic,
                 hipStream_t stream) {
    Launch<T> L{"acas2d_reset", cfg, st, nullptr, seed, env_offset, n_envs, n_traffic, 1, stream};
    const auto go = [&] {
        if (do_init < 0) return fail("%s: do_init = %d", L.name, do_init);
        const StepResetParams<T, true> rp = make_reset_params<T, true>(*cfg);
        dispatch(*cfg, L.sh, [&](auto fast, auto C, auto G, auto packed) {
            hipLaunchKernelGGL((reset_kernel<T, C, G, packed, fast>), dim3(L.g.grid), dim3(kBlock), L.g.lds_bytes, stream,
                               L.p, rp, L.s, mask, (T*)obs, do_init, L.k0, L.k1, env_offset, n_envs, n_traffic, L.g.tile_elems);
        });
        return ACAS2D_OK;
    };
    return prepare(L, Words{"cfg", "%s: n_traffic = %d", kNegative}, true, [] { return ACAS2D_OK; },
                   [&](Shape* sh) { return resolve_shape<T>(n_traffic, sh); }, go);
}

// 1 when acas2d_step_* (auto-reset) would take the kernel whose loads all go through preloaded base pointers for this
// state: float32, a packed work shape, the consecutive layout of arena_layout()
template <typename T>
int state_consecutive(const Acas2dState* st, int64_t n_envs, int32_t n_traffic) {
    if (!state_complete(st) || n_envs <= 0 || n_traffic < 1) return 0;
    Shape sh;
    if (resolve_shape<T>(n_traffic, &sh) != ACAS2D_OK || !sh.packed) return 0;
    return arena_layout<T>(make_state<T>(*st), n_envs, n_traffic, sh.G) ? 1 : 0;
}

template <typename T>
int shape_geometry(int64_t n_envs, int32_t n_traffic, int32_t* lanes, int32_t* per_lane, int64_t* grid) {
    Shape sh;
    if (int rc = resolve_shape<T>(n_traffic, &sh)) return rc;
    Geometry g;
    if (int rc = geometry_for<T>(sh, n_envs, n_traffic, &g)) return rc;
    *lanes = sh.G; *per_lane = sh.packed ? sh.C : -1; *grid = g.grid;
    return ACAS2D_OK;
}

// the launchers of this unit's element type (acas2d_kernels.hpp declares them, acas2d_api.hip calls them); a unit that
// defines ACAS2D_LAUNCHERS_BY_NAME instantiates the ones it names itself (acas2d_collect_disturbed.hip and its kin)
#ifndef ACAS2D_LAUNCHERS_BY_NAME
template decltype(launch_step<Elem>) launch_step<Elem>;
template decltype(launch_rollout<Elem>) launch_rollout<Elem>;
template decltype(launch_rollout_policy<Elem>) launch_rollout_policy<Elem>;
template decltype(launch_collect<Elem>) launch_collect<Elem>;
template decltype(launch_rollout_policy_group<Elem>) launch_rollout_policy_group<Elem>;
template decltype(launch_collect_group<Elem>) launch_collect_group<Elem>;
template decltype(launch_evaluate_policies<Elem, Scoring::Plain>) launch_evaluate_policies<Elem, Scoring::Plain>;
template decltype(launch_reset<Elem>) launch_reset<Elem>;
template decltype(shape_geometry<Elem>) shape_geometry<Elem>;
template decltype(state_consecutive<Elem>) state_consecutive<Elem>;
#endif

}  // namespace acas2d
