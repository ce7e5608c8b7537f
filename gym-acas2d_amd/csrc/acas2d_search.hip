// acas2d_search.hip -- what a cross-entropy search over encounters (Rubinstein's cross-entropy method with importance
// sampling) needs around the unchanged stats evaluator, in THREE small launches per generation with no host decision in
// between (include/acas2d.h, Acas2dEncounterSearch):
//
//   encounter_sample_kernel  acas2d_encounter_sample_f32 / _f64: candidate i of policy block k draws the N + 1 Philox blocks
//                            of reset_entity() -- counter (lane lo, lane hi, generation, entity), lane = env_offset + i -- and
//                            sends each of the 4 (N + 1) uniforms through its coordinate's piecewise-constant proposal; the
//                            state follows by reset_entity()'s float64 formulas and is stored into the evaluation engine's
//                            arrays, with the bins and the log likelihood ratio of the candidate.
//   encounter_select_kernel  acas2d_encounter_select_f32 / _f64: per policy, the n_quantile-th smallest minimum separation by
//                            a radix select, the elite set and its weights, one row of the device log, and the archive of
//                            the closest encounter ever found (its state is drawn AGAIN from the tables of its generation:
//                            the evaluator has stepped the arrays the sampler wrote).
//   encounter_refit_kernel   acas2d_encounter_refit: per (coordinate, policy) the weighted bin masses of the elite, the
//                            smoothed, floored and renormalised proposal, and its cdf and log-ratio rows.
//
// Sums.  Every floating sum over candidates is taken in one fixed order, as member_episodes_kernel (acas2d_pbt.hip) does
// it: in the thread its candidates tid, tid + T, ... ascending; in the wave the xor tree 32, 16, 8, 4, 2, 1; across the
// waves 0, 1, ... in thread 0.  The only atomics are integer adds into the digit histograms of the radix select, so the
// same inputs give the same bits.  Everything is float64 with every operation rounded on its own (the unit is built with
// -ffp-contract=off; the pragmas below say so again where the rounding is part of the definition).
#include <float.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>

#include <type_traits>

#include "acas2d_kernels.hpp"

namespace acas2d {
namespace {

constexpr int kSampleThreads = 256, kSelectThreads = 256, kSelectWaves = kSelectThreads / 64, kRefitThreads = 128;
constexpr int kHistoryWidth = ACAS2D_SEARCH_HISTORY_WIDTH;

// the reset distribution's constants in float64 (reset_entity()'s float64 branch reads the same eighteen)
struct DrawParams {
    double own_x0, own_y0, own_v, own_heading0, own_heading_jitter, goal_x, goal_y;
    double t0_x, t0_y_base, t0_y_span, t0_heading_base, t0_heading_step, t0_heading_jitter;
    double tn_x_max, tn_y_max, speed_factor_min, speed_factor_max, airspeed;
};

// what names a candidate's draw: the proposal's tables, the Philox key and counter words, the layout
struct DrawArgs {
    const double *p, *cdf, *log_ratio;   // [K][n_coord][B], [K][n_coord][B + 1], [K][n_coord][B]
    const uint8_t* active;               // [n_coord]
    DrawParams rp;
    int64_t env_offset;
    uint32_t k0, k1, generation;
    int32_t n_bins, n_coord, n_traffic, n_cand, ep;      // ep = n_cand rounded up to 64
};

// The eighteen constants into VGPRs once (there are registers to spare; as scalars they and the kernel's pointers do not fit
// the SGPR file together and the allocator spills)
__device__ __forceinline__ void pin(DrawParams& rp) {
    pin_vgpr(rp.own_x0); pin_vgpr(rp.own_y0); pin_vgpr(rp.own_v); pin_vgpr(rp.own_heading0); pin_vgpr(rp.own_heading_jitter);
    pin_vgpr(rp.goal_x); pin_vgpr(rp.goal_y); pin_vgpr(rp.t0_x); pin_vgpr(rp.t0_y_base); pin_vgpr(rp.t0_y_span);
    pin_vgpr(rp.t0_heading_base); pin_vgpr(rp.t0_heading_step); pin_vgpr(rp.t0_heading_jitter); pin_vgpr(rp.tn_x_max);
    pin_vgpr(rp.tn_y_max); pin_vgpr(rp.speed_factor_min); pin_vgpr(rp.speed_factor_max); pin_vgpr(rp.airspeed);
}

// One coordinate through the inverse CDF of its row (wave-uniform rows: scalar loads).  An inactive coordinate keeps its
// uniform and adds nothing to the log ratio.
__device__ __forceinline__ double draw_coordinate(const DrawArgs& a, size_t row, bool active, double u, uint32_t& bin,
                                                   double& log_w) {
#pragma clang fp contract(off)
    const int B = a.n_bins;
    if (!active) {
        const int b = (int)(u * (double)B);
        bin = (uint32_t)(b < B - 1 ? b : B - 1);
        return u;
    }
    const double* __restrict__ p = a.p + row * (size_t)B;
    const double* __restrict__ cdf = a.cdf + row * (size_t)(B + 1);
    const double* __restrict__ lr = a.log_ratio + row * (size_t)B;
    int b = 0;
    double lo = cdf[0], pb = p[0], l = lr[0];
    for (int j = 1; j < B; ++j) {                        // the largest j with cdf[j] <= u
        const double cj = cdf[j], pj = p[j], lj = lr[j];
        const bool ge = cj <= u;
        b = ge ? j : b; lo = ge ? cj : lo; pb = ge ? pj : pb; l = ge ? lj : l;
    }
    double t = (u - lo) / pb;
    t = t > 0.0 ? t : 0.0;                               // (also a NaN: 0 / 0 of an empty bin)
    t = t < 0x1.fffffffffffffp-1 ? t : 0x1.fffffffffffffp-1;
    bin = (uint32_t)b;
    log_w += l;
    return ((double)b + t) / (double)B;
}

// Entity `ent` (0 = the player, n + 1 = traffic n) of candidate `cand` in policy block k: its four coordinates, and the
// state by reset_entity()'s float64 formulas with the coordinates in place of u01(w).
__device__ __forceinline__ void draw_entity(const DrawArgs& a, uint32_t k, uint32_t cand, int ent, double& x, double& y,
                                            double& psi, double& v, uint32_t bin[4], double& log_w) {
#pragma clang fp contract(off)
    const uint64_t gid = (uint64_t)a.env_offset + cand;
    const U4 w = philox4x32(U4{(uint32_t)gid, (uint32_t)(gid >> 32), a.generation, (uint32_t)ent}, a.k0, a.k1);
    const size_t row = (size_t)k * (size_t)a.n_coord + 4u * (size_t)ent;
    const uint8_t* __restrict__ act = a.active + 4 * ent;
    const double cx = draw_coordinate(a, row + 0, act[0] != 0, u01(w.x), bin[0], log_w);
    const double cy = draw_coordinate(a, row + 1, act[1] != 0, u01(w.y), bin[1], log_w);
    const double cz = draw_coordinate(a, row + 2, act[2] != 0, u01(w.z), bin[2], log_w);
    const double cw = draw_coordinate(a, row + 3, act[3] != 0, u01(w.w), bin[3], log_w);
    const DrawParams& rp = a.rp;
    const bool own = ent == 0, first = ent == 1;
    const double down = cx >= 0.5 ? 1.0 : 0.0;
    const double jitter = own ? rp.own_heading_jitter : rp.t0_heading_jitter;
    const double base = own ? rp.own_heading0 : (rp.t0_heading_base + (down * rp.t0_heading_step));
    const double psi_special = py_mod360(base + uniform(-jitter, jitter, cz));
    psi = (own || first) ? psi_special : uniform(0.0, 360.0, cz);
    x = own ? rp.own_x0 : (first ? rp.t0_x : uniform(0.0, rp.tn_x_max, cx));
    y = own ? rp.own_y0 : (first ? (rp.t0_y_base + (down * rp.t0_y_span)) : uniform(0.0, rp.tn_y_max, cy));
    v = own ? rp.own_v : uniform(rp.speed_factor_min, rp.speed_factor_max, cw) * rp.airspeed;
}

// ---- sample --------------------------------------------------------------------------------------------------------------
template <typename T>
struct SampleArgs {
    DrawArgs d;
    T *own_x, *own_y, *own_psi, *own_v, *goal_x, *goal_y, *trf_x, *trf_y, *trf_psi, *trf_v;
    int32_t* steps;
    T* total_reward;
    uint8_t* bins;                       // [K][n_coord][n_cand]
    double* log_w;                       // [K][n_cand]
};

// grid (ep / 256 rounded up, K): one lane per env of the block's policy; the padding lanes (n_cand <= i < ep) repeat
// candidate 0 and store the state only
template <typename T>
__global__ __launch_bounds__(kSampleThreads) void encounter_sample_kernel(SampleArgs<T> a) {
    DrawArgs d = a.d;
    pin(d.rp);
    const uint32_t i = blockIdx.x * kSampleThreads + threadIdx.x, k = blockIdx.y;
    if (i >= (uint32_t)d.ep) return;
    const bool real = i < (uint32_t)d.n_cand;
    const uint32_t cand = real ? i : 0u;
    const size_t env = (size_t)k * (size_t)d.ep + i, L = (size_t)d.n_cand;
    const int N = d.n_traffic;
    uint8_t* __restrict__ bins = a.bins + (size_t)k * (size_t)d.n_coord * L + cand;
    double log_w = 0.0;
    {                                                    // the player
        double x, y, psi, v;
        uint32_t bin[4];
        draw_entity(d, k, cand, 0, x, y, psi, v, bin, log_w);
        a.own_x[env] = (T)x; a.own_y[env] = (T)y; a.own_psi[env] = (T)psi; a.own_v[env] = (T)v;
        a.goal_x[env] = (T)d.rp.goal_x; a.goal_y[env] = (T)d.rp.goal_y;
        a.steps[env] = 0; a.total_reward[env] = T(0);
        if (real) {
#pragma unroll
            for (int j = 0; j < 4; ++j) bins[(size_t)j * L] = (uint8_t)bin[j];
        }
    }
    for (int ent = 1; ent <= N; ++ent) {                 // traffic ent - 1
        double x, y, psi, v;
        uint32_t bin[4];
        draw_entity(d, k, cand, ent, x, y, psi, v, bin, log_w);
        const size_t at = env * (size_t)N + (size_t)(ent - 1);
        a.trf_x[at] = (T)x; a.trf_y[at] = (T)y; a.trf_psi[at] = (T)psi; a.trf_v[at] = (T)v;
        if (real) {
#pragma unroll
            for (int j = 0; j < 4; ++j) bins[(size_t)(4 * ent + j) * L] = (uint8_t)bin[j];
        }
    }
    if (real) a.log_w[(size_t)k * L + cand] = log_w;
}

// ---- select --------------------------------------------------------------------------------------------------------------
template <typename T>
struct SelectArgs {
    DrawArgs d;
    const uint8_t* outcome;              // [K][n_cand]
    const T* min_sep;                    // [K][n_cand]
    const double* log_w;                 // [K][n_cand]
    double* elite_w;                     // [K][n_cand]
    double* history;                     // [K][kHistoryWidth]: this generation's row
    T* best_score;                       // [K]
    uint32_t* best_generation;           // [K]
    int32_t* best_candidate;             // [K]
    T *best_own_psi, *best_traffic;      // [K], [K][N][4]
    T level;
    int32_t n_quantile, weighted;
};

template <typename T> struct KeyOf;
template <> struct KeyOf<float> { using type = uint32_t; };
template <> struct KeyOf<double> { using type = uint64_t; };

// the integer whose unsigned order is the order of the floats (-inf < ... < -0 < +0 < ... < +inf)
template <typename T>
__device__ __forceinline__ typename KeyOf<T>::type ordered_key(T v) {
    using K = typename KeyOf<T>::type;
    K u;
    __builtin_memcpy(&u, &v, sizeof(T));
    const K top = (K)1 << (8 * sizeof(T) - 1);
    return (u & top) ? ~u : (u | top);
}
template <typename T>
__device__ __forceinline__ T from_key(typename KeyOf<T>::type key) {
    using K = typename KeyOf<T>::type;
    const K top = (K)1 << (8 * sizeof(T) - 1);
    const K u = (key & top) ? (key & ~top) : ~key;
    T v;
    __builtin_memcpy(&v, &u, sizeof(T));
    return v;
}
// a candidate's score: its minimum separation where the episode finished and the value is a number, else +inf
template <typename T>
__device__ __forceinline__ T score_of(uint8_t outcome, T sep) {
    return (outcome != 0 && sep == sep) ? sep : (T)__builtin_inff();
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// one workgroup per policy
template <typename T>
__global__ __launch_bounds__(kSelectThreads) void encounter_select_kernel(SelectArgs<T> a) {
    using Key = typename KeyOf<T>::type;
    __shared__ uint32_t s_hist[256];
    __shared__ Key s_prefix;
    __shared__ uint32_t s_rank;
    __shared__ double s_sum[kSelectWaves][4];
    __shared__ uint32_t s_cnt[kSelectWaves][4];
    __shared__ T s_min[kSelectWaves];
    __shared__ uint32_t s_arg[kSelectWaves];
    __shared__ uint32_t s_best;          // the candidate that enters the archive, or 0xffffffff
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, k = blockIdx.x;
    const uint32_t L = (uint32_t)a.d.n_cand;
    const uint8_t* __restrict__ outcome = a.outcome + (size_t)k * L;
    const T* __restrict__ sep = a.min_sep + (size_t)k * L;

    // gamma_q: the n_quantile-th smallest score, one 8-bit digit of its key per pass from the top
    Key prefix = 0;
    uint32_t rank = (uint32_t)a.n_quantile;
    for (int pass = 0; pass < (int)sizeof(T); ++pass) {
        const int shift = 8 * ((int)sizeof(T) - 1 - pass);
        const Key above = pass == 0 ? (Key)0 : (Key)(~(Key)0 << (shift + 8));
        if (tid < 256u) s_hist[tid] = 0u;
        __syncthreads();
        for (uint32_t i = tid; i < L; i += kSelectThreads) {
            const Key key = ordered_key<T>(score_of<T>(outcome[i], sep[i]));
            if ((key & above) == prefix) atomicAdd(&s_hist[(uint32_t)(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (wave == 0) {                                 // lane l: digits 4 l .. 4 l + 3; the first digit whose running count reaches rank
            const uint32_t h0 = s_hist[4 * lane], h1 = s_hist[4 * lane + 1], h2 = s_hist[4 * lane + 2], h3 = s_hist[4 * lane + 3];
            const uint32_t mine = h0 + h1 + h2 + h3;
            uint32_t incl = mine;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t t = __shfl_up(incl, o, 64);
                incl += lane >= (uint32_t)o ? t : 0u;
            }
            const uint64_t reached = __ballot(incl >= rank);         // never empty: the prefix holds at least `rank` keys
            if (lane == (uint32_t)(__ffsll((unsigned long long)reached) - 1)) {
                const uint32_t e0 = incl - mine, e1 = e0 + h0, e2 = e1 + h1, e3 = e2 + h2;
                const uint32_t j = e1 >= rank ? 0u : (e2 >= rank ? 1u : (e3 >= rank ? 2u : 3u));
                const uint32_t below = j == 0u ? e0 : (j == 1u ? e1 : (j == 2u ? e2 : e3));
                s_prefix = prefix | ((Key)(4u * lane + j) << shift);
                s_rank = rank - below;
            }
        }
        __syncthreads();
        prefix = s_prefix;
        rank = s_rank;
    }
    const T gamma_q = from_key<T>(prefix);
    const T level = a.level;
    const T gamma = gamma_q > level ? gamma_q : level;
    const T inf = (T)__builtin_inff();

    // weights, counts, sums and the minimum: each thread its candidates ascending
    const double* __restrict__ log_w = a.log_w + (size_t)k * L;
    double* __restrict__ elite_w = a.elite_w + (size_t)k * L;
    double sw_ev = 0.0, sw2_ev = 0.0, sw = 0.0, sw2 = 0.0;
    uint32_t n_fin = 0, n_elite = 0, n_event = 0;
    T best = inf;
    uint32_t arg = 0xffffffffu;
    {
#pragma clang fp contract(off)
        for (uint32_t i = tid; i < L; i += kSelectThreads) {
            const uint8_t oc = outcome[i];
            const T s = score_of<T>(oc, sep[i]);
            const double w = a.weighted ? exp(log_w[i]) : 1.0;
            const bool elite = s <= gamma && s < inf, event = s <= level;
            elite_w[i] = elite ? w : 0.0;
            n_fin += oc != 0 ? 1u : 0u; n_elite += elite ? 1u : 0u; n_event += event ? 1u : 0u;
            const double w2 = w * w;
            sw += w; sw2 += w2;
            if (event) { sw_ev += w; sw2_ev += w2; }
            if (s < best || arg == 0xffffffffu) { best = s; arg = i; }
        }
    }
    double r[4] = {wave_sum(sw_ev), wave_sum(sw2_ev), wave_sum(sw), wave_sum(sw2)};
    uint32_t c[3] = {wave_sum(n_fin), wave_sum(n_elite), wave_sum(n_event)};
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {                   // (score, candidate) lexicographically: exact in any order
        const T ob = __shfl_xor(best, o, 64);
        const uint32_t oa = __shfl_xor(arg, o, 64);
        if (ob < best || (ob == best && oa < arg)) { best = ob; arg = oa; }
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) s_sum[wave][j] = r[j];
#pragma unroll
        for (int j = 0; j < 3; ++j) s_cnt[wave][j] = c[j];
        s_min[wave] = best; s_arg[wave] = arg;
    }
    __syncthreads();
    if (tid == 0) {
#pragma clang fp contract(off)
        for (int w = 1; w < kSelectWaves; ++w) {
#pragma unroll
            for (int j = 0; j < 4; ++j) r[j] += s_sum[w][j];
#pragma unroll
            for (int j = 0; j < 3; ++j) c[j] += s_cnt[w][j];
            if (s_min[w] < best || (s_min[w] == best && s_arg[w] < arg)) { best = s_min[w]; arg = s_arg[w]; }
        }
        double* __restrict__ h = a.history + (size_t)k * kHistoryWidth;
        h[0] = (double)c[0]; h[1] = (double)(L - c[0]); h[2] = (double)c[1]; h[3] = (double)gamma_q; h[4] = (double)gamma;
        h[5] = (double)c[2]; h[6] = r[0]; h[7] = r[1]; h[8] = r[2]; h[9] = r[3]; h[10] = (double)best; h[11] = (double)arg;
        h[12] = (double)a.d.generation; h[13] = 0.0; h[14] = 0.0; h[15] = 0.0;
        const bool better = best < a.best_score[k];      // strictly: the first occurrence keeps its place
        s_best = better ? arg : 0xffffffffu;
        if (better) { a.best_score[k] = best; a.best_generation[k] = a.d.generation; a.best_candidate[k] = (int32_t)arg; }
    }
    __syncthreads();
    const uint32_t cand = s_best;
    if (cand != 0xffffffffu && tid <= (uint32_t)a.d.n_traffic) {     // thread e: entity e of the archived encounter, drawn again
        double x, y, psi, v, lw = 0.0;
        uint32_t bin[4];
        DrawArgs d = a.d;
        pin(d.rp);
        draw_entity(d, k, cand, (int)tid, x, y, psi, v, bin, lw);
        if (tid == 0) {
            a.best_own_psi[k] = (T)psi;
        } else {
            T* __restrict__ t = a.best_traffic + ((size_t)k * (size_t)a.d.n_traffic + (tid - 1u)) * 4u;
            t[0] = (T)x; t[1] = (T)y; t[2] = (T)psi; t[3] = (T)v;
        }
    }
}

// ---- refit ---------------------------------------------------------------------------------------------------------------
struct RefitArgs {
    double *p, *cdf, *log_ratio;
    const uint8_t* active;
    const uint8_t* bins;                 // [K][n_coord][n_cand]
    const double* elite_w;               // [K][n_cand]
    double alpha, p_floor;
    int32_t n_bins, n_coord, n_cand;
};

// grid (n_coord, K), dynamic LDS double[B][kRefitThreads]: thread t's private column of bin masses (no register array is
// indexed by a bin), then per bin the wave tree and the waves in order; thread 0 refits the row
__global__ __launch_bounds__(kRefitThreads) void encounter_refit_kernel(RefitArgs a) {
#pragma clang fp contract(off)
    extern __shared__ double tile[];     // [B][kRefitThreads]
    const uint32_t c = blockIdx.x, k = blockIdx.y, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (a.active[c] == 0) return;                        // block-uniform: never refit, flat for ever
    const int B = a.n_bins;
    const uint32_t L = (uint32_t)a.n_cand;
    const size_t row = (size_t)k * (size_t)a.n_coord + c;
    const uint8_t* __restrict__ bins = a.bins + row * L;
    const double* __restrict__ w = a.elite_w + (size_t)k * L;
    for (int b = 0; b < B; ++b) tile[b * kRefitThreads + tid] = 0.0;
    for (uint32_t i = tid; i < L; i += kRefitThreads) {
        const double wi = w[i];
        const uint32_t b = bins[i];
        if (wi != 0.0 && b < (uint32_t)B) tile[b * kRefitThreads + tid] += wi;       // (a non-elite adds nothing)
    }
    for (int b = 0; b < B; ++b) {
        double v = tile[b * kRefitThreads + tid];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) tile[b * kRefitThreads + wave * 64] = v;
    }
    __syncthreads();
    if (tid != 0) return;
    constexpr int kWaves = kRefitThreads / 64;
    double s_tot = 0.0;
    for (int b = 0; b < B; ++b) {
        double s = tile[b * kRefitThreads];
        for (int v = 1; v < kWaves; ++v) s += tile[b * kRefitThreads + v * 64];
        tile[b * kRefitThreads] = s;
        s_tot += s;
    }
    if (!(s_tot > 0.0)) return;                          // no elite: the proposal stays as it is
    double* __restrict__ p = a.p + row * (size_t)B;
    double* __restrict__ cdf = a.cdf + row * (size_t)(B + 1);
    double* __restrict__ lr = a.log_ratio + row * (size_t)B;
    const double keep = 1.0 - a.alpha;
    double norm = 0.0;
    for (int b = 0; b < B; ++b) {
        const double q = tile[b * kRefitThreads] / s_tot;
        double pn = (keep * p[b]) + (a.alpha * q);
        pn = pn > a.p_floor ? pn : a.p_floor;
        tile[b * kRefitThreads + 1] = pn;
        norm += pn;
    }
    double run = 0.0;
    cdf[0] = 0.0;
    for (int b = 0; b < B; ++b) {
        const double pb = tile[b * kRefitThreads + 1] / norm;
        p[b] = pb;
        run += pb;
        cdf[b + 1] = run;
        lr[b] = -log((double)B * pb);
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------
int refuse(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
int refuse(const char* fmt, ...) {
    char buf[400];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    set_error("%s", buf);
    return ACAS2D_EINVAL;
}

// the checks the three entries share; n_traffic < 0: the entry does not know it (refit)
int check_search(const char* name, const Acas2dEncounterSearch* s, int32_t K, int32_t L, int32_t N) {
    if (!s) return refuse("%s: NULL search", name);
    if (!s->p || !s->cdf || !s->log_ratio || !s->active || !s->bins || !s->log_w || !s->elite_w || !s->outcome || !s->min_sep ||
        !s->history || !s->best_score || !s->best_generation || !s->best_candidate || !s->best_own_psi || !s->best_traffic)
        return refuse("%s: the fifteen buffers of search are required", name);
    if (K < 1 || K > 65535 || L < 1) return refuse("%s: n_policies = %d (1 .. 65535), n_candidates = %d (at least 1)", name, K, L);
    const int B = s->n_bins;
    if (B < 2 || B > 64 || (B & (B - 1)) != 0) return refuse("%s: n_bins = %d (a power of two, 2 .. 64)", name, B);
    if (N >= 0 ? (N < 1 || s->n_coord != 4 * (N + 1)) : (s->n_coord < 8 || s->n_coord % 4 != 0)) {
        if (N >= 0) return refuse("%s: n_coord = %d, n_traffic = %d (n_coord = 4 x (n_traffic + 1), n_traffic at least 1)", name, s->n_coord, N);
        return refuse("%s: n_coord = %d (4 x (n_traffic + 1), n_traffic at least 1)", name, s->n_coord);
    }
    if (s->n_coord > 4 * 65536) return refuse("%s: n_coord = %d (at most 4 x 65 536)", name, s->n_coord);
    if (s->n_quantile < 1 || s->n_quantile > L) return refuse("%s: n_quantile = %d (1 .. n_candidates = %d)", name, s->n_quantile, L);
    if (!(s->alpha >= 0.0 && s->alpha <= 1.0)) return refuse("%s: alpha = %g (0 .. 1)", name, s->alpha);
    if (!(s->p_floor >= 0.0 && s->p_floor < 1.0 / B)) return refuse("%s: p_floor = %g (0 <= p_floor < 1 / n_bins = %g)", name, s->p_floor, 1.0 / B);
    if (s->generation >= (1ull << 32)) return refuse("%s: generation = %llu exceeds the 32-bit episode counter", name, (unsigned long long)s->generation);
    if (s->level != s->level) return refuse("%s: level is NaN", name);
    return ACAS2D_OK;
}

int launched(const char* name) {
    const hipError_t err = hipGetLastError();
    if (err == hipSuccess) return ACAS2D_OK;
    set_error("%s launch: %s", name, hipGetErrorString(err));
    return ACAS2D_EHIP;
}

DrawArgs draw_args(const Acas2dConfig& c, const Acas2dEncounterSearch& s, uint64_t seed, int64_t env_offset, int32_t L, int32_t N) {
    DrawArgs d;
    d.p = s.p; d.cdf = s.cdf; d.log_ratio = s.log_ratio; d.active = s.active;
    d.rp = DrawParams{c.own_x0, c.own_y0, c.own_v, c.own_heading0, c.own_heading_jitter, c.goal_x, c.goal_y, c.t0_x, c.t0_y_base,
                      c.t0_y_span, c.t0_heading_base, c.t0_heading_step, c.t0_heading_jitter, c.tn_x_max, c.tn_y_max,
                      c.speed_factor_min, c.speed_factor_max, c.airspeed};
    d.env_offset = env_offset;
    d.k0 = (uint32_t)seed; d.k1 = (uint32_t)(seed >> 32); d.generation = (uint32_t)s.generation;
    d.n_bins = s.n_bins; d.n_coord = s.n_coord; d.n_traffic = N; d.n_cand = L; d.ep = (int32_t)(((int64_t)L + 63) / 64 * 64);
    return d;
}

template <typename T>
int search_sample(const Acas2dConfig* cfg, const Acas2dState* st, int64_t n_envs, int32_t K, int32_t L, uint64_t seed, int64_t env_offset,
           int32_t N, const Acas2dEncounterSearch* s, hipStream_t stream) {
    const char* name = "acas2d_encounter_sample";
    if (!cfg) return refuse("%s: NULL cfg", name);
    if (!st || !st->own_x || !st->own_y || !st->own_psi || !st->own_v || !st->goal_x || !st->goal_y || !st->trf_x || !st->trf_y ||
        !st->trf_psi || !st->trf_v || !st->steps || !st->total_reward)
        return refuse("%s: NULL state or a NULL state buffer", name);
    if (int rc = check_search(name, s, K, L, N)) return rc;
    if (env_offset < 0) return refuse("%s: negative env_offset", name);
    const int64_t ep = ((int64_t)L + 63) / 64 * 64, total = (int64_t)K * ep;
    if (ep > 0x7fffffc0LL) return refuse("%s: n_candidates = %d (rounded up to 64 it must fit an int32)", name, L);
    if (n_envs < total)
        return refuse("%s: the state holds n_envs = %lld envs, %d policies x %lld (n_candidates = %d rounded up to 64) need %lld", name,
                      (long long)n_envs, K, (long long)ep, L, (long long)total);
    SampleArgs<T> a;
    a.d = draw_args(*cfg, *s, seed, env_offset, L, N);
    a.own_x = (T*)st->own_x; a.own_y = (T*)st->own_y; a.own_psi = (T*)st->own_psi; a.own_v = (T*)st->own_v;
    a.goal_x = (T*)st->goal_x; a.goal_y = (T*)st->goal_y;
    a.trf_x = (T*)st->trf_x; a.trf_y = (T*)st->trf_y; a.trf_psi = (T*)st->trf_psi; a.trf_v = (T*)st->trf_v;
    a.steps = st->steps; a.total_reward = (T*)st->total_reward;
    a.bins = s->bins; a.log_w = s->log_w;
    hipLaunchKernelGGL(encounter_sample_kernel<T>, dim3((unsigned)((ep + kSampleThreads - 1) / kSampleThreads), (unsigned)K),
                       dim3(kSampleThreads), 0, stream, a);
    return launched(name);
}

template <typename T>
int search_select(const Acas2dConfig* cfg, int32_t K, int32_t L, uint64_t seed, int64_t env_offset, int32_t N,
           const Acas2dEncounterSearch* s, hipStream_t stream) {
    const char* name = "acas2d_encounter_select";
    if (!cfg) return refuse("%s: NULL cfg", name);
    if (int rc = check_search(name, s, K, L, N)) return rc;
    if (env_offset < 0) return refuse("%s: negative env_offset", name);
    if (N + 1 > kSelectThreads) return refuse("%s: n_traffic = %d (at most %d)", name, N, kSelectThreads - 1);
    SelectArgs<T> a;
    a.d = draw_args(*cfg, *s, seed, env_offset, L, N);
    a.outcome = s->outcome; a.min_sep = (const T*)s->min_sep; a.log_w = s->log_w; a.elite_w = s->elite_w; a.history = s->history;
    a.best_score = (T*)s->best_score; a.best_generation = s->best_generation; a.best_candidate = s->best_candidate;
    a.best_own_psi = (T*)s->best_own_psi; a.best_traffic = (T*)s->best_traffic;
    a.level = (T)s->level; a.n_quantile = s->n_quantile; a.weighted = s->weighted;
    hipLaunchKernelGGL(encounter_select_kernel<T>, dim3((unsigned)K), dim3(kSelectThreads), 0, stream, a);
    return launched(name);
}

}  // namespace
}  // namespace acas2d

using namespace acas2d;

extern "C" size_t acas2d_encounter_search_size(void) { return sizeof(Acas2dEncounterSearch); }

extern "C" int acas2d_encounter_sample_f32(const Acas2dConfig* cfg, const Acas2dState* state, int64_t n_envs, int32_t n_policies,
                                           int32_t n_candidates, uint64_t seed, int64_t env_offset, int32_t n_traffic,
                                           const Acas2dEncounterSearch* search, void* stream) {
    return search_sample<float>(cfg, state, n_envs, n_policies, n_candidates, seed, env_offset, n_traffic, search, (hipStream_t)stream);
}
extern "C" int acas2d_encounter_sample_f64(const Acas2dConfig* cfg, const Acas2dState* state, int64_t n_envs, int32_t n_policies,
                                           int32_t n_candidates, uint64_t seed, int64_t env_offset, int32_t n_traffic,
                                           const Acas2dEncounterSearch* search, void* stream) {
    return search_sample<double>(cfg, state, n_envs, n_policies, n_candidates, seed, env_offset, n_traffic, search, (hipStream_t)stream);
}
extern "C" int acas2d_encounter_select_f32(const Acas2dConfig* cfg, int32_t n_policies, int32_t n_candidates, uint64_t seed,
                                           int64_t env_offset, int32_t n_traffic, const Acas2dEncounterSearch* search, void* stream) {
    return search_select<float>(cfg, n_policies, n_candidates, seed, env_offset, n_traffic, search, (hipStream_t)stream);
}
extern "C" int acas2d_encounter_select_f64(const Acas2dConfig* cfg, int32_t n_policies, int32_t n_candidates, uint64_t seed,
                                           int64_t env_offset, int32_t n_traffic, const Acas2dEncounterSearch* search, void* stream) {
    return search_select<double>(cfg, n_policies, n_candidates, seed, env_offset, n_traffic, search, (hipStream_t)stream);
}

extern "C" int acas2d_encounter_refit(const Acas2dEncounterSearch* s, int32_t n_policies, int32_t n_candidates, void* stream) {
    const char* name = "acas2d_encounter_refit";
    if (int rc = check_search(name, s, n_policies, n_candidates, -1)) return rc;
    RefitArgs a{s->p, s->cdf, s->log_ratio, s->active, s->bins, s->elite_w, s->alpha, s->p_floor, s->n_bins, s->n_coord, n_candidates};
    const size_t lds = (size_t)s->n_bins * kRefitThreads * sizeof(double);
    hipLaunchKernelGGL(encounter_refit_kernel, dim3((unsigned)s->n_coord, (unsigned)n_policies), dim3(kRefitThreads), lds,
                       (hipStream_t)stream, a);
    return launched(name);
}
