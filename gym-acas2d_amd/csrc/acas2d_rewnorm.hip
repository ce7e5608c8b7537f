// acas2d_rewnorm.hip -- SB3's VecNormalize(norm_obs=False, norm_reward=True) over the collector's [T][E] reward buffer, on
// the device between the collector and acas2d_gae_f32: every reward divided by the running standard deviation of the
// discounted return.  acas2d_reward_normalize_f32, include/acas2d.h; the arithmetic (all of it float64, every operation
// its own rounding: this unit is built with -ffp-contract=off like the GAE unit) is stated there.
//
// The arithmetic separates into four pieces, and the call is these four launches on the caller's stream, nothing else:
//
//   rewnorm_sweep_kernel    one lane per env, 64-thread workgroups, sweeping t = 0 ... T-1 like gae_kernel sweeps down:
//                           G = G * gamma_k + r, G[t][e] (double) into the workspace, G = 0 where done.  The only serial
//                           piece PER ENV; rows are coalesced wave-instructions, kRewnormDepth rows of loads in flight.
//   rewnorm_moments_kernel  one wavefront per (t, k): bm = sum_e G / EM, then bv = sum_e (G - bm)^2 / EM over member k's EM
//                           columns of row t.  T x K independent rows: the batch reduction that a per-step formulation
//                           would serialise (two workgroup reductions per step) runs at full width instead.
//   rewnorm_merge_kernel    one lane per member: the T Welford merges in order (a dozen dependent float64 operations and
//                           two divisions per step: the only piece serial in t ACROSS envs, and it touches 16 bytes a
//                           step), sqrt(var + epsilon) per (t, k) into the workspace, the statistics back into `stats`.
//   rewnorm_scale_kernel    element-wise: out[t][e] = (float)clamp(r / scale[t][k]).
//
// One launch would need a workgroup (or a grid) barrier twice per step for the batch moments -- T x 2 barriers in series,
// each with a cross-wave reduction behind it -- where the sweep above pays none; the workspace (8 bytes per sample) is what
// buys that.
//
// The order of the additions in the moments is fixed and a function of EM alone: lane l adds its columns l, l + 64, ...
// ascending (a lane past the row's end holds 0), then the wave adds along the xor tree 32, 16, 8, 4, 2, 1 -- the two
// operands of every tree addition are the same pair in both lanes, so every lane ends with the same bits.  No atomics.
// A row's result depends on nothing but the row, a member's merge on nothing but its own rows in order: the same inputs
// give the same bits; a call over T rows equals a call over the first T1 and one over the rest with the carried `returns`
// and `stats`; K members equal K calls on the column slices.
#include <float.h>
#include <math.h>

#include "acas2d_kernels.hpp"

namespace acas2d {
namespace {

constexpr int kRewnormDepth = 16;    // rows of loads in flight per lane of the sweep (acas2d_reward_norm_pipeline_depth())
constexpr int kScaleThreads = 256;

struct RewnormArgs {
    const float* reward;             // [T][E]
    const uint8_t* done;             // [T][E]
    float* out;                      // [T][E] (may be reward)
    double* returns;                 // [E]
    double* stats;                   // [K][3]: mean, var, count
    const double* gamma;             // [K]
    double* ws_g;                    // [T][E]     the discounted return after step t, before the reset
    double* ws_mom;                  // [T][K][2]  bm, bv
    double* ws_scale;                // [T][K]     sqrt(var + epsilon) after the merge of step t
    double epsilon, clip;
    int64_t n_envs;
    uint32_t member_stride;          // EM
    int32_t n_steps, n_members;
};

__device__ __forceinline__ float scrub(float r) {        // acas2d_gae_f32's: NaN -> 0, +-inf -> +-FLT_MAX
    return r != r ? 0.0f : fminf(fmaxf(r, -FLT_MAX), FLT_MAX);
}

// ---- the per-env sweep ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void rewnorm_sweep_kernel(RewnormArgs a) {
    constexpr int U = kRewnormDepth;
    const uint32_t lane = threadIdx.x;
    const uint32_t e0 = blockIdx.x * 64u;            // the wave's first env (n_envs < 2^31)
    // the member is the workgroup's: K > 1 needs EM % 64 == 0, K == 1 has member_stride == n_envs
    const uint32_t km = e0 / a.member_stride;
    if ((int64_t)e0 + lane >= a.n_envs) return;      // tail lanes of the last wave (K == 1 only)

    const double gamma = ((const double ACAS2D_AS4*)a.gamma)[km];
    const size_t E = (size_t)a.n_envs;
    const int T = a.n_steps;
    const float ACAS2D_AS1* reward = (const float ACAS2D_AS1*)a.reward + e0;
    const uint8_t ACAS2D_AS1* done = (const uint8_t ACAS2D_AS1*)a.done + e0;
    double ACAS2D_AS1* ws = (double ACAS2D_AS1*)a.ws_g + e0;

    // two register blocks of U rows, as in gae_kernel: slot i of `cur` holds row base + i, `nxt` the U rows above; the
    // loads of `nxt` are issued before the chain runs over `cur` (rows past T - 1 read row T - 1 and are never consumed)
    struct Rows { float r[U]; uint8_t d[U]; };
    const auto fetch = [&](Rows& b, int base, bool whole) __attribute__((always_inline)) {
        size_t o = (size_t)(base < T - 1 ? base : T - 1) * E;
#pragma unroll
        for (int i = 0; i < U; ++i) {
            b.r[i] = (reward + o)[lane]; b.d[i] = (done + o)[lane];
            o = (whole || base + i + 1 < T) ? o + E : o;
        }
    };
    Rows cur, nxt;
    fetch(cur, 0, T >= U);

    double G = a.returns[(size_t)e0 + lane];
    const auto row = [&](int i, int t) __attribute__((always_inline)) {
        const double r = (double)scrub(cur.r[i]);
        G = G * gamma + r;
        (ws + (size_t)t * E)[lane] = G;
        G = cur.d[i] ? 0.0 : G;
    };
    int base = 0;
    for (; base + U <= T; base += U) {               // whole blocks of U rows
        fetch(nxt, base + U, base + 2 * U <= T);
        __builtin_amdgcn_sched_barrier(0);           // (nothing moves across, as in gae_kernel)
#pragma unroll
        for (int i = 0; i < U; ++i) { row(i, base + i); __builtin_amdgcn_sched_barrier(0); }
        cur = nxt;
    }
#pragma unroll
    for (int i = 0; i < U - 1; ++i)                  // the last T - base < U rows: already in their slots
        if (base + i < T) row(i, base + i);
    a.returns[(size_t)e0 + lane] = G;
}

// ---- the per-row batch moments ----------------------------------------------------------------------------------------
// the wave's sum in every lane; a fixed tree (lane l adds lane l ^ 32, then ^ 16, ...): the same bits on every run
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(64) void rewnorm_moments_kernel(RewnormArgs a) {
    const uint32_t lane = threadIdx.x, EM = a.member_stride, K = (uint32_t)a.n_members;
    for (size_t rowk = blockIdx.x; rowk < (size_t)a.n_steps * K; rowk += gridDim.x) {        // (t, k), wave-uniform
        const size_t t = rowk / K, k = rowk % K;
        const double ACAS2D_AS1* g = (const double ACAS2D_AS1*)a.ws_g + t * (size_t)a.n_envs + k * EM;
        const double n = (double)EM;
        // four columns in flight per lane; added in ascending order (the loads do not depend on the sum)
        double s = 0.0;
        uint32_t c = lane;
        for (; c + 192u < EM; c += 256u) {                   // (EM < 2^31: no wrap)
            const double x0 = g[c], x1 = g[c + 64u], x2 = g[c + 128u], x3 = g[c + 192u];
            s += x0; s += x1; s += x2; s += x3;
        }
        for (; c < EM; c += 64u) s += g[c];
        const double bm = wave_sum(s) / n;
        double q = 0.0;
        c = lane;
        for (; c + 192u < EM; c += 256u) {                   // (EM < 2^31: no wrap)
            const double d0 = g[c] - bm, d1 = g[c + 64u] - bm, d2 = g[c + 128u] - bm, d3 = g[c + 192u] - bm;
            q += d0 * d0; q += d1 * d1; q += d2 * d2; q += d3 * d3;
        }
        for (; c < EM; c += 64u) { const double d = g[c] - bm; q += d * d; }
        const double bv = wave_sum(q) / n;
        if (lane == 0) { a.ws_mom[2 * rowk] = bm; a.ws_mom[2 * rowk + 1] = bv; }
    }
}

// ---- the merges in t: RunningMeanStd.update_from_moments, one lane per member -------------------------------------------
__global__ __launch_bounds__(64) void rewnorm_merge_kernel(RewnormArgs a) {
    const uint32_t k = blockIdx.x * 64u + threadIdx.x, K = (uint32_t)a.n_members;
    if (k >= K) return;
    const double* __restrict__ mom = a.ws_mom;
    double* __restrict__ scale = a.ws_scale;
    double mean = a.stats[3 * (size_t)k], var = a.stats[3 * (size_t)k + 1], count = a.stats[3 * (size_t)k + 2];
    const double n = (double)a.member_stride, eps = a.epsilon;
    const int T = a.n_steps;
#pragma unroll 8
    for (int t = 0; t < T; ++t) {                    // (unrolled: the loads of the rows ahead do not wait for the chain)
        const size_t at = (size_t)t * K + k;
        const double bm = mom[2 * at], bv = mom[2 * at + 1];
        const double delta = bm - mean, tot = count + n;
        const double mean_new = mean + delta * n / tot;
        const double m2 = var * count + bv * n + delta * delta * count * n / tot;
        var = m2 / tot;
        mean = mean_new;
        count = tot;
        scale[at] = sqrt(var + eps);
    }
    a.stats[3 * (size_t)k] = mean; a.stats[3 * (size_t)k + 1] = var; a.stats[3 * (size_t)k + 2] = count;
}

// ---- the element-wise division ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kScaleThreads) void rewnorm_scale_kernel(RewnormArgs a) {
    const size_t E = (size_t)a.n_envs, chunks = (E + kScaleThreads - 1) / kScaleThreads;
    const uint32_t K = (uint32_t)a.n_members;
    const double clip = a.clip;
    for (size_t tile = blockIdx.x; tile < (size_t)a.n_steps * chunks; tile += gridDim.x) {   // (t, 256 envs), uniform
        const size_t t = tile / chunks;
        const size_t e = (tile % chunks) * kScaleThreads + threadIdx.x;
        if (e >= E) continue;
        const uint32_t km = (uint32_t)e / a.member_stride;
        const double s = a.ws_scale[t * K + km];
        const double r = (double)scrub(a.reward[t * E + e]);
        a.out[t * E + e] = (float)fmin(fmax(r / s, -clip), clip);
    }
}

size_t align_up(size_t n) { return (n + 15) & ~(size_t)15; }

}  // namespace
}  // namespace acas2d

using namespace acas2d;

extern "C" size_t acas2d_reward_norm_size(void) { return sizeof(Acas2dRewardNorm); }
extern "C" int acas2d_reward_norm_pipeline_depth(void) { return kRewnormDepth; }

extern "C" size_t acas2d_reward_norm_workspace_bytes(int64_t n_envs, int32_t n_steps, int32_t n_members) {
    if (n_envs < 1 || n_steps < 1 || n_members < 1 || n_envs >= ((int64_t)1 << 31)) return 0;
    const size_t T = (size_t)n_steps, E = (size_t)n_envs, K = (size_t)n_members;
    return align_up(T * E * sizeof(double)) + align_up(T * K * 2 * sizeof(double)) + align_up(T * K * sizeof(double));
}

extern "C" int acas2d_reward_normalize_f32(const Acas2dRewardNorm* n, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!n) { set_error("acas2d_reward_normalize: NULL argument"); return ACAS2D_EINVAL; }
    if (!n->reward || !n->done || !n->out || !n->returns || !n->stats || !n->gamma || !n->workspace) {
        set_error("acas2d_reward_normalize: reward, done, out, returns, stats, gamma and workspace are required");
        return ACAS2D_EINVAL;
    }
    if (n->n_steps < 1 || n->n_envs < 1 || n->n_members < 1) {
        set_error("acas2d_reward_normalize: n_steps = %d, n_envs = %lld, n_members = %d (each at least 1)", n->n_steps,
                  (long long)n->n_envs, n->n_members);
        return ACAS2D_EINVAL;
    }
    if (n->n_envs >= ((int64_t)1 << 31)) {
        set_error("acas2d_reward_normalize: n_envs = %lld (less than 2^31 per call)", (long long)n->n_envs); return ACAS2D_EINVAL; }
    const int64_t K = n->n_members;
    if (K > 1 && (n->n_envs % K != 0 || (n->n_envs / K) % 64 != 0)) {
        set_error("acas2d_reward_normalize: n_envs = %lld is not n_members = %d x a multiple of 64 (a wavefront's envs belong to "
                  "one member)", (long long)n->n_envs, n->n_members);
        return ACAS2D_EINVAL;
    }
    if (!(n->epsilon > 0.0 && n->epsilon < (double)INFINITY) || !(n->clip > 0.0 && n->clip < (double)INFINITY)) {
        set_error("acas2d_reward_normalize: epsilon = %g, clip = %g (each finite and positive)", n->epsilon, n->clip);
        return ACAS2D_EINVAL;
    }
    const void* all[] = {n->reward, n->done, n->out, n->returns, n->stats, n->gamma, n->workspace};
    const int written[] = {2, 3, 4, 6};              // out, returns, stats, workspace
    for (int w : written)
        for (int j = 0; j < 7; ++j)
            if (j != w && all[w] == all[j] && !(w == 2 && j == 0)) {
                set_error("acas2d_reward_normalize: out, returns, stats and workspace must not be another buffer of the struct "
                          "(out == reward, in place, is the one exception)");
                return ACAS2D_EINVAL;
            }
    if (((uintptr_t)n->returns | (uintptr_t)n->stats | (uintptr_t)n->gamma | (uintptr_t)n->workspace) & 7u) {
        set_error("acas2d_reward_normalize: returns, stats, gamma and workspace hold doubles: 8-byte aligned"); return ACAS2D_EINVAL; }

    const size_t T = (size_t)n->n_steps, E = (size_t)n->n_envs;
    char* ws = (char*)n->workspace;
    RewnormArgs a{(const float*)n->reward, n->done, (float*)n->out, n->returns, n->stats, n->gamma,
                  (double*)ws, (double*)(ws + align_up(T * E * sizeof(double))),
                  (double*)(ws + align_up(T * E * sizeof(double)) + align_up(T * (size_t)K * 2 * sizeof(double))),
                  n->epsilon, n->clip, n->n_envs, (uint32_t)(n->n_envs / K), n->n_steps, n->n_members};
    const auto capped = [](size_t blocks) { return dim3((unsigned)(blocks < ((size_t)1 << 20) ? blocks : ((size_t)1 << 20))); };
    hipLaunchKernelGGL(rewnorm_sweep_kernel, dim3((unsigned)((E + 63) / 64)), dim3(64), 0, stream, a);
    hipLaunchKernelGGL(rewnorm_moments_kernel, capped(T * (size_t)K), dim3(64), 0, stream, a);
    hipLaunchKernelGGL(rewnorm_merge_kernel, dim3((unsigned)((K + 63) / 64)), dim3(64), 0, stream, a);
    hipLaunchKernelGGL(rewnorm_scale_kernel, capped(T * ((E + kScaleThreads - 1) / kScaleThreads)), dim3(kScaleThreads), 0,
                       stream, a);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) { set_error("acas2d_reward_normalize launch: %s", hipGetErrorString(err)); return ACAS2D_EHIP; }
    return ACAS2D_OK;
}
