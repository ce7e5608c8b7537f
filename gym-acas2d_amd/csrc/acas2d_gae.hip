// acas2d_gae.hip -- what lies between the collector and the minibatch update of a PPO iteration, in ONE launch: the critic's
// value of the last observation (optional) and SB3's RolloutBuffer.compute_returns_and_advantage (GAE) over the
// collector's [T][E] buffers.  acas2d_gae_f32, include/acas2d.h.
//
//   gae_kernel<D>   one lane per env, 64-thread workgroups (E = 1 024 gives 16 wavefronts: one per workgroup spreads them
//                   over 16 CUs), sweeping t = T-1 ... 0.  Consecutive lanes hold consecutive envs, so every row access
//                   (reward[t], value[t], done[t], adv[t], ret[t]) is one coalesced wave-instruction.
//
// The bit contract.  Per (t, e) every operation is its own float32 rounding, in the order ppo.compute_gae's torch ops
// take them (this unit is built with -ffp-contract=off like the env kernels, so nothing fuses):
//     r     = scrub(reward[t][e])                       NaN -> 0, +-inf -> +-FLT_MAX   (torch.nan_to_num(x, nan=0.0))
//     nt    = done[t][e] ? 0.0f : 1.0f
//     nv    = (t == T-1) ? last_value[e] : value[t+1][e]
//     delta = ((r + ((gamma_k * nv) * nt)) - value[t][e])
//     last  = delta + ((gl_k * nt) * last)              last starts at 0
//     adv[t][e] = last;  ret[t][e] = last + value[t][e]
// The multiplications by nt stay multiplications (0 * inf = NaN, as in torch).  T is NOT split across waves: composing
// affine maps would round differently.
//
// The software pipeline.  Only the five-operation chain above is serial; the loads of the rows below t do not depend on
// it.  A lane holds two blocks of kGaeDepth = 16 rows (reward, value, done: 2 x 48 VGPRs): the chain runs over one while
// the 48 loads of the next, all issued before the block's first row, arrive.  Why 16: one row costs the wave about 60
// cycles (the chain at ~8 cycles per dependent VALU op plus the issue of its loads and two stores), an HBM miss about
// 900, so a block of 16 rows covers a miss; 48 loads + 32 stores per block also stay near the 63 memory operations
// s_waitcnt can count, and the 16 wavefronts of a 1 024-env sweep run one per SIMD, where registers are free.
//
// The bootstrap value.  With last_value == NULL the lane evaluates the critic on obs_last[e] itself: policy_mlp<D>() of
// acas2d_kernels.hpp on the transposed value-net stacks, a non-finite entry fed as 0 -- the instruction sequence the
// collector's `values` come from, so the result has the bits values[0] of a collection started on that observation has.
// Member k (envs [k EM, (k + 1) EM), EM a multiple of 64 for K > 1) is wave-uniform: its gamma, gamma x lambda and
// critic weights are scalar loads, as in Mode::CollectSet.
#include <float.h>

#include "acas2d_kernels.hpp"

namespace acas2d {
namespace {

constexpr int kGaeDepth = 16;        // rows in flight per lane (acas2d_gae_pipeline_depth())

struct GaeArgs {
    const float *reward, *value;     // [T][E]
    const uint8_t* done;             // [T][E]
    float *adv, *ret;                // [T][E]
    const float* last_value;         // [E] or NULL (D > 0: the critic runs here)
    const float* obs_last;           // [E][D]
    const float *v1t, *vb1, *v2t, *vb2, *v3, *vb3;      // [K] stacks, Acas2dActorCritic's layout
    const float *gamma, *gamma_lambda;                  // [K]
    float* last_value_out;           // [E] or NULL
    int32_t* nan_count;              // [K] or NULL
    int64_t n_envs;
    uint32_t member_stride;
    int32_t n_steps;
};

__device__ __forceinline__ float scrub(float r) {        // torch.nan_to_num(r, nan=0.0)
    return r != r ? 0.0f : fminf(fmaxf(r, -FLT_MAX), FLT_MAX);       // (selects and min / max: no branch in the sweep)
}

// D == 0: last_value is given; otherwise the compile-time observation width of the bootstrap
template <int D>
__global__ __launch_bounds__(64) void gae_kernel(GaeArgs a) {
    constexpr int U = kGaeDepth;
    const uint32_t lane = threadIdx.x;
    const uint32_t e0 = blockIdx.x * 64u;            // the wave's first env (n_envs < 2^31)
    // the member is the workgroup's: K > 1 needs EM % 64 == 0, K == 1 has member_stride == n_envs
    const uint32_t km = e0 / a.member_stride;
    if ((int64_t)e0 + lane >= a.n_envs) return;      // tail lanes of the last wave (K == 1 only)

    // ---- the bootstrap value: given, or the critic on the last observation (the collector's arithmetic)
    float nv;
    if constexpr (D == 0) {
        nv = a.last_value[(size_t)e0 + lane];
    } else {
        float x[D];
        const float* xo = a.obs_last + ((size_t)e0 + lane) * D;
#pragma unroll
        for (int i = 0; i < D; ++i) x[i] = (xo[i] == xo[i] && fabsf(xo[i]) < __builtin_inff()) ? xo[i] : 0.0f;
        nv = policy_mlp<D>(a.v1t + (size_t)km * (D * kPolicyHidden), a.vb1 + (size_t)km * kPolicyHidden,
                           a.v2t + (size_t)km * (kPolicyHidden * kPolicyHidden), a.vb2 + (size_t)km * kPolicyHidden,
                           a.v3 + (size_t)km * kPolicyHidden, a.vb3 + km, x);
    }
    if (a.last_value_out) a.last_value_out[(size_t)e0 + lane] = nv;

    const float gamma = ((const float ACAS2D_AS4*)a.gamma)[km];
    const float gl = ((const float ACAS2D_AS4*)a.gamma_lambda)[km];
    const size_t E = (size_t)a.n_envs;
    const int T = a.n_steps;
    // every row address is (wave-uniform base of the row: scalar arithmetic) + lane: one 32-bit lane offset for all of them
    const float ACAS2D_AS1* reward = (const float ACAS2D_AS1*)a.reward + e0;
    const float ACAS2D_AS1* value = (const float ACAS2D_AS1*)a.value + e0;
    const uint8_t ACAS2D_AS1* done = (const uint8_t ACAS2D_AS1*)a.done + e0;
    float ACAS2D_AS1* adv = (float ACAS2D_AS1*)a.adv + e0;
    float ACAS2D_AS1* ret = (float ACAS2D_AS1*)a.ret + e0;

    // two register blocks of U rows: slot i of `cur` holds row top - i, `nxt` receives the U rows below it.  All loads of
    // `nxt` are issued BEFORE the chain runs over `cur`, so they have a whole block of serial arithmetic to arrive in
    // (rows below 0 are clamped to row 0 and never consumed)
    struct Rows { float r[U], v[U]; uint8_t d[U]; };
    // whole == true: every row top .. top - U + 1 exists (one scalar subtraction per row); else rows below 0 read row 0
    const auto fetch = [&](Rows& b, int top, bool whole) __attribute__((always_inline)) {
        size_t o = (size_t)(top > 0 ? top : 0) * E;
#pragma unroll
        for (int i = 0; i < U; ++i) {
            b.r[i] = (reward + o)[lane]; b.v[i] = (value + o)[lane]; b.d[i] = (done + o)[lane];
            o = (whole || top - i > 0) ? o - E : 0;
        }
    };
    Rows cur, nxt;
    fetch(cur, T - 1, false);

    int nans = 0;                    // wave-uniform: NaN rewards of this wave's envs
    float last = 0.0f;
    // one row of the serial chain, from slot i of `cur`
    const auto row = [&](int i, int t) __attribute__((always_inline)) {
        const float rw = cur.r[i], v = cur.v[i];
        nans += __popcll(__ballot(rw != rw));
        const float r = scrub(rw);
        const float nt = cur.d[i] ? 0.0f : 1.0f;
        const float delta = (r + ((gamma * nv) * nt)) - v;
        last = delta + ((gl * nt) * last);
        const size_t o = (size_t)t * E;
        (adv + o)[lane] = last;
        (ret + o)[lane] = last + v;
        nv = v;
    };
    int top = T - 1;
    for (; top >= U - 1; top -= U) {             // whole blocks of U rows
        if (top - U >= U - 1) fetch(nxt, top - U, true);
        else fetch(nxt, top - U, false);
        // (nothing moves across: left alone, hipcc hoists the rows' chain-independent arithmetic above the loads, issues
        // them halfway down the block and waits for them at its end)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < U; ++i) { row(i, top - i); __builtin_amdgcn_sched_barrier(0); }
        cur = nxt;
    }
#pragma unroll
    for (int i = 0; i < U - 1; ++i)              // the last top + 1 < U rows: already in their slots
        if (top - i >= 0) row(i, top - i);
    if (a.nan_count && nans != 0 && lane == 0) atomicAdd(a.nan_count + km, nans);
}

template <int D>
int launch_gae(const GaeArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL((gae_kernel<D>), dim3((unsigned)((a.n_envs + 63) / 64)), dim3(64), 0, stream, a);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) { set_error("acas2d_gae launch: %s", hipGetErrorString(err)); return ACAS2D_EHIP; }
    return ACAS2D_OK;
}

}  // namespace
}  // namespace acas2d

using namespace acas2d;

extern "C" size_t acas2d_gae_size(void) { return sizeof(Acas2dGae); }
extern "C" int acas2d_gae_pipeline_depth(void) { return kGaeDepth; }

extern "C" int acas2d_gae_f32(const Acas2dGae* g, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!g) { set_error("acas2d_gae: NULL argument"); return ACAS2D_EINVAL; }
    if (!g->reward || !g->value || !g->done || !g->adv || !g->ret || !g->gamma || !g->gamma_lambda) {
        set_error("acas2d_gae: reward, value, done, adv, ret, gamma and gamma_lambda are required"); return ACAS2D_EINVAL; }
    if (g->n_steps < 1 || g->n_envs < 1 || g->n_members < 1) {
        set_error("acas2d_gae: n_steps = %d, n_envs = %lld, n_members = %d (each at least 1)", g->n_steps, (long long)g->n_envs,
                  g->n_members);
        return ACAS2D_EINVAL;
    }
    const int64_t K = g->n_members;
    if (K > 1 && (g->n_envs % K != 0 || (g->n_envs / K) % 64 != 0)) {
        set_error("acas2d_gae: n_envs = %lld is not n_members = %d x a multiple of 64 (a wavefront's envs belong to one member)",
                  (long long)g->n_envs, g->n_members);
        return ACAS2D_EINVAL;
    }
    if (g->n_envs >= ((int64_t)1 << 31)) {
        set_error("acas2d_gae: n_envs = %lld (less than 2^31 per call)", (long long)g->n_envs); return ACAS2D_EINVAL; }
    if (!g->last_value && !g->obs_last) {
        set_error("acas2d_gae: pass last_value, or obs_last and the critic for the bootstrap value"); return ACAS2D_EINVAL; }
    const bool bootstrap = !g->last_value;
    const int D = g->obs_dim;
    if (bootstrap) {
        if (D != 8 && D != 11 && D != 14 && D != 17 && D != 29) {
            set_error("acas2d_gae: the in-kernel bootstrap value is built for obs_dim in {8, 11, 14, 17, 29} (n_traffic 1, 2, 3, "
                      "4, 8), got %d -- the wide widths (53, 101, 197) must pass last_value", D);
            return ACAS2D_EINVAL;
        }
        if (!g->v1t || !g->vb1 || !g->v2t || !g->vb2 || !g->v3 || !g->vb3) {
            set_error("acas2d_gae: the in-kernel bootstrap value needs the critic's six stacks v1t .. vb3"); return ACAS2D_EINVAL; }
    }
    const void* inputs[] = {g->reward, g->value, g->done, g->last_value, g->obs_last, g->v1t, g->vb1, g->v2t, g->vb2, g->v3,
                            g->vb3, g->gamma, g->gamma_lambda, g->last_value_out, g->nan_count};
    for (const void* p : inputs)
        if (p && (p == g->adv || p == g->ret)) {
            set_error("acas2d_gae: adv and ret must not be one of the other buffers (the sweep reads row t - 16 while it "
                      "writes row t)");
            return ACAS2D_EINVAL;
        }
    if (g->adv == g->ret) { set_error("acas2d_gae: adv and ret must be two buffers"); return ACAS2D_EINVAL; }

    GaeArgs a{(const float*)g->reward, (const float*)g->value, g->done, (float*)g->adv, (float*)g->ret,
              (const float*)g->last_value, (const float*)g->obs_last, (const float*)g->v1t, (const float*)g->vb1,
              (const float*)g->v2t, (const float*)g->vb2, (const float*)g->v3, (const float*)g->vb3, (const float*)g->gamma,
              (const float*)g->gamma_lambda, (float*)g->last_value_out, g->nan_count, g->n_envs, (uint32_t)(g->n_envs / K), g->n_steps};
    if (!bootstrap) return launch_gae<0>(a, stream);
    switch (D) {
        case 8: return launch_gae<8>(a, stream);
        case 11: return launch_gae<11>(a, stream);
        case 14: return launch_gae<14>(a, stream);
        case 17: return launch_gae<17>(a, stream);
        default: return launch_gae<29>(a, stream);
    }
}
