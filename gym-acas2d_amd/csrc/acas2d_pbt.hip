// acas2d_pbt.hip -- what population-based training (Jaderberg et al. 2017) needs between two PPO iterations of a
// population, in TWO small launches with no host decision in between (include/acas2d.h):
//
//   member_episodes_kernel     acas2d_member_episodes_f32: the episodes that ended in a collection, per member -- count,
//                              outcome counts, summed length, summed return -- ADDED to device accumulators, and the
//                              members' score (mean return of the window) derived from the totals.
//   population_exploit_kernel  acas2d_population_exploit_f32: truncation selection on that score, the bit copy of a
//                              better member's parameters and Adam state into each of the worst, and the perturbation of
//                              the copied hyper-parameter row.
//
// Episodes.  One 1 024-thread workgroup per member k (columns [k EM, (k + 1) EM) of the collector's [T][E] buffers).  Wave w
// takes the rows w, w + 16, ...; lane l the columns l, l + 64, ... of a row, four column chunks in flight.  ep_return and
// ep_steps are loaded only where done != 0 and enter the sums through that branch alone, so whatever lies at the other
// positions (NaN, inf, INT32_MIN) reaches nothing.  The order of the additions is fixed -- in the lane: rows, then columns,
// ascending; in the wave: the xor tree 32, 16, 8, 4, 2, 1; across waves: 0 .. 15 in thread 0 -- and there are no atomics, so
// the same inputs give the same bits.  The return sum is carried in double.
//
// Exploit.  Grid (kCopyBlocks, K), 256 threads: the kCopyBlocks workgroups of member k each derive, from the K scores in
// LDS, member k's rank, its random donor and the copy condition (the same integers in each of them), and then share the
// copy: 15 rows (13 parameter tensors, adam_m, adam_v) moved as 16-byte words where source and destination are congruent
// modulo 16 bytes, as dwords otherwise (a member's row of adam_m is an odd number of floats).  Donors (rank < R) are only
// read and a recipient (rank >= K - R, 2R <= K) is written by its own workgroups only: in place without a race.
#include <float.h>

#include "acas2d_kernels.hpp"

namespace acas2d {
namespace {

// ---- per-member episode statistics ------------------------------------------------------------------------------------
constexpr int kEpThreads = 1024, kEpWaves = kEpThreads / 64;

struct EpisodesArgs {
    const uint8_t *done, *outcome;   // [T][E]
    const float* ep_return;          // [T][E], defined where done
    const int32_t* ep_steps;         // [T][E], defined where done
    int64_t *ep_count, *ep_outcomes, *ep_steps_sum;     // [K], [K][4], [K]
    double* ep_return_sum;           // [K]
    float* score;                    // [K]
    int64_t n_envs;
    uint32_t member_stride;          // EM
    int32_t n_steps;
};

// the wave's sum in every lane; a fixed tree (lane l adds lane l ^ 32, then ^ 16, ...): the same bits on every run
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int64_t wave_sum(int64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(kEpThreads) void member_episodes_kernel(EpisodesArgs a) {
    __shared__ double s_ret[kEpWaves];
    __shared__ int64_t s_int[kEpWaves][6];               // count, outcomes 0 .. 3, steps
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t k = blockIdx.x, EM = a.member_stride;
    const size_t E = (size_t)a.n_envs, col0 = (size_t)k * EM;

    // a lane sees fewer than 2^32 entries (each is a byte of `done` in memory): 32-bit counts, widened at the end
    uint32_t n = 0, no[4] = {0, 0, 0, 0};
    int64_t steps = 0;
    double ret = 0.0;
    const auto entry = [&](uint8_t d, uint8_t o, size_t at) __attribute__((always_inline)) {
        if (d) {                                         // the only way into the sums: nothing of a non-done position
            const float r = a.ep_return[at];
            const int32_t s = a.ep_steps[at];
            n += 1u;
#pragma unroll
            for (int j = 0; j < 4; ++j) no[j] += (o == j) ? 1u : 0u;
            steps += (int64_t)s - 1;                     // ep_steps is step() calls + 1
            ret += (double)r;
        }
    };
    for (int t = (int)wave; t < a.n_steps; t += kEpWaves) {
        const size_t row = (size_t)t * E + col0;
        uint32_t c = lane;
        for (; c + 192u < EM; c += 256u) {               // four chunks of 64 columns: eight byte loads before the first use
            uint8_t d[4], o[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { d[u] = a.done[row + c + 64u * u]; o[u] = a.outcome[row + c + 64u * u]; }
#pragma unroll
            for (int u = 0; u < 4; ++u) entry(d[u], o[u], row + c + 64u * u);
        }
        for (; c < EM; c += 64u) entry(a.done[row + c], a.outcome[row + c], row + c);
    }

    const double w_ret = wave_sum(ret);
    int64_t w_int[6] = {wave_sum((int64_t)n), wave_sum((int64_t)no[0]), wave_sum((int64_t)no[1]), wave_sum((int64_t)no[2]),
                        wave_sum((int64_t)no[3]), wave_sum(steps)};
    if (lane == 0) {
        s_ret[wave] = w_ret;
#pragma unroll
        for (int j = 0; j < 6; ++j) s_int[wave][j] = w_int[j];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = s_ret[0];
        int64_t v[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) v[j] = s_int[0][j];
        for (int w = 1; w < kEpWaves; ++w) {
            r += s_ret[w];
#pragma unroll
            for (int j = 0; j < 6; ++j) v[j] += s_int[w][j];
        }
        const int64_t count = a.ep_count[k] + v[0];
        const double total = a.ep_return_sum[k] + r;
        a.ep_count[k] = count;
#pragma unroll
        for (int j = 0; j < 4; ++j) a.ep_outcomes[(size_t)k * 4 + j] += v[1 + j];
        a.ep_steps_sum[k] += v[5];
        a.ep_return_sum[k] = total;
        a.score[k] = (float)(total / (double)count);     // 0 / 0: NaN where no episode ended
    }
}

// ---- exploit / explore -------------------------------------------------------------------------------------------------
constexpr int kPbtMaxMembers = 1024, kExThreads = 256, kCopyBlocks = 16, kRows = 15;

struct ExploitArgs {
    uint32_t* row[kRows];            // the 13 parameter stacks, adam_m, adam_v: [K][len]
    uint32_t len[kRows];             // floats per member
    int32_t* adam_step;              // [K]
    float* hyper;                    // [K][8]
    const float* score;              // [K]
    int32_t* donor;                  // [K]
    int32_t n_members, n_replace;
    uint32_t generation, seed_lo, seed_hi, perturb_mask;
    float factor_lo, factor_hi;
    float lo[8], hi[8];
};

// the rank of `key` held by member k: members with a greater key, and those with an equal key and a smaller index
__device__ __forceinline__ int rank_of(const float* keys, int K, float key, int k) {
    int r = 0;
    for (int j = 0; j < K; ++j) r += (keys[j] > key || (keys[j] == key && j < k)) ? 1 : 0;
    return r;
}

// n dwords from src to dst by the threads `me` of `nthreads`; 16-byte words where both ends allow them
__device__ __forceinline__ void copy_row(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, uint32_t n, uint32_t me,
                                         uint32_t nthreads) {
    if ((((uintptr_t)dst ^ (uintptr_t)src) & 15u) == 0 && n >= 8u) {
        uint32_t head = (uint32_t)((16u - ((uintptr_t)dst & 15u)) & 15u) >> 2;       // dwords up to a 16-byte boundary
        if (head > n) head = n;
        const uint32_t body = (n - head) >> 2, tail = head + 4u * body;
        if (me < head) dst[me] = src[me];
        const uint4* s4 = (const uint4*)(src + head);
        uint4* d4 = (uint4*)(dst + head);
        for (uint32_t i = me; i < body; i += nthreads) d4[i] = s4[i];
        if (me < n - tail) dst[tail + me] = src[tail + me];
    } else {
        for (uint32_t i = me; i < n; i += nthreads) dst[i] = src[i];
    }
}

__global__ __launch_bounds__(kExThreads) void population_exploit_kernel(ExploitArgs a) {
    __shared__ float keys[kPbtMaxMembers];
    __shared__ int s_rank[kExThreads / 64];
    __shared__ int s_donor;
    const int K = a.n_members, R = a.n_replace, k = (int)blockIdx.y;
    const uint32_t tid = threadIdx.x;
    for (int j = (int)tid; j < K; j += kExThreads) {
        const float s = a.score[j];
        keys[j] = (s != s) ? -__builtin_inff() : s;      // a NaN score ranks last
    }
    if (tid == 0) s_donor = k;
    __syncthreads();
    const float key = keys[k];
    // member k's rank: every thread a strided share of the members, then an integer sum (exact in any order)
    int part = 0;
    for (int j = (int)tid; j < K; j += kExThreads) part += (keys[j] > key || (keys[j] == key && j < k)) ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
    if ((tid & 63u) == 0) s_rank[tid >> 6] = part;
    __syncthreads();
    const int rank = s_rank[0] + s_rank[1] + s_rank[2] + s_rank[3];
    if (rank < K - R) {                                  // not a recipient (block-uniform)
        if (blockIdx.x == 0 && tid == 0) a.donor[k] = k;
        return;
    }
    const U4 w = philox4x32(U4{(uint32_t)k, a.generation, 0u, 0x70627431u}, a.seed_lo, a.seed_hi);
    const int rho = (int)__umulhi(w.x, (uint32_t)R);     // (uint64(w.x) * R) >> 32: a rank among the R best
    for (int j = (int)tid; j < K; j += kExThreads)
        if (rank_of(keys, K, keys[j], j) == rho) s_donor = j;        // ranks are a permutation: exactly one writer
    __syncthreads();
    const int d = s_donor;
    if (!(keys[d] > key)) {                              // the donor is not strictly better: nothing of member k changes
        if (blockIdx.x == 0 && tid == 0) a.donor[k] = k;
        return;
    }
    const uint32_t me = blockIdx.x * kExThreads + tid, nthreads = kCopyBlocks * kExThreads;
#pragma unroll
    for (int i = 0; i < kRows; ++i)
        copy_row(a.row[i] + (size_t)k * a.len[i], a.row[i] + (size_t)d * a.len[i], a.len[i], me, nthreads);
    if (blockIdx.x == 0) {
        if (tid < 8u) {                                  // explore: the donor's row, the masked slots times one of two factors
            const float h = a.hyper[(size_t)d * 8 + tid];
            const float f = ((w.y >> tid) & 1u) ? a.factor_hi : a.factor_lo;
            const float p = fminf(fmaxf(h * f, a.lo[tid]), a.hi[tid]);
            a.hyper[(size_t)k * 8 + tid] = ((a.perturb_mask >> tid) & 1u) ? p : h;
        }
        if (tid == 8u) a.adam_step[k] = a.adam_step[d];
        if (tid == 9u) a.donor[k] = d;
    }
}

bool finite_positive(float f) { return f > 0.0f && f <= FLT_MAX; }

}  // namespace
}  // namespace acas2d

using namespace acas2d;

extern "C" size_t acas2d_member_episodes_size(void) { return sizeof(Acas2dMemberEpisodes); }
extern "C" size_t acas2d_population_exploit_size(void) { return sizeof(Acas2dPopulationExploit); }

extern "C" int acas2d_member_episodes_f32(const Acas2dMemberEpisodes* m, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!m) { set_error("acas2d_member_episodes: NULL argument"); return ACAS2D_EINVAL; }
    if (!m->done || !m->outcome || !m->ep_return || !m->ep_steps || !m->ep_count || !m->ep_outcomes || !m->ep_steps_sum ||
        !m->ep_return_sum || !m->score) {
        set_error("acas2d_member_episodes: done, outcome, ep_return, ep_steps, ep_count, ep_outcomes, ep_steps_sum, "
                  "ep_return_sum and score are required");
        return ACAS2D_EINVAL;
    }
    if (m->n_steps < 1 || m->n_envs < 1 || m->n_members < 1 || m->n_members > 65535) {
        set_error("acas2d_member_episodes: n_steps = %d, n_envs = %lld (each at least 1), n_members = %d (1 .. 65535)",
                  m->n_steps, (long long)m->n_envs, m->n_members);
        return ACAS2D_EINVAL;
    }
    const int64_t K = m->n_members;
    if (K > 1 && (m->n_envs % K != 0 || (m->n_envs / K) % 64 != 0)) {
        set_error("acas2d_member_episodes: n_envs = %lld is not n_members = %d x a multiple of 64 (the rule of the collector "
                  "and of acas2d_gae_f32)", (long long)m->n_envs, m->n_members);
        return ACAS2D_EINVAL;
    }
    if (m->n_envs >= ((int64_t)1 << 31)) {
        set_error("acas2d_member_episodes: n_envs = %lld (less than 2^31 per call)", (long long)m->n_envs);
        return ACAS2D_EINVAL;
    }
    EpisodesArgs a{m->done, m->outcome, (const float*)m->ep_return, m->ep_steps, m->ep_count, m->ep_outcomes, m->ep_steps_sum,
                   m->ep_return_sum, (float*)m->score, m->n_envs, (uint32_t)(m->n_envs / K), m->n_steps};
    hipLaunchKernelGGL(member_episodes_kernel, dim3((unsigned)K), dim3(kEpThreads), 0, stream, a);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) { set_error("acas2d_member_episodes launch: %s", hipGetErrorString(err)); return ACAS2D_EHIP; }
    return ACAS2D_OK;
}

extern "C" int acas2d_population_exploit_f32(const Acas2dPopulationExploit* x, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!x) { set_error("acas2d_population_exploit: NULL argument"); return ACAS2D_EINVAL; }
    void* const rows[kRows] = {x->actor_w1, x->actor_b1, x->actor_w2, x->actor_b2, x->actor_w3, x->actor_b3, x->critic_w1,
                               x->critic_b1, x->critic_w2, x->critic_b2, x->critic_w3, x->critic_b3, x->log_std, x->adam_m,
                               x->adam_v};
    const void* const others[4] = {x->adam_step, x->hyper, x->score, x->donor};
    for (const void* p : rows)
        if (!p) { set_error("acas2d_population_exploit: every parameter stack, adam_m and adam_v are required"); return ACAS2D_EINVAL; }
    for (const void* p : others)
        if (!p) { set_error("acas2d_population_exploit: adam_step, hyper, score and donor are required"); return ACAS2D_EINVAL; }
    const int D = x->obs_dim;
    if (D != 8 && D != 11 && D != 14 && D != 17 && D != 29 && D != 53 && D != 101 && D != 197) {
        set_error("acas2d_population_exploit: obs_dim in {8, 11, 14, 17, 29, 53, 101, 197} (n_traffic 1, 2, 3, 4, 8, 16, 32, "
                  "64), got %d", D);
        return ACAS2D_EINVAL;
    }
    const int K = x->n_members, R = x->n_replace;
    if (K < 1 || K > kPbtMaxMembers) {
        set_error("acas2d_population_exploit: n_members = %d (1 .. %d: the scores are ranked in LDS)", K, kPbtMaxMembers);
        return ACAS2D_EINVAL;
    }
    if (R < 0 || 2 * (int64_t)R > K) {
        set_error("acas2d_population_exploit: n_replace = %d needs 0 <= 2 x n_replace <= n_members = %d (donors and recipients "
                  "must be disjoint)", R, K);
        return ACAS2D_EINVAL;
    }
    if (!finite_positive(x->factor_lo) || !finite_positive(x->factor_hi)) {
        set_error("acas2d_population_exploit: factor_lo = %g, factor_hi = %g (finite and positive)", (double)x->factor_lo,
                  (double)x->factor_hi);
        return ACAS2D_EINVAL;
    }
    for (int s = 0; s < 8; ++s)
        if (((x->perturb_mask >> s) & 1u) && !(x->lo[s] <= x->hi[s])) {
            set_error("acas2d_population_exploit: hyper slot %d is perturbed into [lo, hi] = [%g, %g], which is empty", s,
                      (double)x->lo[s], (double)x->hi[s]);
            return ACAS2D_EINVAL;
        }
    for (const void* out : {(const void*)x->donor, x->score}) {
        int same = 0;
        for (const void* p : rows) same += p == out;
        for (const void* p : others) same += p == out;
        if (same != 1) {
            set_error("acas2d_population_exploit: donor and score must not be one of the other buffers (every workgroup ranks "
                      "the scores while others write)");
            return ACAS2D_EINVAL;
        }
    }

    ExploitArgs a;
    const uint32_t net[6] = {64u * (uint32_t)D, 64u, 64u * 64u, 64u, 64u, 1u};
    const uint32_t ws = (uint32_t)acas2d_ppo_workspace_floats(D);
    for (int i = 0; i < kRows; ++i) {
        a.row[i] = (uint32_t*)rows[i];
        a.len[i] = i < 12 ? net[i % 6] : (i == 12 ? 1u : ws);
    }
    a.adam_step = x->adam_step; a.hyper = (float*)x->hyper; a.score = (const float*)x->score; a.donor = x->donor;
    a.n_members = K; a.n_replace = R;
    a.generation = x->generation; a.seed_lo = (uint32_t)x->seed; a.seed_hi = (uint32_t)(x->seed >> 32);
    a.perturb_mask = x->perturb_mask & 0xffu;
    a.factor_lo = x->factor_lo; a.factor_hi = x->factor_hi;
    for (int s = 0; s < 8; ++s) { a.lo[s] = x->lo[s]; a.hi[s] = x->hi[s]; }
    hipLaunchKernelGGL(population_exploit_kernel, dim3(kCopyBlocks, (unsigned)K), dim3(kExThreads), 0, stream, a);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) { set_error("acas2d_population_exploit launch: %s", hipGetErrorString(err)); return ACAS2D_EHIP; }
    return ACAS2D_OK;
}
