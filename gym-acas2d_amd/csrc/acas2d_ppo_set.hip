// acas2d_ppo_set.hip -- one PPO minibatch update of K independent SB3 MlpPolicy actor-critics ("members" of a population:
// the seeds of a sweep, or its hyper-parameter sets) as TWO launches, whatever K is.  acas2d_ppo.hip gives one learner
// 128 single-wave workgroups at a minibatch of 4 096 and one workgroup for Adam on a device with 256 CUs; here the K
// learners lie side by side in the same two launches.
//
//   ppo_grad_set_kernel   grid (ceil(n_rows / 64), 2, K): blockIdx.z is the member, and per member the arithmetic is
//                         ppo_grad_kernel<D>'s, chain for chain (acas2d_ppo.hip: one wave per 64 samples and network, the
//                         weights through scalar loads, the advantage statistics of the member's WHOLE minibatch
//                         idx[k][.] recomputed by every actor wave, per-sample vectors in LDS with row stride 65, float
//                         atomics into grad[k]).  The member's parameters are slices of [K][...] stacks, its clip_range
//                         and vf_coef come from hyper[k] by scalar load.  The rollout buffer is ONE flat buffer shared by
//                         all members; idx holds its global row numbers.
//   ppo_apply_set_kernel  grid (K), 1 024 threads: ppo_apply_kernel's norm, clip_grad_norm_ coefficient, Adam and zeroing
//                         on member k's slices, with hyper[k] and adam_step[k].
//
// Self-contained on purpose: acas2d_ppo.hip's kernels take their hyper-parameters as launch constants and have no member
// dimension, and that unit's code stays as it is.  Only the layout helpers of acas2d_ppo.hpp are shared.
// Run-to-run: as for the sibling, the per-wave partial gradients are added to grad[k] with float atomics, whose order is
// not fixed, so two runs of the same update agree to float32 rounding of the sums (~1e-7 relative), not bit for bit.
// Out of scope (rejected): float64, the wide widths (obs_dim 53 / 101 / 197: acas2d_ppo_update_wide_f32, one learner per
// call), members with different n_rows.
#include <atomic>

#include "acas2d_ppo.hpp"

namespace acas2d {
using namespace ppo;

namespace {

// the 13 parameter stacks in FusedUpdate's order (actor w1 b1 w2 b2 w3 b3, critic likewise, log_std): [K][...]
struct SetParams { float* p[13]; };

__host__ __device__ constexpr int seg_count(int D, int k) {
    return k == 12 ? 1 : (k % 6 == 0 ? kH * D : (k % 6 == 2 ? kH * kH : (k % 6 == 5 ? 1 : kH)));
}

template <int D>
__global__ __launch_bounds__(64) void ppo_grad_set_kernel(SetParams prm, const float* obs, const float* act,
                                                          const float* old_logp, const float* adv, const float* ret,
                                                          const int64_t* idx_all, int B, const float* hyper, float* grad_all,
                                                          float* stats_all) {
    extern __shared__ float lds[];
    float* l_h1 = lds;                       // [64][65]
    float* l_h2 = l_h1 + 64 * kRow;
    float* l_dz1 = l_h2 + 64 * kRow;
    float* l_dz2 = l_dz1 + 64 * kRow;
    float* l_x = l_dz2 + 64 * kRow;          // [64][D + 1]
    float* l_do = l_x + 64 * (D + 1);        // [64]
    const int lane = threadIdx.x;
    const bool is_actor = blockIdx.y == 0;
    // ---- the member: its slices of the stacks, its minibatch, its gradient block, its two hyper-parameters
    const size_t m = blockIdx.z;
    const auto net = [&](int i) -> const float* { return is_actor ? prm.p[i] : prm.p[6 + i]; };
    const float ACAS2D_C4* w1 = (const float ACAS2D_C4*)(net(0) + m * (kH * D));
    const float ACAS2D_C4* b1 = (const float ACAS2D_C4*)(net(1) + m * kH);
    const float ACAS2D_C4* w2 = (const float ACAS2D_C4*)(net(2) + m * (kH * kH));
    const float ACAS2D_C4* b2 = (const float ACAS2D_C4*)(net(3) + m * kH);
    const float ACAS2D_C4* w3 = (const float ACAS2D_C4*)(net(4) + m * kH);
    const float ACAS2D_C4* b3 = (const float ACAS2D_C4*)(net(5) + m);
    const float* log_std_p = prm.p[12] + m;
    const int64_t* idx = idx_all + m * (size_t)B;
    float* grad = grad_all + m * (size_t)(2 * net_size(D) + 1);
    float* stats = stats_all + m * 8;
    const float ACAS2D_C4* hy = (const float ACAS2D_C4*)(hyper + m * 8);
    const float clip_range = hy[0], vf_coef = hy[1];

    const int row = blockIdx.x * 64 + lane;
    const bool live = row < B;
    const int64_t s = idx[live ? row : 0];

    // ---- the minibatch's advantage statistics (SB3 normalises per minibatch; torch.std is Bessel-corrected)
    float a_mean = 0.0f, a_std = 1.0f;
    if (is_actor) {
        float sum = 0.0f;
        for (int i = lane; i < B; i += 64) sum += adv[idx[i]];
        a_mean = wave_sum(sum) / (float)B;
        float sq = 0.0f;
        for (int i = lane; i < B; i += 64) { const float d = adv[idx[i]] - a_mean; sq = fmaf(d, d, sq); }
        a_std = sqrtf(wave_sum(sq) / (float)(B > 1 ? B - 1 : 1));
    }

    // ---- forward: obs -> Linear(D, 64) tanh -> Linear(64, 64) tanh -> Linear(64, 1), weights by scalar loads
    float x[D];
#pragma unroll
    for (int k = 0; k < D; ++k) { x[k] = obs[s * D + k]; l_x[lane * (D + 1) + k] = x[k]; }
    for (int i = 0; i < kH; ++i) {
        float z = b1[i];
#pragma unroll
        for (int k = 0; k < D; ++k) z = fmaf(w1[i * D + k], x[k], z);
        l_h1[lane * kRow + i] = tanhf(z);
    }
    float h1[kH];
#pragma unroll
    for (int k = 0; k < kH; ++k) h1[k] = l_h1[lane * kRow + k];
    float out = b3[0];
    for (int i = 0; i < kH; ++i) {
        float z = b2[i];
#pragma unroll
        for (int k = 0; k < kH; ++k) z = fmaf(w2[i * kH + k], h1[k], z);
        const float h2 = tanhf(z);
        l_h2[lane * kRow + i] = h2;
        out = fmaf(w3[i], h2, out);
    }

    // ---- d loss / d output (SB3 PPO.train(): clipped surrogate on minibatch-normalised advantages, MSE value loss)
    float dout = 0.0f, dls = 0.0f, pg_s = 0.0f, vf_s = 0.0f;
    if (live) {
        if (is_actor) {
            const float ls = log_std_p[0], inv_var = expf(-2.0f * ls);
            const float diff = act[s] - out;
            const float logp = -0.5f * diff * diff * inv_var - ls - 0.9189385332046727f;
            const float a = (adv[s] - a_mean) / (a_std + 1e-8f);
            const float ratio = expf(logp - old_logp[s]);
            const float surr1 = a * ratio, surr2 = a * fminf(fmaxf(ratio, 1.0f - clip_range), 1.0f + clip_range);
            pg_s = -fminf(surr1, surr2) / (float)B;
            const float dlogp = (surr1 <= surr2) ? -(a * ratio) / (float)B : 0.0f;     // torch.min: ties go to the first operand
            dout = dlogp * diff * inv_var;                       // d logp / d mean
            dls = dlogp * (diff * diff * inv_var - 1.0f);        // d logp / d log_std
        } else {
            const float e = out - ret[s];
            vf_s = e * e / (float)B;
            dout = vf_coef * 2.0f * e / (float)B;
        }
    }
    l_do[lane] = dout;

    // ---- backward to the pre-activations: dz2 = dout w3 (1 - h2^2), dh1 = W2^T dz2, dz1 = dh1 (1 - h1^2)
    float dh1[kH];
#pragma unroll
    for (int k = 0; k < kH; ++k) dh1[k] = 0.0f;
    for (int i = 0; i < kH; ++i) {
        const float h2 = l_h2[lane * kRow + i];
        const float dz2 = dout * w3[i] * (1.0f - h2 * h2);
        l_dz2[lane * kRow + i] = dz2;
#pragma unroll
        for (int k = 0; k < kH; ++k) dh1[k] = fmaf(w2[i * kH + k], dz2, dh1[k]);
    }
#pragma unroll
    for (int k = 0; k < kH; ++k) l_dz1[lane * kRow + k] = dh1[k] * (1.0f - h1[k] * h1[k]);
    __syncthreads();

    // ---- weight gradients: thread t takes row t of every weight matrix, summed over the wave's 64 samples
    float* g = grad + (is_actor ? 0 : net_size(D));
    const int t = lane;
    {
        float acc[kH];
#pragma unroll
        for (int j = 0; j < kH; ++j) acc[j] = 0.0f;
        float bsum = 0.0f;
        for (int q = 0; q < 64; ++q) {
            const float dz = l_dz2[q * kRow + t];
            bsum += dz;
#pragma unroll
            for (int j = 0; j < kH; ++j) acc[j] = fmaf(dz, l_h1[q * kRow + j], acc[j]);
        }
#pragma unroll
        for (int j = 0; j < kH; ++j) atomicAdd(g + off_w2(D) + t * kH + j, acc[j]);
        atomicAdd(g + off_b2(D) + t, bsum);
    }
    {
        float acc[D];
#pragma unroll
        for (int k = 0; k < D; ++k) acc[k] = 0.0f;
        float bsum = 0.0f, w3sum = 0.0f;
        for (int q = 0; q < 64; ++q) {
            const float dz = l_dz1[q * kRow + t];
            bsum += dz;
            w3sum = fmaf(l_do[q], l_h2[q * kRow + t], w3sum);
#pragma unroll
            for (int k = 0; k < D; ++k) acc[k] = fmaf(dz, l_x[q * (D + 1) + k], acc[k]);
        }
#pragma unroll
        for (int k = 0; k < D; ++k) atomicAdd(g + t * D + k, acc[k]);
        atomicAdd(g + off_b1(D) + t, bsum);
        atomicAdd(g + off_w3(D) + t, w3sum);
    }
    const float dsum = wave_sum(dout), lsum = wave_sum(dls), pgsum = wave_sum(pg_s), vfsum = wave_sum(vf_s);
    if (lane == 0) {
        atomicAdd(g + off_b3(D), dsum);
        if (is_actor) { atomicAdd(grad + 2 * net_size(D), lsum); atomicAdd(stats + 0, pgsum); }
        else atomicAdd(stats + 1, vfsum);
    }
}

// clip_grad_norm_ + Adam for all parameters of member blockIdx.x, in place; the gradient and the statistics accumulate
// for ONE minibatch.  hyper[k]: clip_range, vf_coef, ent_coef, max_grad_norm, learning_rate, beta1, beta2, adam_eps.
__global__ __launch_bounds__(1024) void ppo_apply_set_kernel(SetParams prm, int D, const float* hyper, float* grad_all,
                                                             float* m_all, float* v_all, int32_t* step_all, float* stats_all) {
    __shared__ float red[16];
    __shared__ float coef_s;
    const int tid = threadIdx.x;
    const size_t k_m = blockIdx.x;
    const int total = 2 * net_size(D) + 1;
    float* grad = grad_all + k_m * (size_t)total;
    float* m = m_all + k_m * (size_t)total;
    float* v = v_all + k_m * (size_t)total;
    int32_t* step = step_all + k_m;
    float* stats = stats_all + k_m * 8;
    const float ACAS2D_C4* hy = (const float ACAS2D_C4*)(hyper + k_m * 8);
    const float ent_coef = hy[2], max_norm = hy[3], lr = hy[4], beta1 = hy[5], beta2 = hy[6], eps = hy[7];
    if (tid == 0) grad[total - 1] -= ent_coef;               // d(ent_coef * -entropy) / d log_std (the last entry)
    __syncthreads();
    float sq = 0.0f;
    for (int i = tid; i < total; i += 1024) sq = fmaf(grad[i], grad[i], sq);
    sq = wave_sum(sq);
    if ((tid & 63) == 0) red[tid >> 6] = sq;
    __syncthreads();
    if (tid == 0) {
        float tot = 0.0f;
        for (int i = 0; i < 16; ++i) tot += red[i];
        const float norm = sqrtf(tot);
        coef_s = fminf(1.0f, max_norm / (norm + 1e-6f));      // torch.nn.utils.clip_grad_norm_
        stats[2] = norm;
        stats[4] = stats[0]; stats[5] = stats[1];             // the minibatch's policy / value loss, for the log
        stats[0] = 0.0f; stats[1] = 0.0f;
    }
    __syncthreads();
    const float coef = coef_s;
    const int tstep = step[0] + 1;
    const float bc1 = 1.0f - powf(beta1, (float)tstep), bc2 = 1.0f - powf(beta2, (float)tstep);
    int offset = 0;
    for (int k = 0; k < 13; ++k) {
        const int count = seg_count(D, k);
        float* p = prm.p[k] + k_m * (size_t)count;
        for (int i = tid; i < count; i += 1024) {
            const int gi = offset + i;
            const float gr = grad[gi] * coef;
            const float mm = fmaf(beta1, m[gi], (1.0f - beta1) * gr);
            const float vv = fmaf(beta2, v[gi], (1.0f - beta2) * gr * gr);
            m[gi] = mm; v[gi] = vv;
            p[i] -= (lr / bc1) * mm / (sqrtf(vv) / sqrtf(bc2) + eps);          // torch.optim.Adam
            grad[gi] = 0.0f;
        }
        offset += count;
    }
    __syncthreads();
    if (tid == 0) step[0] = tstep;
}

SetParams set_params(const Acas2dPpoUpdateSet& u) {
    return SetParams{{(float*)u.actor_w1, (float*)u.actor_b1, (float*)u.actor_w2, (float*)u.actor_b2, (float*)u.actor_w3,
                      (float*)u.actor_b3, (float*)u.critic_w1, (float*)u.critic_b1, (float*)u.critic_w2, (float*)u.critic_b2,
                      (float*)u.critic_w3, (float*)u.critic_b3, (float*)u.log_std}};
}

// Dynamic LDS of ppo_grad_set_kernel<D>: as ppo_grad_kernel<D>'s (69.6 - 74.8 KB for D = 8 ... 29), more than the 64 KB a
// HIP launch gets without asking.  The attribute that raises the kernel's limit belongs to a (kernel, device) pair, so
// what was asked for is remembered PER DEVICE: a process that updates on a second device asks again there.
constexpr int kMaxDevices = 64;

template <int D>
int launch_grad_set(const Acas2dPpoUpdateSet& u, hipStream_t stream) {
    const size_t lds_bytes = (size_t)(4 * 64 * kRow + 64 * (D + 1) + 64) * sizeof(float);
    static std::atomic<int> lds_limit[kMaxDevices];          // per instantiation and device; 0: not asked yet
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { set_error("acas2d_ppo_update_set: cannot query the current device"); return ACAS2D_EHIP; }
    int limit = (dev >= 0 && dev < kMaxDevices) ? lds_limit[dev].load(std::memory_order_acquire) : 0;
    if (limit == 0) {
        int optin = 0;
        if (hipDeviceGetAttribute(&optin, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) {
            set_error("acas2d_ppo_update_set: cannot query the device's LDS size"); return ACAS2D_EHIP; }
        if ((size_t)optin >= lds_bytes)
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ppo_grad_set_kernel<D>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        (void)hipGetLastError();
        limit = optin > 0 ? optin : -1;
        if (dev >= 0 && dev < kMaxDevices) lds_limit[dev].store(limit, std::memory_order_release);
    }
    if (limit < 0 || (size_t)limit < lds_bytes) {
        set_error("acas2d_ppo_update_set: the gradient kernel needs %zu bytes of LDS per workgroup, this device offers %d "
                  "(built for gfx950's 160 KB)", lds_bytes, limit < 0 ? 0 : limit);
        return ACAS2D_EINVAL;
    }
    hipLaunchKernelGGL((ppo_grad_set_kernel<D>), dim3((unsigned)((u.n_rows + 63) / 64), 2, (unsigned)u.n_members), dim3(64),
                       lds_bytes, stream, set_params(u), (const float*)u.obs, (const float*)u.act, (const float*)u.old_logp,
                       (const float*)u.adv, (const float*)u.ret, (const int64_t*)u.idx, u.n_rows, (const float*)u.hyper,
                       (float*)u.grad, (float*)u.stats);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) { set_error("acas2d_ppo_update_set gradient launch: %s", hipGetErrorString(err)); return ACAS2D_EHIP; }
    return ACAS2D_OK;
}

}  // namespace
}  // namespace acas2d

using namespace acas2d;
using namespace acas2d::ppo;

extern "C" int acas2d_ppo_update_set_f32(const Acas2dPpoUpdateSet* u, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!u) { set_error("acas2d_ppo_update_set: NULL argument"); return ACAS2D_EINVAL; }
    const void* need[] = {u->actor_w1, u->actor_b1, u->actor_w2, u->actor_b2, u->actor_w3, u->actor_b3, u->critic_w1, u->critic_b1,
                          u->critic_w2, u->critic_b2, u->critic_w3, u->critic_b3, u->log_std, u->obs, u->act, u->old_logp, u->adv,
                          u->ret, u->idx, u->hyper, u->grad, u->adam_m, u->adam_v, u->adam_step, u->stats};
    for (const void* p : need) if (!p) { set_error("acas2d_ppo_update_set: every pointer is required"); return ACAS2D_EINVAL; }
    if (u->n_members < 1 || u->n_members > 65535) {
        set_error("acas2d_ppo_update_set: n_members = %d (1 to 65535 members, one grid plane each)", u->n_members); return ACAS2D_EINVAL; }
    if (u->n_rows < 2) {
        set_error("acas2d_ppo_update_set: n_rows = %d (the advantage normalisation needs 2; every member takes the same "
                  "number of rows)", u->n_rows);
        return ACAS2D_EINVAL;
    }
    const int D = u->obs_dim;
    int rc;
    switch (D) {
        case 8: rc = launch_grad_set<8>(*u, stream); break;
        case 11: rc = launch_grad_set<11>(*u, stream); break;
        case 14: rc = launch_grad_set<14>(*u, stream); break;
        case 17: rc = launch_grad_set<17>(*u, stream); break;
        case 29: rc = launch_grad_set<29>(*u, stream); break;
        default:
            set_error("acas2d_ppo_update_set: obs_dim = %d (float32, built for n_traffic in {1, 2, 3, 4, 8}: obs_dim 8, 11, 14, "
                      "17, 29; the wide update of n_traffic 16 / 32 / 64 takes one learner per call)", D);
            return ACAS2D_EINVAL;
    }
    if (rc != ACAS2D_OK) return rc;                      // (a failed gradient launch must not read as a zero gradient)
    if (u->apply == 0) return ACAS2D_OK;                 // tests: the raw gradients stay in `grad`, nothing is applied
    hipLaunchKernelGGL(ppo_apply_set_kernel, dim3((unsigned)u->n_members), dim3(1024), 0, stream, set_params(*u), D,
                       (const float*)u->hyper, (float*)u->grad, (float*)u->adam_m, (float*)u->adam_v, u->adam_step,
                       (float*)u->stats);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) { set_error("acas2d_ppo_update_set launch: %s", hipGetErrorString(err)); return ACAS2D_EHIP; }
    return ACAS2D_OK;
}
