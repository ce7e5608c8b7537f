// acas2d_ppo_set.hip -- one PPO minibatch update of K independent SB3 MlpPolicy actor-critics ("members" of a population:
// the seeds of a sweep, or its hyper-parameter sets) as TWO launches, whatever K is.  acas2d_ppo.hip gives one learner
// 128 single-wave workgroups at a minibatch of 4 096 and one workgroup for Adam on a device with 256 CUs; here the K
// learners lie side by side in the same two launches.
//
//   ppo_grad_set_kernel   grid (ceil(n_rows / 64), 2, K): blockIdx.z is the member.  It is grad_narrow_member<D>
//                         (acas2d_ppo.hpp): the prologue that takes the member's slices of the [K][...] parameter stacks,
//                         its minibatch idx[k][.], its gradient block grad[k], and its clip_range and vf_coef from
//                         hyper[k] by scalar load, in front of grad_narrow<D>, the body ppo_grad_kernel<D> runs.  The
//                         rollout buffer is ONE flat buffer shared by all members; idx holds its global row numbers.
//   ppo_apply_set_kernel  grid (K), 1 024 threads: apply_body (acas2d_ppo.hpp), the body ppo_apply_kernel runs, on member
//                         k's slices with hyper[k] and adam_step[k].
//
// With one wave per network (n_rows <= 64) every gradient entry receives one atomic add, and the set and the solo update
// agree in every bit.  Out of scope (rejected): float64, members with different n_rows, and the wide widths (obs_dim 53 /
// 101 / 197): those are acas2d_ppo_update_wide_set_f32 (acas2d_ppo_wide_set.hip), which shares ppo_apply_set_kernel.
#include "acas2d_ppo.hpp"

namespace acas2d {
using namespace ppo;

namespace {

template <int D>
__global__ __launch_bounds__(64) void ppo_grad_set_kernel(ParamPtrs prm, const float* obs, const float* act,
                                                          const float* old_logp, const float* adv, const float* ret,
                                                          const int64_t* idx_all, int B, const float* hyper, float* grad_all,
                                                          float* stats_all) {
    extern __shared__ float lds[];
    grad_narrow_member<D>(prm, obs, act, old_logp, adv, ret, idx_all, B, hyper, grad_all, stats_all, lds);
}

// hyper[k]: clip_range, vf_coef, ent_coef, max_grad_norm, learning_rate, beta1, beta2, adam_eps
__global__ __launch_bounds__(1024) void ppo_apply_set_kernel(ParamPtrs prm, int D, const float* hyper, float* grad_all,
                                                             float* m_all, float* v_all, int32_t* step_all, float* stats_all) {
    const size_t k_m = blockIdx.x;
    const size_t total = 2 * net_size(D) + 1;
    const float ACAS2D_C4* hy = (const float ACAS2D_C4*)(hyper + k_m * 8);
    apply_body(prm, k_m, D, grad_all + k_m * total, m_all + k_m * total, v_all + k_m * total, step_all + k_m,
               stats_all + k_m * 8, hy[2], hy[3], hy[4], hy[5], hy[6], hy[7]);
}

template <int D>
int launch_grad_set(const Acas2dPpoUpdateSet& u, hipStream_t stream) {
    const int rc = ensure_dynamic_lds<&ppo_grad_set_kernel<D>>(narrow_lds_bytes(D), "acas2d_ppo_update_set");
    if (rc != ACAS2D_OK) return rc;
    hipLaunchKernelGGL((ppo_grad_set_kernel<D>), dim3((unsigned)((u.n_rows + 63) / 64), 2, (unsigned)u.n_members), dim3(64),
                       narrow_lds_bytes(D), stream, param_ptrs(u), (const float*)u.obs, (const float*)u.act, (const float*)u.old_logp,
                       (const float*)u.adv, (const float*)u.ret, (const int64_t*)u.idx, u.n_rows, (const float*)u.hyper,
                       (float*)u.grad, (float*)u.stats);
    return launched("acas2d_ppo_update_set gradient launch");
}

}  // namespace

// ppo_apply_set_kernel on the K members of `u`; the wide set update (acas2d_ppo_wide_set.hip) ends with it too
int launch_ppo_apply_set(const Acas2dPpoUpdateSet& u, hipStream_t stream) {
    hipLaunchKernelGGL(ppo_apply_set_kernel, dim3((unsigned)u.n_members), dim3(1024), 0, stream, param_ptrs(u), u.obs_dim,
                       (const float*)u.hyper, (float*)u.grad, (float*)u.adam_m, (float*)u.adam_v, u.adam_step,
                       (float*)u.stats);
    return launched("acas2d_ppo_update_set launch");
}

}  // namespace acas2d

using namespace acas2d;
using namespace acas2d::ppo;

extern "C" int acas2d_ppo_update_set_f32(const Acas2dPpoUpdateSet* u, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = check_set(u, "acas2d_ppo_update_set");
    if (rc != ACAS2D_OK) return rc;
    const int D = u->obs_dim;
    switch (D) {
        case 8: rc = launch_grad_set<8>(*u, stream); break;
        case 11: rc = launch_grad_set<11>(*u, stream); break;
        case 14: rc = launch_grad_set<14>(*u, stream); break;
        case 17: rc = launch_grad_set<17>(*u, stream); break;
        case 29: rc = launch_grad_set<29>(*u, stream); break;
        default:
            set_error("acas2d_ppo_update_set: obs_dim = %d (float32, built for n_traffic in {1, 2, 3, 4, 8}: obs_dim 8, 11, 14, "
                      "17, 29; n_traffic 16 / 32 / 64 is acas2d_ppo_update_wide_set_f32)", D);
            return ACAS2D_EINVAL;
    }
    if (rc != ACAS2D_OK) return rc;                      // (a failed gradient launch must not read as a zero gradient)
    if (u->apply == 0) return ACAS2D_OK;                 // tests: the raw gradients stay in `grad`, nothing is applied
    return launch_ppo_apply_set(*u, stream);
}
