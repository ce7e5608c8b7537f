// acas2d_ppo_wide_set.hip -- acas2d_ppo_update_set_f32 at obs_dim 53, 101, 197 (16, 32, 64 traffic aircraft): one PPO
// minibatch update of K independent actor-critics as TWO launches, whatever K is.  acas2d_ppo_update_wide_f32 gives one
// learner ceil(n_rows / 64) x 2 workgroups -- 128 at a minibatch of 4 096, on 256 CUs -- and one workgroup for Adam;
// here the K learners lie side by side.
//
//   ppo_grad_wide_set_kernel   grid (ceil(n_rows / 64), 2, K), 256 threads: blockIdx.z is the member.  The prologue is a
//                              SetMember (acas2d_ppo_wide.hpp): the member's slices of the [K][...] parameter stacks, its
//                              minibatch idx[k][.], its gradient block grad[k], its stats[k], and its clip_range and
//                              vf_coef from hyper[k] by scalar load; the rest is grad_wide<D> (the same header), the body
//                              ppo_grad_wide_kernel<D> runs.
//   ppo_apply_set_kernel       acas2d_ppo_set.hip's, through launch_ppo_apply_set: it takes D at run time.
//
// grad_wide<D> asks for each of the member's pointers where it uses it (acas2d_ppo_wide.hpp says why): the SetMember
// hands it the stacks and the member number, not six sums.
#include "acas2d_ppo_wide.hpp"

namespace acas2d {
using namespace ppo;
using namespace ppo::wide;

namespace {

template <int D>
__global__ __launch_bounds__(kThreads) void ppo_grad_wide_set_kernel(SetNets nets, const float* obs, const float* act,
                                                                     const float* old_logp, const float* adv,
                                                                     const float* ret, const int64_t* idx_all, int B,
                                                                     const float* hyper, float* grad_all, float* stats_all) {
    grad_wide<D>(SetMember{nets, idx_all, hyper, grad_all, stats_all, B, 2 * net_size(D) + 1}, obs, act, old_logp, adv, ret, B);
}

// The dynamic LDS is 79 - 115 KB: ensure_dynamic_lds raises the kernel's limit on the current device and checks the size.
template <int D>
int launch_grad_wide_set(const Acas2dPpoUpdateSet& u, hipStream_t stream) {
    constexpr size_t bytes = lds_bytes(D);
    const int rc = ensure_dynamic_lds<&ppo_grad_wide_set_kernel<D>>(bytes, "acas2d_ppo_update_wide_set");
    if (rc != ACAS2D_OK) return rc;
    hipLaunchKernelGGL((ppo_grad_wide_set_kernel<D>), dim3((unsigned)((u.n_rows + 63) / 64), 2, (unsigned)u.n_members),
                       dim3(kThreads), bytes, stream, set_nets_of(u), (const float*)u.obs, (const float*)u.act,
                       (const float*)u.old_logp, (const float*)u.adv, (const float*)u.ret, (const int64_t*)u.idx, u.n_rows,
                       (const float*)u.hyper, (float*)u.grad, (float*)u.stats);
    return launched("acas2d_ppo_update_wide_set gradient launch");
}

}  // namespace
}  // namespace acas2d

using namespace acas2d;
using namespace acas2d::ppo;

extern "C" int acas2d_ppo_update_wide_set_f32(const Acas2dPpoUpdateSet* u, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = check_set(u, "acas2d_ppo_update_wide_set");
    if (rc != ACAS2D_OK) return rc;
    switch (u->obs_dim) {
        case 53: rc = launch_grad_wide_set<53>(*u, stream); break;
        case 101: rc = launch_grad_wide_set<101>(*u, stream); break;
        case 197: rc = launch_grad_wide_set<197>(*u, stream); break;
        case 8: case 11: case 14: case 17: case 29:
            set_error("acas2d_ppo_update_wide_set: obs_dim = %d is a narrow width (n_traffic in {1, 2, 3, 4, 8}): use "
                      "acas2d_ppo_update_set_f32; this entry is built for n_traffic in {16, 32, 64}: obs_dim 53, 101, 197", u->obs_dim);
            return ACAS2D_EINVAL;
        default:
            set_error("acas2d_ppo_update_wide_set: obs_dim = %d (float32, built for n_traffic in {16, 32, 64}: obs_dim 53, 101, "
                      "197; acas2d_ppo_update_set_f32 serves obs_dim 8, 11, 14, 17, 29)", u->obs_dim);
            return ACAS2D_EINVAL;
    }
    if (rc != ACAS2D_OK) return rc;                      // (a failed gradient launch must not read as a zero gradient)
    if (u->apply == 0) return ACAS2D_OK;                 // tests: the raw gradients stay in `grad`, nothing is applied
    return launch_ppo_apply_set(*u, stream);
}
