// acas2d_ppo.hip -- one PPO minibatch update of the SB3 MlpPolicy actor-critic as TWO hand-written launches.
//
// What it replaces: the body of the minibatch loop of SB3 1.1.0's PPO.train() as training_main.py:44-52 runs it
// (`PPO('MlpPolicy', env).learn()`): forward of the separate 2 x 64 tanh actor / critic on the minibatch, the clipped
// surrogate + value + entropy loss, backward, clip_grad_norm_, Adam -- ~60 library kernels per minibatch when it runs
// as torch ops (gym-acas2d_amd/ppo.py, ppo_loss()), and what bounds a PPO iteration on the device-resident env.
//
//   ppo_grad_kernel    grid (ceil(n_rows / 64), 2): one wave per 64 samples and network (blockIdx.y: 0 actor, 1 critic).
//                      The prologue picks that network's weights; the rest is grad_narrow<D> (acas2d_ppo.hpp).
//   ppo_apply_kernel   one workgroup: apply_body (acas2d_ppo.hpp) on the 13 parameter tensors, with the hyper-parameters
//                      as launch constants.  It does not depend on the width: the wide update launches it too.
#include "acas2d_ppo.hpp"

namespace acas2d {
using namespace ppo;

namespace {

template <int D>
__global__ __launch_bounds__(64) void ppo_grad_kernel(NetW actor, NetW critic, const float* log_std_p, const float* obs,
                                                      const float* act, const float* old_logp, const float* adv,
                                                      const float* ret, const int64_t* idx, int B, float clip_range,
                                                      float vf_coef, float* grad, float* stats) {
    extern __shared__ float lds[];
    const NetW net = blockIdx.y == 0 ? actor : critic;
    grad_narrow<D>((const float ACAS2D_C4*)net.w1, (const float ACAS2D_C4*)net.b1, (const float ACAS2D_C4*)net.w2,
                   (const float ACAS2D_C4*)net.b2, (const float ACAS2D_C4*)net.w3, (const float ACAS2D_C4*)net.b3, log_std_p,
                   obs, act, old_logp, adv, ret, idx, B, clip_range, vf_coef, grad, stats, lds);
}

// the hyper-parameters are launch constants; one learner, so member 0 of "stacks" of one
__global__ __launch_bounds__(1024) void ppo_apply_kernel(ParamPtrs prm, int D, float* grad, float* m, float* v,
                                                         int32_t* step, float ent_coef, float max_norm, float lr,
                                                         float beta1, float beta2, float eps, float* stats) {
    apply_body(prm, 0, D, grad, m, v, step, stats, ent_coef, max_norm, lr, beta1, beta2, eps);
}

template <int D>
int launch_grad(const Acas2dPpoUpdate& u, hipStream_t stream) {
    const int rc = ensure_dynamic_lds<&ppo_grad_kernel<D>>(narrow_lds_bytes(D), "acas2d_ppo_update");
    if (rc != ACAS2D_OK) return rc;
    const Nets nets = nets_of(u);
    hipLaunchKernelGGL((ppo_grad_kernel<D>), dim3((unsigned)((u.n_rows + 63) / 64), 2), dim3(64), narrow_lds_bytes(D), stream,
                       nets.n[0], nets.n[1], (const float*)u.log_std, (const float*)u.obs, (const float*)u.act,
                       (const float*)u.old_logp, (const float*)u.adv, (const float*)u.ret, (const int64_t*)u.idx, u.n_rows,
                       u.clip_range, u.vf_coef, (float*)u.grad, (float*)u.stats);
    return launched("acas2d_ppo_update gradient launch");
}

}  // namespace

int launch_ppo_apply(const Acas2dPpoUpdate& u, hipStream_t stream) {
    hipLaunchKernelGGL(ppo_apply_kernel, dim3(1), dim3(1024), 0, stream, param_ptrs(u), u.obs_dim, (float*)u.grad,
                       (float*)u.adam_m, (float*)u.adam_v, (int32_t*)u.adam_step, u.ent_coef, u.max_grad_norm, u.learning_rate,
                       u.beta1, u.beta2, u.adam_eps, (float*)u.stats);
    return launched("acas2d_ppo_update launch");
}

}  // namespace acas2d

using namespace acas2d;
using namespace acas2d::ppo;

extern "C" int acas2d_ppo_workspace_floats(int32_t obs_dim) { return 2 * net_size(obs_dim) + 1; }

extern "C" int acas2d_ppo_update_f32(const Acas2dPpoUpdate* u, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = check_update(u, "acas2d_ppo_update", u, "");
    if (rc != ACAS2D_OK) return rc;
    const int D = u->obs_dim;
    switch (D) {
        case 8: rc = launch_grad<8>(*u, stream); break;
        case 11: rc = launch_grad<11>(*u, stream); break;
        case 14: rc = launch_grad<14>(*u, stream); break;
        case 17: rc = launch_grad<17>(*u, stream); break;
        case 29: rc = launch_grad<29>(*u, stream); break;
        default: set_error("acas2d_ppo_update: obs_dim = %d (built for n_traffic in {1, 2, 3, 4, 8})", D); return ACAS2D_EINVAL;
    }
    if (rc != ACAS2D_OK) return rc;                      // (a failed gradient launch must not read as a zero gradient)
    if (u->max_grad_norm < 0.0f) return ACAS2D_OK;      // tests: the raw gradient stays in `grad`, nothing is applied
    return launch_ppo_apply(*u, stream);
}
