// acas2d_ppo_wide.hip -- the PPO minibatch update of acas2d_ppo.hip at obs_dim 53, 101, 197 (16, 32, 64 traffic
// aircraft): acas2d_ppo_update_wide_f32, same struct, same flat gradient / moment layout, same `stats`, same probe mode.
//
// ppo_grad_kernel<D> keeps x[D] and a D-wide gradient row per lane in registers; at these widths that does not fit.
// ppo_grad_wide_kernel<D> is a prologue in front of grad_wide<D> (acas2d_ppo_wide.hpp), the body it shares with the
// K-learner kernels of acas2d_ppo_wide_set.hip and acas2d_ppo_guard.hip.  That body keeps the scheme -- one lane per sample, weights as scalar
// operands, the per-sample vectors in LDS with row stride 65 -- and tiles what is D-sized, with FOUR waves per 64 samples
// and network:
//
//   forward / backward to the pre-activations   every wave holds the same 64 samples (lane = sample) and takes 16 of the
//                      64 hidden units of each layer: layer 1 accumulates its 16 pre-activations in registers over
//                      chunks of 4 observation entries read back from LDS (k ascending: the fmaf chain of the narrow
//                      kernel), layer 2 and dh1 = W2^T dz2 likewise; the waves meet in LDS between the layers.
//   weight gradients   lane = COLUMN of the weight matrix, wave = 16 of its rows: dW1[i][c] = sum_q dz1[q][i] x[q][c]
//                      in column blocks of 64 (4 at D = 197), dW2 in one; dz comes as an LDS broadcast, x[q][c] / h1[q][c]
//                      as conflict-free rows, q ascending.  The 64 lanes of one atomic instruction then hit 64
//                      CONSECUTIVE floats of `grad` (the narrow kernel's lanes are D floats apart).
//   the advantage statistics of the whole minibatch are taken by the actor workgroup's 256 threads together.
// d loss / d output is loss_grad of acas2d_ppo.hpp, the narrow kernels' own.  ppo_apply_kernel (norm, clip_grad_norm_,
// Adam) does not depend on the width: launch_ppo_apply of acas2d_ppo.hip.
#include "acas2d_ppo_wide.hpp"

namespace acas2d {
using namespace ppo;
using namespace ppo::wide;

namespace {

// one learner: the kernel's own arguments, no offsets
struct OneLearner {
    const Nets& nets;
    const float* log_std_p;
    const int64_t* idx_p;
    float clip, vf;
    float *grad_p, *stats_p;
    __device__ __forceinline__ NetW net() const { return nets.n[blockIdx.y]; }
    __device__ __forceinline__ static constexpr int at(int) { return 0; }
    __device__ __forceinline__ const int64_t* idx() const { return idx_p; }
    __device__ __forceinline__ const float* log_std() const { return log_std_p; }
    __device__ __forceinline__ float clip_range() const { return clip; }
    __device__ __forceinline__ float vf_coef() const { return vf; }
    __device__ __forceinline__ float* grad() const { return grad_p; }
    __device__ __forceinline__ float* stats() const { return stats_p; }
};

template <int D>
__global__ __launch_bounds__(kThreads) void ppo_grad_wide_kernel(Nets nets, const float* log_std_p,
                                                                 const float* obs, const float* act, const float* old_logp,
                                                                 const float* adv, const float* ret, const int64_t* idx,
                                                                 int B, float clip_range, float vf_coef, float* grad,
                                                                 float* stats) {
    grad_wide<D>(OneLearner{nets, log_std_p, idx, clip_range, vf_coef, grad, stats}, obs, act, old_logp, adv, ret, B);
}

// The dynamic LDS is 79 - 115 KB: ensure_dynamic_lds raises the kernel's limit on the current device and checks the size.
template <int D>
int launch_grad_wide(const Acas2dPpoUpdate& u, hipStream_t stream) {
    constexpr size_t bytes = lds_bytes(D);
    const int rc = ensure_dynamic_lds<&ppo_grad_wide_kernel<D>>(bytes, "acas2d_ppo_update_wide");
    if (rc != ACAS2D_OK) return rc;
    const Nets nets = nets_of(u);
    hipLaunchKernelGGL((ppo_grad_wide_kernel<D>), dim3((unsigned)((u.n_rows + 63) / 64), 2), dim3(kThreads), bytes, stream, nets,
                       (const float*)u.log_std, (const float*)u.obs, (const float*)u.act, (const float*)u.old_logp,
                       (const float*)u.adv, (const float*)u.ret, (const int64_t*)u.idx, u.n_rows, u.clip_range, u.vf_coef,
                       (float*)u.grad, (float*)u.stats);
    return launched("acas2d_ppo_update_wide gradient launch");
}

}  // namespace
}  // namespace acas2d

using namespace acas2d;
using namespace acas2d::ppo;
using namespace acas2d::ppo::wide;

extern "C" int acas2d_ppo_wide_lds_bytes(int32_t obs_dim) {
    switch (obs_dim) {
        case 53: return (int)lds_bytes(53);
        case 101: return (int)lds_bytes(101);
        case 197: return (int)lds_bytes(197);
        default: set_error("acas2d_ppo_wide_lds_bytes: obs_dim = %d (built for n_traffic in {16, 32, 64})", obs_dim); return ACAS2D_EINVAL;
    }
}

extern "C" int acas2d_ppo_update_wide_f32(const Acas2dPpoUpdate* u, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = check_update(u, "acas2d_ppo_update_wide", u, "");
    if (rc != ACAS2D_OK) return rc;
    switch (u->obs_dim) {
        case 53: rc = launch_grad_wide<53>(*u, stream); break;
        case 101: rc = launch_grad_wide<101>(*u, stream); break;
        case 197: rc = launch_grad_wide<197>(*u, stream); break;
        default: set_error("acas2d_ppo_update_wide: obs_dim = %d (built for n_traffic in {16, 32, 64}: obs_dim 53, 101, 197)", u->obs_dim);
                 return ACAS2D_EINVAL;
    }
    if (rc != ACAS2D_OK) return rc;                      // (a failed gradient launch must not read as a zero gradient)
    if (u->max_grad_norm < 0.0f) return ACAS2D_OK;      // tests: the raw gradient stays in `grad`, nothing is applied
    return launch_ppo_apply(*u, stream);
}
