// acas2d_ppo_sb3.hip -- the rest of SB3 1.1.0's PPO.__init__ for the set updates: clip_range_vf (the value-function
// clipping) and per-update factors on learning_rate, clip_range and clip_range_vf (what a schedule of progress_remaining
// evaluates to), inside the two launches of acas2d_ppo_update_guarded_set_f32 at all eight widths:
// acas2d_ppo_update_sb3_set_f32.  The factors MULTIPLY what hyper[k] holds when the kernels run, so they compose with
// acas2d_population_exploit_f32 rewriting those rows on the device.
//
//   ppo_grad_sb3_set_kernel<D>        grad_narrow_member<D, true, true> (acas2d_ppo.hpp): the guarded kernel's prologue
//   ppo_grad_wide_sb3_set_kernel<D>   a SetMember with the three option pointers in front of grad_wide<D, ., true, true>
//                         stopped[k] != 0: the workgroup returns at its top, as in the guarded kernels.  An actor workgroup
//                         uses clip_range = hyper[k][0] * scale[k][1] (ONE float32 product) for the surrogate and for the
//                         guard's clipped count.  A critic workgroup forms c = clip_range_vf[k] * scale[k][2]; c > 0: SB3's
//                         clipped value loss against old_val (loss_grad<., true>); otherwise (0, negative, NaN) the plain
//                         MSE branch, and old_val is not read for that member.
//   ppo_apply_sb3_set_kernel          ppo_apply_guarded_set_kernel's statistics and stop decision, then the unchanged
//                         apply_body with lr = hyper[k][4] * scale[k][0].
//
// scale rows of ones and clip_range_vf of zeros give the guarded entry's result: x * 1.0f is exact and the critic branch
// is the plain one, so where n_rows <= 64 (one atomic add per gradient entry) the two agree bit for bit.
#include "acas2d_ppo_wide.hpp"

namespace acas2d {
using namespace ppo;
using namespace ppo::wide;

namespace {

// as in acas2d_ppo_guard.hip: the flag by scalar load, the member number through an empty asm so that this address is
// not kept as the common subexpression of the member offsets formed after layer 1
__device__ __forceinline__ bool member_stopped(const int32_t* stopped, uint32_t m) {
    asm volatile("" : "+s"(m));
    return ((const int32_t ACAS2D_C4*)stopped)[m] != 0;
}

template <int D>
__global__ __launch_bounds__(64) void ppo_grad_sb3_set_kernel(ParamPtrs prm, const float* obs, const float* act,
                                                              const float* old_logp, const float* adv, const float* ret,
                                                              const int64_t* idx_all, int B, const float* hyper,
                                                              float* grad_all, float* stats_all, const int32_t* stopped,
                                                              float* diag_all, const float* old_val,
                                                              const float* clip_range_vf, const float* scale) {
    extern __shared__ float lds[];
    if (member_stopped(stopped, blockIdx.z)) return;
    grad_narrow_member<D, true, true>(prm, obs, act, old_logp, adv, ret, idx_all, B, hyper, grad_all, stats_all, lds, diag_all,
                                      old_val, clip_range_vf, scale);
}

// `stopped` stands where the guarded kernel has it; the three option pointers are read after layer 3, with hyper.
template <int D>
__global__ __launch_bounds__(kThreads) void ppo_grad_wide_sb3_set_kernel(SetNets nets, const float* obs, const float* act,
                                                                         const float* old_logp, const float* adv,
                                                                         const float* ret, const int64_t* idx_all,
                                                                         const int32_t* stopped, int B, const float* hyper,
                                                                         float* grad_all, float* stats_all, float* diag_all,
                                                                         const float* old_val, const float* clip_range_vf,
                                                                         const float* scale) {
    if (member_stopped(stopped, blockIdx.z)) return;
    grad_wide<D, OptsMember, true, true>(OptsMember(SetMember{nets, idx_all, hyper, grad_all, stats_all, B,
                                                              2 * net_size(D) + 1, diag_all, old_val, clip_range_vf, scale}),
                                         obs, act, old_logp, adv, ret, B);
}

// ppo_apply_guarded_set_kernel with the learning rate hyper[k][4] * scale[k][0] (one float32 product)
__global__ __launch_bounds__(1024) void ppo_apply_sb3_set_kernel(ParamPtrs prm, int D, const float* hyper, float* grad_all,
                                                                 float* m_all, float* v_all, int32_t* step_all,
                                                                 float* stats_all, int B, const float* target_kl,
                                                                 int32_t* stopped, float* diag_all, const float* scale) {
    __shared__ int stop_s;
    const size_t k_m = blockIdx.x;
    if (member_stopped(stopped, blockIdx.x)) return;
    const int tid = threadIdx.x;
    const int total = 2 * net_size(D) + 1;
    float* grad = grad_all + k_m * total;
    float* stats = stats_all + k_m * 8;
    float* diag = diag_all + k_m * 8;
    if (tid == 0) {
        const float kl = diag[0] / (float)B, cf = diag[1] / (float)B;
        diag[2] = kl; diag[3] = cf;
        diag[4] += kl; diag[5] += cf; diag[6] += 1.0f;
        diag[0] = 0.0f; diag[1] = 0.0f;
        const float limit = target_kl[k_m];
        const bool stop = limit > 0.0f && kl > 1.5f * limit;
        if (stop) {
            stopped[k_m] = 1;
            stats[4] = stats[0]; stats[5] = stats[1];             // the stopping minibatch's losses, for the log
            stats[0] = 0.0f; stats[1] = 0.0f;
        }
        stop_s = stop ? 1 : 0;
    }
    __syncthreads();
    if (stop_s) {                                                 // (uniform over the workgroup)
        for (int i = tid; i < total; i += 1024) grad[i] = 0.0f;
        return;
    }
    const float ACAS2D_C4* hy = (const float ACAS2D_C4*)(hyper + k_m * 8);
    const float lr = hy[4] * ((const float ACAS2D_C4*)scale)[k_m * 4];
    apply_body(prm, k_m, D, grad, m_all + k_m * total, v_all + k_m * total, step_all + k_m, stats, hy[2], hy[3], lr, hy[5],
               hy[6], hy[7]);
    if (tid == 0) diag[7] += 1.0f;
}

constexpr const char* kEntry = "acas2d_ppo_update_sb3_set";

template <int D>
int launch_grad_sb3(const Acas2dPpoUpdateSet& u, const Acas2dPpoGuard& g, const Acas2dPpoOptions& o, hipStream_t stream) {
    const dim3 grid((unsigned)((u.n_rows + 63) / 64), 2, (unsigned)u.n_members);
    if constexpr (D <= 29) {
        const int rc = ensure_dynamic_lds<&ppo_grad_sb3_set_kernel<D>>(narrow_lds_bytes(D), kEntry);
        if (rc != ACAS2D_OK) return rc;
        hipLaunchKernelGGL((ppo_grad_sb3_set_kernel<D>), grid, dim3(64), narrow_lds_bytes(D), stream, param_ptrs(u),
                           (const float*)u.obs, (const float*)u.act, (const float*)u.old_logp, (const float*)u.adv,
                           (const float*)u.ret, (const int64_t*)u.idx, u.n_rows, (const float*)u.hyper, (float*)u.grad,
                           (float*)u.stats, (const int32_t*)g.stopped, (float*)g.diag, (const float*)o.old_val,
                           (const float*)o.clip_range_vf, (const float*)o.scale);
    } else {
        constexpr size_t bytes = lds_bytes(D);
        const int rc = ensure_dynamic_lds<&ppo_grad_wide_sb3_set_kernel<D>>(bytes, kEntry);
        if (rc != ACAS2D_OK) return rc;
        hipLaunchKernelGGL((ppo_grad_wide_sb3_set_kernel<D>), grid, dim3(kThreads), bytes, stream, set_nets_of(u),
                           (const float*)u.obs, (const float*)u.act, (const float*)u.old_logp, (const float*)u.adv,
                           (const float*)u.ret, (const int64_t*)u.idx, (const int32_t*)g.stopped, u.n_rows,
                           (const float*)u.hyper, (float*)u.grad, (float*)u.stats, (float*)g.diag, (const float*)o.old_val,
                           (const float*)o.clip_range_vf, (const float*)o.scale);
    }
    return launched("acas2d_ppo_update_sb3_set gradient launch");
}

}  // namespace
}  // namespace acas2d

using namespace acas2d;
using namespace acas2d::ppo;

extern "C" size_t acas2d_ppo_options_size(void) { return sizeof(Acas2dPpoOptions); }

extern "C" int acas2d_ppo_update_sb3_set_f32(const Acas2dPpoUpdateSet* u, const Acas2dPpoGuard* g, const Acas2dPpoOptions* o,
                                             void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = check_set(u, kEntry);
    if (rc != ACAS2D_OK) return rc;
    if (!g || !g->target_kl || !g->stopped || !g->diag) {
        set_error("%s: the guard and its three pointers (target_kl, stopped, diag) are required", kEntry); return ACAS2D_EINVAL; }
    if (!o) { set_error("%s: the options are required (NULL `o`)", kEntry); return ACAS2D_EINVAL; }
    const char* missing = !o->old_val ? "old_val" : !o->clip_range_vf ? "clip_range_vf" : !o->scale ? "scale" : nullptr;
    if (missing) { set_error("%s: options field %s is NULL (every pointer of the options is required)", kEntry, missing);
                   return ACAS2D_EINVAL; }
    const int D = u->obs_dim;
    const bool known = D == 8 || D == 11 || D == 14 || D == 17 || D == 29 || D == 53 || D == 101 || D == 197;
    if (!known) {
        set_error("%s: obs_dim = %d (float32, built for n_traffic in {1, 2, 3, 4, 8, 16, 32, 64}: obs_dim 8, 11, 14, 17, 29, 53, "
                  "101, 197)", kEntry, D);
        return ACAS2D_EINVAL;
    }
    if (u->apply == 0) {
        set_error("%s: apply = 0 (the probe mode applies nothing, so there is no stop to decide and no rate to scale: take the "
                  "raw gradients from acas2d_ppo_update_set_f32 or acas2d_ppo_update_wide_set_f32)", kEntry);
        return ACAS2D_EINVAL;
    }
    switch (D) {
        case 8: rc = launch_grad_sb3<8>(*u, *g, *o, stream); break;
        case 11: rc = launch_grad_sb3<11>(*u, *g, *o, stream); break;
        case 14: rc = launch_grad_sb3<14>(*u, *g, *o, stream); break;
        case 17: rc = launch_grad_sb3<17>(*u, *g, *o, stream); break;
        case 29: rc = launch_grad_sb3<29>(*u, *g, *o, stream); break;
        case 53: rc = launch_grad_sb3<53>(*u, *g, *o, stream); break;
        case 101: rc = launch_grad_sb3<101>(*u, *g, *o, stream); break;
        default: rc = launch_grad_sb3<197>(*u, *g, *o, stream); break;
    }
    if (rc != ACAS2D_OK) return rc;                      // (a failed gradient launch must not read as a zero gradient)
    hipLaunchKernelGGL(ppo_apply_sb3_set_kernel, dim3((unsigned)u->n_members), dim3(1024), 0, stream, param_ptrs(*u), D,
                       (const float*)u->hyper, (float*)u->grad, (float*)u->adam_m, (float*)u->adam_v, u->adam_step,
                       (float*)u->stats, u->n_rows, (const float*)g->target_kl, g->stopped, (float*)g->diag,
                       (const float*)o->scale);
    return launched("acas2d_ppo_update_sb3_set launch");
}
