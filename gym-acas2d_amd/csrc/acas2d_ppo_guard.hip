// acas2d_ppo_guard.hip -- SB3's target_kl early stop and its train/approx_kl, train/clip_fraction diagnostics for the set
// updates, decided on the device: acas2d_ppo_update_guarded_set_f32, the two launches of acas2d_ppo_update_set_f32 /
// acas2d_ppo_update_wide_set_f32 at all eight widths, with no launch and no read-back added.
//
//   ppo_grad_guarded_set_kernel<D>        grad_narrow_member<D, true> (acas2d_ppo.hpp): ppo_grad_set_kernel<D>'s prologue,
//                                         and the member's diag row, in front of grad_narrow<D, true>
//   ppo_grad_wide_guarded_set_kernel<D>   a SetMember with the diag rows (acas2d_ppo_wide.hpp): ppo_grad_wide_set_kernel<D>'s
//                                         prologue in front of grad_wide<D, ., true>
//                         A workgroup of a member with stopped[k] != 0 returns at its top (uniform, the flag by scalar
//                         load, before any LDS use or barrier).  Otherwise the arithmetic is the unguarded kernel's, and
//                         an actor workgroup also adds its rows' (ratio - 1) - log ratio to diag[k][0] and its count of
//                         |ratio - 1| > clip_range to diag[k][1] (loss_grad<true>: the ratio the surrogate uses).
//   ppo_apply_guarded_set_kernel          grid (K), 1 024 threads.  stopped[k] != 0: returns.  Otherwise thread 0 closes
//                         the minibatch's statistics: kl = diag[0] / B and cf = diag[1] / B go to diag[2], diag[3] (the
//                         last minibatch's) and are added to diag[4], diag[5], diag[6] += 1 (sums and count over the
//                         update: SB3's train/approx_kl and train/clip_fraction are [4] / [6] and [5] / [6]), diag[0]
//                         = diag[1] = 0.  target_kl[k] > 0 and kl > 1.5 target_kl[k]: the member STOPS -- stopped[k] =
//                         1, the minibatch's losses move to stats[4], stats[5] as apply_body moves them (SB3 logs the
//                         stopping minibatch), the gradient block is zeroed, and nothing is applied: parameters,
//                         moments, adam_step[k] and stats[2] stay.  Otherwise apply_body, then diag[7] += 1 (applied).
//
// SB3 1.1.0's PPO.train() breaks out of both loops BEFORE the optimizer step of the minibatch whose approx_kl exceeds
// 1.5 target_kl, after appending that minibatch to its lists: it counts in diag[4 .. 6] and not in diag[7].  The host keeps
// launching the remaining minibatches of the update; for a stopped member they cost two early returns each.  The caller
// zeroes `stopped` and `diag` where SB3 enters train().
#include "acas2d_ppo_wide.hpp"

namespace acas2d {
using namespace ppo;
using namespace ppo::wide;

namespace {

// stopped[m] != 0, wave-uniform and by scalar load.  The member number passes through an empty asm so that the address
// formed from it here is not the common subexpression of the member's offsets formed after layer 1 (b3, log_std): kept
// for them from the top it is the two SGPRs that layer 1 of the widest kernel does not have.
__device__ __forceinline__ bool member_stopped(const int32_t* stopped, uint32_t m) {
    asm volatile("" : "+s"(m));
    return ((const int32_t ACAS2D_C4*)stopped)[m] != 0;
}

template <int D>
__global__ __launch_bounds__(64) void ppo_grad_guarded_set_kernel(ParamPtrs prm, const float* obs, const float* act,
                                                                  const float* old_logp, const float* adv,
                                                                  const float* ret, const int64_t* idx_all, int B,
                                                                  const float* hyper, float* grad_all, float* stats_all,
                                                                  const int32_t* stopped, float* diag_all) {
    extern __shared__ float lds[];
    if (member_stopped(stopped, blockIdx.z)) return;
    grad_narrow_member<D, true>(prm, obs, act, old_logp, adv, ret, idx_all, B, hyper, grad_all, stats_all, lds, diag_all);
}

// `stopped` stands beside idx_all and B, the arguments the top of the kernel reads anyway: at the end of the list its
// load takes hyper, grad_all and stats_all with it into SGPRs that layer 1 has no room for (12 to 15 spills).
template <int D>
__global__ __launch_bounds__(kThreads) void ppo_grad_wide_guarded_set_kernel(SetNets nets, const float* obs, const float* act,
                                                                             const float* old_logp, const float* adv,
                                                                             const float* ret, const int64_t* idx_all,
                                                                             const int32_t* stopped, int B,
                                                                             const float* hyper, float* grad_all,
                                                                             float* stats_all, float* diag_all) {
    if (member_stopped(stopped, blockIdx.z)) return;
    grad_wide<D, SetMember, true>(SetMember{nets, idx_all, hyper, grad_all, stats_all, B, 2 * net_size(D) + 1, diag_all}, obs,
                                  act, old_logp, adv, ret, B);
}

// hyper[k] as ppo_apply_set_kernel reads it; B: the rows of the minibatch the gradient launch summed over
__global__ __launch_bounds__(1024) void ppo_apply_guarded_set_kernel(ParamPtrs prm, int D, const float* hyper, float* grad_all,
                                                                     float* m_all, float* v_all, int32_t* step_all,
                                                                     float* stats_all, int B, const float* target_kl,
                                                                     int32_t* stopped, float* diag_all) {
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
    apply_body(prm, k_m, D, grad, m_all + k_m * total, v_all + k_m * total, step_all + k_m, stats, hy[2], hy[3], hy[4], hy[5],
               hy[6], hy[7]);
    if (tid == 0) diag[7] += 1.0f;
}

constexpr const char* kEntry = "acas2d_ppo_update_guarded_set";

template <int D>
int launch_grad_guarded(const Acas2dPpoUpdateSet& u, const Acas2dPpoGuard& g, hipStream_t stream) {
    const dim3 grid((unsigned)((u.n_rows + 63) / 64), 2, (unsigned)u.n_members);
    if constexpr (D <= 29) {
        const int rc = ensure_dynamic_lds<&ppo_grad_guarded_set_kernel<D>>(narrow_lds_bytes(D), kEntry);
        if (rc != ACAS2D_OK) return rc;
        hipLaunchKernelGGL((ppo_grad_guarded_set_kernel<D>), grid, dim3(64), narrow_lds_bytes(D), stream, param_ptrs(u),
                           (const float*)u.obs, (const float*)u.act, (const float*)u.old_logp, (const float*)u.adv,
                           (const float*)u.ret, (const int64_t*)u.idx, u.n_rows, (const float*)u.hyper, (float*)u.grad,
                           (float*)u.stats, (const int32_t*)g.stopped, (float*)g.diag);
    } else {
        constexpr size_t bytes = lds_bytes(D);
        const int rc = ensure_dynamic_lds<&ppo_grad_wide_guarded_set_kernel<D>>(bytes, kEntry);
        if (rc != ACAS2D_OK) return rc;
        hipLaunchKernelGGL((ppo_grad_wide_guarded_set_kernel<D>), grid, dim3(kThreads), bytes, stream, set_nets_of(u),
                           (const float*)u.obs, (const float*)u.act, (const float*)u.old_logp, (const float*)u.adv,
                           (const float*)u.ret, (const int64_t*)u.idx, (const int32_t*)g.stopped, u.n_rows,
                           (const float*)u.hyper, (float*)u.grad, (float*)u.stats, (float*)g.diag);
    }
    return launched("acas2d_ppo_update_guarded_set gradient launch");
}

}  // namespace
}  // namespace acas2d

using namespace acas2d;
using namespace acas2d::ppo;

extern "C" size_t acas2d_ppo_guard_size(void) { return sizeof(Acas2dPpoGuard); }

extern "C" int acas2d_ppo_update_guarded_set_f32(const Acas2dPpoUpdateSet* u, const Acas2dPpoGuard* g, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = check_set(u, kEntry);
    if (rc != ACAS2D_OK) return rc;
    if (!g || !g->target_kl || !g->stopped || !g->diag) {
        set_error("%s: the guard and its three pointers (target_kl, stopped, diag) are required", kEntry); return ACAS2D_EINVAL; }
    const int D = u->obs_dim;
    const bool known = D == 8 || D == 11 || D == 14 || D == 17 || D == 29 || D == 53 || D == 101 || D == 197;
    if (!known) {
        set_error("%s: obs_dim = %d (float32, built for n_traffic in {1, 2, 3, 4, 8, 16, 32, 64}: obs_dim 8, 11, 14, 17, 29, 53, "
                  "101, 197)", kEntry, D);
        return ACAS2D_EINVAL;
    }
    if (u->apply == 0) {
        set_error("%s: apply = 0 (the probe mode applies nothing, so there is no stop to decide: take the raw gradients from "
                  "acas2d_ppo_update_set_f32 or acas2d_ppo_update_wide_set_f32)", kEntry);
        return ACAS2D_EINVAL;
    }
    switch (D) {
        case 8: rc = launch_grad_guarded<8>(*u, *g, stream); break;
        case 11: rc = launch_grad_guarded<11>(*u, *g, stream); break;
        case 14: rc = launch_grad_guarded<14>(*u, *g, stream); break;
        case 17: rc = launch_grad_guarded<17>(*u, *g, stream); break;
        case 29: rc = launch_grad_guarded<29>(*u, *g, stream); break;
        case 53: rc = launch_grad_guarded<53>(*u, *g, stream); break;
        case 101: rc = launch_grad_guarded<101>(*u, *g, stream); break;
        default: rc = launch_grad_guarded<197>(*u, *g, stream); break;
    }
    if (rc != ACAS2D_OK) return rc;                      // (a failed gradient launch must not read as a zero gradient)
    hipLaunchKernelGGL(ppo_apply_guarded_set_kernel, dim3((unsigned)u->n_members), dim3(1024), 0, stream, param_ptrs(*u), D,
                       (const float*)u->hyper, (float*)u->grad, (float*)u->adam_m, (float*)u->adam_v, u->adam_step,
                       (float*)u->stats, u->n_rows, (const float*)g->target_kl, g->stopped, (float*)g->diag);
    return launched("acas2d_ppo_update_guarded_set launch");
}
