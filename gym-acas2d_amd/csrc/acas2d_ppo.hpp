// acas2d_ppo.hpp -- what the translation units of the PPO minibatch update share, each thing written once: the flat
// gradient / moment layout, the d loss / d output block (loss_grad), the one-wave gradient body of the narrow widths
// (grad_narrow<D>), the prologue that takes member blockIdx.z of a [K][...] set in front of it (grad_narrow_member<D>),
// the apply body (apply_body: norm, clip_grad_norm_, Adam), and the host helpers of the entry points (pointer check,
// set check, NetW pair, per-device LDS opt-in).  ppo_grad_kernel<D> (acas2d_ppo.hip) is a prologue of its own in front of
// grad_narrow<D>; ppo_grad_set_kernel<D> (acas2d_ppo_set.hip) and ppo_grad_guarded_set_kernel<D> (acas2d_ppo_guard.hip,
// target_kl) are grad_narrow_member<D> with Guard = false and true.  The wide kernels stand likewise in front of
// grad_wide<D> (acas2d_ppo_wide.hpp).  With Guard at its default, false, the gradient bodies are the code they were
// before the guard existed; likewise with Opts (acas2d_ppo_sb3.hip: clip_range_vf and the schedule factors).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "acas2d.h"

namespace acas2d {
void set_error(const char* fmt, ...);

namespace ppo {

constexpr int kH = 64;               // hidden width of SB3's MlpPolicy
constexpr int kRow = 65;             // LDS row stride of a per-sample 64-vector (conflict-free rows AND columns)
#define ACAS2D_C4 __attribute__((address_space(4)))

// gradient / moment block of one network, in floats: w1 [64][D], b1 [64], w2 [64][64], b2 [64], w3 [64], b3 [1]
__host__ __device__ constexpr int net_size(int D) { return kH * D + kH + kH * kH + kH + kH + 1; }
__host__ __device__ constexpr int off_b1(int D) { return kH * D; }
__host__ __device__ constexpr int off_w2(int D) { return kH * D + kH; }
__host__ __device__ constexpr int off_b2(int D) { return kH * D + kH + kH * kH; }
__host__ __device__ constexpr int off_w3(int D) { return kH * D + kH + kH * kH + kH; }
__host__ __device__ constexpr int off_b3(int D) { return kH * D + kH + kH * kH + kH + kH; }

struct NetW { const float *w1, *b1, *w2, *b2, *w3, *b3; };      // torch layouts: [out][in]
struct Nets { NetW n[2]; };                 // actor, critic: a workgroup reads the one it works on (blockIdx.y)
// the 13 parameter tensors in FusedUpdate's order (actor w1 b1 w2 b2 w3 b3, critic likewise, log_std); [K][...] stacks
// in the set update
struct ParamPtrs { float* p[13]; };

// floats in parameter tensor k of ParamPtrs: the flat gradient / moment layout is these 13 segments back to back (a
// table, not a chain of conditions: the apply loop reads it by scalar load where the chain was a dozen branches per k)
__host__ __device__ constexpr int seg_count(int D, int k) {
    constexpr int fixed[13] = {0, kH, kH * kH, kH, kH, 1, 0, kH, kH * kH, kH, kH, 1, 1};      // 0: w1, [64][D]
    return fixed[k] ? fixed[k] : kH * D;
}

// Dynamic LDS of the narrow gradient kernels: 4 x 64 per-sample vectors with row stride 65, the observations, one
// scratch row (69.6 - 74.8 KB for D = 8 ... 29)
__host__ __device__ constexpr size_t narrow_lds_bytes(int D) {
    return (size_t)(4 * 64 * kRow + 64 * (D + 1) + 64) * sizeof(float);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// d loss / d output of one sample (SB3 PPO.train(): clipped surrogate on minibatch-normalised advantages, MSE value
// loss).  act_s ... ret_s point at the sample's entries and log_std_p at the scalar: each is read only on the branch
// that needs it.  A dead lane (row >= B) contributes zeros.
// Guard (the target_kl kernels of acas2d_ppo_guard.hip): a live actor sample also gives its terms of SB3's approx_kl,
// (ratio - 1) - log ratio, and of its clip_fraction, |ratio - 1| > clip_range, from the log ratio and the ratio the
// surrogate is formed from; without it `kl_s` and `cf_s` are zeros nobody reads.
// Opts (the clip_range_vf / schedule kernels of acas2d_ppo_sb3.hip, always with Guard): `clip_range` is the caller's
// hyper[k][0] * scale[k][1], and a critic sample with clip_vf > 0 takes SB3's clipped value loss -- values_pred =
// old_val + clamp(out - old_val, -clip_vf, clip_vf), F.mse_loss(ret, values_pred), no max with the unclipped loss; torch's
// clamp passes the gradient on the closed interval.  clip_vf <= 0 or NaN (wave-uniform): the plain branch, and
// old_val_s is not read.
template <bool Guard = false, bool Opts = false>
__device__ __forceinline__ void loss_grad(bool is_actor, bool live, float out, const float* act_s, const float* old_logp_s,
                                          const float* adv_s, const float* ret_s, float a_mean, float a_std,
                                          const float* log_std_p, int B, float clip_range, float vf_coef, float& dout,
                                          float& dls, float& pg_s, float& vf_s, float& kl_s, float& cf_s,
                                          const float* old_val_s = nullptr, float clip_vf = 0.0f) {
    dout = 0.0f; dls = 0.0f; pg_s = 0.0f; vf_s = 0.0f; kl_s = 0.0f; cf_s = 0.0f;
    if (live) {
        if (is_actor) {
            const float ls = log_std_p[0], inv_var = expf(-2.0f * ls);
            const float diff = act_s[0] - out;
            const float logp = -0.5f * diff * diff * inv_var - ls - 0.9189385332046727f;
            const float a = (adv_s[0] - a_mean) / (a_std + 1e-8f);
            const float log_ratio = logp - old_logp_s[0];
            const float ratio = expf(log_ratio);
            const float surr1 = a * ratio, surr2 = a * fminf(fmaxf(ratio, 1.0f - clip_range), 1.0f + clip_range);
            pg_s = -fminf(surr1, surr2) / (float)B;
            const float dlogp = (surr1 <= surr2) ? -(a * ratio) / (float)B : 0.0f;     // torch.min: ties go to the first operand
            dout = dlogp * diff * inv_var;                       // d logp / d mean
            dls = dlogp * (diff * diff * inv_var - 1.0f);        // d logp / d log_std
            if constexpr (Guard) {
                kl_s = (ratio - 1.0f) - log_ratio;
                cf_s = fabsf(ratio - 1.0f) > clip_range ? 1.0f : 0.0f;
            }
        } else {
            if constexpr (Opts) {
                if (clip_vf > 0.0f) {
                    const float ov = old_val_s[0], d = out - ov;
                    const float e = (ov + fminf(fmaxf(d, -clip_vf), clip_vf)) - ret_s[0];
                    vf_s = e * e / (float)B;
                    dout = (d >= -clip_vf && d <= clip_vf) ? vf_coef * 2.0f * e / (float)B : 0.0f;
                    return;
                }
            }
            const float e = out - ret_s[0];
            vf_s = e * e / (float)B;
            dout = vf_coef * 2.0f * e / (float)B;
        }
    }
}

// The gradient of one wave: 64 samples (one per lane) of the network blockIdx.y names (0 actor, 1 critic), whose weights
// w1 ... b3 are wave-uniform and come through scalar loads.  The lane gathers its sample by `idx`, runs the forward,
// takes loss_grad (the advantage statistics of the WHOLE minibatch are recomputed by every actor wave: 2 B loads per
// lane, no extra launch, no grid sync) and back-propagates to the pre-activations.  The per-sample vectors (h1, h2, dz1,
// dz2) live in LDS (narrow_lds_bytes(D) at `lds`), row stride 65 so that "every lane writes its own row's element i" and
// "every lane reads column t of row s" are both conflict-free; the weight gradients are then sums over the 64 samples
// of outer products, taken by thread t for row t of each weight matrix, and added to `grad` with float atomics.
// Guard: an actor wave also adds its samples' KL and clipped-count terms (loss_grad) to diag[0] and diag[1].
// Opts: `clip_range` is the effective one, and a critic wave with clip_vf > 0 gathers old_val[s] (loss_grad).
template <int D, bool Guard = false, bool Opts = false>
__device__ __forceinline__ void grad_narrow(const float ACAS2D_C4* w1, const float ACAS2D_C4* b1, const float ACAS2D_C4* w2,
                                            const float ACAS2D_C4* b2, const float ACAS2D_C4* w3, const float ACAS2D_C4* b3,
                                            const float* log_std_p, const float* obs, const float* act,
                                            const float* old_logp, const float* adv, const float* ret, const int64_t* idx,
                                            int B, float clip_range, float vf_coef, float* grad, float* stats, float* lds,
                                            float* diag = nullptr, const float* old_val = nullptr, float clip_vf = 0.0f) {
    float* l_h1 = lds;                       // [64][65]
    float* l_h2 = l_h1 + 64 * kRow;
    float* l_dz1 = l_h2 + 64 * kRow;
    float* l_dz2 = l_dz1 + 64 * kRow;
    float* l_x = l_dz2 + 64 * kRow;          // [64][D + 1]
    float* l_do = l_x + 64 * (D + 1);        // [64]
    const int lane = threadIdx.x;
    const bool is_actor = blockIdx.y == 0;
    const int row = blockIdx.x * 64 + lane;
    const bool live = row < B;
    const int64_t s = idx[live ? row : 0];
    // Opts: the sample's old_val address is formed HERE and pinned in VGPRs (there is room: 144 of 256 in use), so that old_val
    // does not sit in two SGPRs across layer 2, whose 64 weights in flight leave none
    [[maybe_unused]] const float* old_val_s = nullptr;
    if constexpr (Opts) { old_val_s = old_val + s; asm volatile("" : "+v"(old_val_s)); }

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

    float dout, dls, pg_s, vf_s, kl_s, cf_s;
    if constexpr (Opts)
        loss_grad<Guard, true>(is_actor, live, out, act + s, old_logp + s, adv + s, ret + s, a_mean, a_std, log_std_p, B,
                               clip_range, vf_coef, dout, dls, pg_s, vf_s, kl_s, cf_s, old_val_s, clip_vf);
    else
        loss_grad<Guard>(is_actor, live, out, act + s, old_logp + s, adv + s, ret + s, a_mean, a_std, log_std_p, B, clip_range,
                         vf_coef, dout, dls, pg_s, vf_s, kl_s, cf_s);
    l_do[lane] = dout;
    if constexpr (Guard) {                                   // (here, not beside the stats atomics: the two terms die at once)
        if (is_actor) {                                      // (uniform over the wave)
            const float klsum = wave_sum(kl_s), cfsum = wave_sum(cf_s);
            if (lane == 0) { atomicAdd(diag + 0, klsum); atomicAdd(diag + 1, cfsum); }
        }
    }

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

// Member blockIdx.z of a set in front of grad_narrow: its slices of the [K][...] parameter stacks, its minibatch
// idx[k][.], its gradient block grad[k], its stats[k], its clip_range and vf_coef from hyper[k] by scalar load (hyper[k]:
// clip_range, vf_coef, ent_coef, max_grad_norm, learning_rate, beta1, beta2, adam_eps) and, Guard only, its diag[k].  The
// rollout buffer (obs ... ret) is ONE flat buffer shared by all members; idx holds its global row numbers.
// Opts: an actor workgroup's clip range is hyper[k][0] * scale[k][1], a critic workgroup's value clip clip_range_vf[k] *
// scale[k][2], one float32 product each, by scalar loads on the branch that needs them (scale: float[K][4]).
template <int D, bool Guard = false, bool Opts = false>
__device__ __forceinline__ void grad_narrow_member(const ParamPtrs& prm, const float* obs, const float* act,
                                                   const float* old_logp, const float* adv, const float* ret,
                                                   const int64_t* idx_all, int B, const float* hyper, float* grad_all,
                                                   float* stats_all, float* lds, float* diag_all = nullptr,
                                                   const float* old_val = nullptr, const float* clip_range_vf = nullptr,
                                                   const float* scale = nullptr) {
    const bool is_actor = blockIdx.y == 0;
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

    if constexpr (Opts) {
        const float ACAS2D_C4* sc = (const float ACAS2D_C4*)(scale + m * 4);
        // the workgroup's ONE clip (the actor's range or the critic's value clip), kept in a VGPR for the same reason
        float clip = is_actor ? clip_range * sc[1] : ((const float ACAS2D_C4*)clip_range_vf)[m] * sc[2];
        // so are the pointers only the atomics at the end use: eight SGPRs that layer 2 then has for its weights
        float* diag = diag_all + m * 8;
        asm volatile("" : "+v"(clip), "+v"(grad), "+v"(stats), "+v"(diag), "+v"(log_std_p));
        grad_narrow<D, Guard, true>(w1, b1, w2, b2, w3, b3, log_std_p, obs, act, old_logp, adv, ret, idx, B, clip, vf_coef,
                                    grad, stats, lds, diag, old_val, clip);
    } else {
        grad_narrow<D, Guard>(w1, b1, w2, b2, w3, b3, log_std_p, obs, act, old_logp, adv, ret, idx, B, clip_range, vf_coef,
                              grad, stats, lds, Guard ? diag_all + m * 8 : nullptr);
    }
}

// One 1 024-thread workgroup: the global gradient norm, torch.nn.utils.clip_grad_norm_'s coefficient, Adam
// (torch.optim.Adam's bias-corrected form) on the 13 tensors prm.p[k] + member * seg_count(D, k) in place, gradient
// zeroed for the next minibatch.  grad / m / v / step / stats are the learner's own; the gradient and the statistics
// accumulate for ONE minibatch.
__device__ __forceinline__ void apply_body(const ParamPtrs& prm, size_t member, int D, float* grad, float* m, float* v,
                                           int32_t* step, float* stats, float ent_coef, float max_norm, float lr,
                                           float beta1, float beta2, float eps) {
    __shared__ float red[16];
    __shared__ float coef_s;
    const int tid = threadIdx.x;
    const int total = 2 * net_size(D) + 1;
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
        float* p = prm.p[k] + member * (size_t)count;
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

// ---- host side of the entry points; U is Acas2dPpoUpdate or Acas2dPpoUpdateSet, which name their pointers alike
template <class U>
ParamPtrs param_ptrs(const U& u) {
    return ParamPtrs{{(float*)u.actor_w1, (float*)u.actor_b1, (float*)u.actor_w2, (float*)u.actor_b2, (float*)u.actor_w3,
                      (float*)u.actor_b3, (float*)u.critic_w1, (float*)u.critic_b1, (float*)u.critic_w2, (float*)u.critic_b2,
                      (float*)u.critic_w3, (float*)u.critic_b3, (float*)u.log_std}};
}

inline Nets nets_of(const Acas2dPpoUpdate& u) {
    const ParamPtrs q = param_ptrs(u);
    return Nets{{{q.p[0], q.p[1], q.p[2], q.p[3], q.p[4], q.p[5]}, {q.p[6], q.p[7], q.p[8], q.p[9], q.p[10], q.p[11]}}};
}

// every pointer of `u` (and `more`: the set's hyper) is required, and n_rows >= 2; ACAS2D_OK or ACAS2D_EINVAL with the
// error set in the name of `entry`
template <class U>
int check_update(const U* u, const char* entry, const void* more, const char* rows_note) {
    if (!u) { set_error("%s: NULL argument", entry); return ACAS2D_EINVAL; }
    const ParamPtrs q = param_ptrs(*u);
    const void* need[] = {u->obs, u->act, u->old_logp, u->adv, u->ret, u->idx, u->grad, u->adam_m, u->adam_v, u->adam_step,
                          u->stats, more};
    bool ok = true;
    for (const float* p : q.p) ok = ok && p;
    for (const void* p : need) ok = ok && p;
    if (!ok) { set_error("%s: every pointer is required", entry); return ACAS2D_EINVAL; }
    if (u->n_rows >= 2) return ACAS2D_OK;
    set_error("%s: n_rows = %d (the advantage normalisation needs 2%s)", entry, u->n_rows, rows_note);
    return ACAS2D_EINVAL;
}

// check_update for a set (hyper is required too), and 1 to 65535 members
inline int check_set(const Acas2dPpoUpdateSet* u, const char* entry) {
    const int rc = check_update(u, entry, u ? u->hyper : nullptr, "; every member takes the same number of rows");
    if (rc != ACAS2D_OK) return rc;
    if (u->n_members >= 1 && u->n_members <= 65535) return ACAS2D_OK;
    set_error("%s: n_members = %d (1 to 65535 members, one grid plane each)", entry, u->n_members);
    return ACAS2D_EINVAL;
}

// A launch with more than 64 KB of dynamic LDS has to raise the kernel's limit first.  That attribute belongs to a
// (kernel, device) pair, so what was asked for is remembered PER DEVICE (0: not asked yet): a process that updates on a
// second device asks again there, and two threads in a first call at worst both ask.  ACAS2D_EINVAL where the device
// offers less than `bytes` (gfx950: 160 KB per workgroup).
template <auto Kernel>
int ensure_dynamic_lds(size_t bytes, const char* entry) {
    constexpr int kMaxDevices = 64;
    static std::atomic<int> asked[kMaxDevices];              // per kernel and device
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { set_error("%s: cannot query the current device", entry); return ACAS2D_EHIP; }
    const bool known = dev >= 0 && dev < kMaxDevices;
    int limit = known ? asked[dev].load(std::memory_order_acquire) : 0;
    if (limit == 0) {
        int optin = 0;
        if (hipDeviceGetAttribute(&optin, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) {
            set_error("%s: cannot query the device's LDS size", entry); return ACAS2D_EHIP; }
        if ((size_t)optin >= bytes)
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        (void)hipGetLastError();
        limit = optin > 0 ? optin : -1;
        if (known) asked[dev].store(limit, std::memory_order_release);
    }
    if (limit < 0 || (size_t)limit < bytes) {
        set_error("%s: the gradient kernel needs %zu bytes of LDS per workgroup, this device offers %d (built for gfx950's "
                  "160 KB)", entry, bytes, limit < 0 ? 0 : limit);
        return ACAS2D_EINVAL;
    }
    return ACAS2D_OK;
}

// after a launch: ACAS2D_OK, or ACAS2D_EHIP with "<what>: <the runtime's words>"
inline int launched(const char* what) {
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) { set_error("%s: %s", what, hipGetErrorString(err)); return ACAS2D_EHIP; }
    return ACAS2D_OK;
}

}  // namespace ppo

// ppo_apply_kernel on the 13 parameter tensors of `u` (acas2d_ppo.hip); ACAS2D_OK or ACAS2D_EHIP with the error set
int launch_ppo_apply(const Acas2dPpoUpdate& u, hipStream_t stream);
// ppo_apply_set_kernel on the K members of `u`, whatever its obs_dim (acas2d_ppo_set.hip); likewise
int launch_ppo_apply_set(const Acas2dPpoUpdateSet& u, hipStream_t stream);

}  // namespace acas2d
