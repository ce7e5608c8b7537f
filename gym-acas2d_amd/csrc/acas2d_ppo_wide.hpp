// acas2d_ppo_wide.hpp -- the gradient body of the PPO minibatch update at obs_dim 53, 101, 197 (16, 32, 64 traffic
// aircraft), written once: grad_wide<D>, four waves per 64 samples and network (acas2d_ppo_wide.hip describes the
// tiling), its constants and its LDS size, and the learner it works for when that is member blockIdx.z of a [K][...] set
// (SetNets, SetMember, set_nets_of).  ppo_grad_wide_kernel<D> (acas2d_ppo_wide.hip, one learner: OneLearner),
// ppo_grad_wide_set_kernel<D> (acas2d_ppo_wide_set.hip) and ppo_grad_wide_guarded_set_kernel<D> (acas2d_ppo_guard.hip,
// target_kl; both a SetMember) are prologues in front of it, as the narrow kernels are in front of grad_narrow<D>.
#pragma once
#include "acas2d_ppo.hpp"

namespace acas2d {
namespace ppo {
namespace wide {

constexpr int kWaves = 4;                   // per workgroup: one per SIMD
constexpr int kThreads = 64 * kWaves;
constexpr int kU = kH / kWaves;             // hidden units (rows of a weight gradient) per wave
constexpr int kChunk = 4;                   // observation entries per layer-1 step (8: the weights in flight spill SGPRs)

// LDS row stride of the observation tile: odd, so that "every lane reads entry k of its own row" is conflict-free
__host__ __device__ constexpr int x_stride(int D) { return D | 1; }
// dynamic LDS in bytes: the 64 gathered row indices, 4 x [64][65] per-sample vectors, the observations, d loss / d
// output per sample, the two cross-wave partial sums
__host__ __device__ constexpr size_t lds_bytes(int D) {
    return 64 * sizeof(int64_t) + (size_t)(4 * 64 * kRow + 64 * x_stride(D) + 64 + 2 * kWaves) * sizeof(float);
}

// The gradient of one workgroup: 64 samples (one per lane, the same 64 in each of the four waves) of the network
// blockIdx.y names (0 actor, 1 critic), whose weights are wave-uniform and come through scalar loads.  `lds_raw` is
// lds_bytes(D) of dynamic LDS, 16-byte aligned.  `lr` names the learner the workgroup works for (OneLearner in
// acas2d_ppo_wide.hip, SetMember below for a member of a set):
//   lr.net()                        the six weight pointers of network blockIdx.y ([K][...] stacks for a member)
//   lr.at(n)                        the learner's element offset into a stack of n floats per learner (0 for one learner)
//   lr.idx()  lr.log_std()  lr.grad()  lr.stats()  lr.clip_range()  lr.vf_coef()       the learner's own
//   lr.diag()                       Guard only (target_kl): the learner's float[8] of KL / clip statistics
// Each is asked for WHERE IT IS USED, not up front: a member's pointers are sums, and sums formed at the top stay in
// SGPRs across layer 1, whose 64 weights in flight leave no room for them (20 SGPR spills); the stack pointers and the
// member number they are formed from are live anyway.
// Guard: the wave that adds the scalars also adds the 64 samples' KL and clipped-count terms (loss_grad) to lr.diag()[0]
// and [1], right after loss_grad: lr.diag() is asked for there, next to lr.clip_range(), and is dead again before the
// weight gradients (held to the end beside lr.stats() it costs the widest kernel an SGPR spill).
// Opts (acas2d_ppo_sb3.hip, always with Guard): lr.clip_x(is_actor) is the actor's effective clip range or the critic's
// value clip, and lr.old_val the rollout's values, for loss_grad's clipped value loss.  These are asked for at the TOP and
// kept in VGPRs: the exception to the rule above, because three more kernel arguments cannot wait in SGPRs.
template <int D, class Learner, bool Guard = false, bool Opts = false>
__device__ __forceinline__ void grad_wide(const Learner& lr, const float* obs, const float* act, const float* old_logp,
                                          const float* adv, const float* ret, int B) {
    constexpr int XS = x_stride(D);
    extern __shared__ __align__(16) unsigned char lds_raw[];
    int64_t* l_idx = reinterpret_cast<int64_t*>(lds_raw);             // [64]
    float* l_h1 = reinterpret_cast<float*>(l_idx + 64);                // [64][65]
    float* l_h2 = l_h1 + 64 * kRow;
    float* l_dz1 = l_h2 + 64 * kRow;
    float* l_dz2 = l_dz1 + 64 * kRow;
    float* l_x = l_dz2 + 64 * kRow;                                    // [64][XS], columns < D only
    float* l_do = l_x + 64 * XS;                                       // [64]
    float* l_red = l_do + 64;                                          // [2][kWaves]
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);           // wave-uniform: weight addresses stay scalar
    const int u0 = w * kU;
    const int u0v = (tid >> 6) * kU;                                   // the same in a VGPR: the atomics' addresses
    const bool is_actor = blockIdx.y == 0;
    const NetW net = lr.net();
    const int64_t* idx = lr.idx();
    const int row = blockIdx.x * 64 + lane;
    const bool live = row < B;
    const int64_t s = idx[live ? row : 0];
    if (w == 0) l_idx[lane] = s;
    // Opts: the workgroup's ONE clip (the actor's effective range or the critic's value clip) and the sample's old_val
    // address are formed HERE and pinned in VGPRs (94 to 98 of 256 in use): layer 1 has no SGPR for three more pointers
    [[maybe_unused]] float clip_x = 0.0f;
    [[maybe_unused]] const float* old_val_s = nullptr;
    if constexpr (Opts) {
        clip_x = lr.clip_x(is_actor); old_val_s = lr.old_val + s;
        asm volatile("" : "+v"(clip_x), "+v"(old_val_s));
    }

    // ---- the minibatch's advantage statistics (SB3 normalises per minibatch; torch.std is Bessel-corrected)
    float a_mean = 0.0f, a_std = 1.0f;
    if (is_actor) {                                                    // (uniform over the workgroup)
        float sum = 0.0f;
        for (int i = tid; i < B; i += kThreads) sum += adv[idx[i]];
        sum = wave_sum(sum);
        if (lane == 0) l_red[w] = sum;
        __syncthreads();
        a_mean = (l_red[0] + l_red[1] + l_red[2] + l_red[3]) / (float)B;
        float sq = 0.0f;
        for (int i = tid; i < B; i += kThreads) { const float d = adv[idx[i]] - a_mean; sq = fmaf(d, d, sq); }
        sq = wave_sum(sq);
        if (lane == 0) l_red[kWaves + w] = sq;
        __syncthreads();
        a_std = sqrtf((l_red[kWaves] + l_red[kWaves + 1] + l_red[kWaves + 2] + l_red[kWaves + 3]) / (float)(B > 1 ? B - 1 : 1));
    }
    __syncthreads();

    // ---- the 64 observation rows into LDS, coalesced along a row; nothing past column D - 1 of a row is read
    for (int e = tid; e < 64 * D; e += kThreads) {
        const int r = e / D, k = e - r * D;
        l_x[r * XS + k] = obs[l_idx[r] * D + k];
    }
    __syncthreads();

    // ---- forward: obs -> Linear(D, 64) tanh -> Linear(64, 64) tanh -> Linear(64, 1), weights by scalar loads
    // (the stacks; each layer moves the ones it reads to the learner, lr.at(), where it starts)
    const float ACAS2D_C4* w1s = (const float ACAS2D_C4*)net.w1;
    const float ACAS2D_C4* b1s = (const float ACAS2D_C4*)net.b1;
    const float ACAS2D_C4* w2s = (const float ACAS2D_C4*)net.w2;
    const float ACAS2D_C4* b2s = (const float ACAS2D_C4*)net.b2;
    const float ACAS2D_C4* w3s = (const float ACAS2D_C4*)net.w3;
    const float ACAS2D_C4* b3s = (const float ACAS2D_C4*)net.b3;
    {
        const float ACAS2D_C4* w1 = w1s + lr.at(kH * D);
        const float ACAS2D_C4* b1 = b1s + lr.at(kH);
        float z[kU];
#pragma unroll
        for (int j = 0; j < kU; ++j) z[j] = b1[u0 + j];
        const float* xr = l_x + lane * XS;
        for (int k0 = 0; k0 + kChunk <= D; k0 += kChunk) {
            float xv[kChunk];
#pragma unroll
            for (int kk = 0; kk < kChunk; ++kk) xv[kk] = xr[k0 + kk];
#pragma unroll
            for (int j = 0; j < kU; ++j)
#pragma unroll
                for (int kk = 0; kk < kChunk; ++kk) z[j] = fmaf(w1[(u0 + j) * D + k0 + kk], xv[kk], z[j]);
        }
        constexpr int kTail = D % kChunk, kT0 = D - kTail;
        if (kTail > 0) {
            float xv[kTail > 0 ? kTail : 1];
#pragma unroll
            for (int kk = 0; kk < kTail; ++kk) xv[kk] = xr[kT0 + kk];
#pragma unroll
            for (int j = 0; j < kU; ++j)
#pragma unroll
                for (int kk = 0; kk < kTail; ++kk) z[j] = fmaf(w1[(u0 + j) * D + kT0 + kk], xv[kk], z[j]);
        }
#pragma unroll
        for (int j = 0; j < kU; ++j) l_h1[lane * kRow + u0 + j] = tanhf(z[j]);
    }
    __syncthreads();
    {
        const float ACAS2D_C4* w2 = w2s + lr.at(kH * kH);
        const float ACAS2D_C4* b2 = b2s + lr.at(kH);
        float h1[kH];
#pragma unroll
        for (int k = 0; k < kH; ++k) h1[k] = l_h1[lane * kRow + k];
#pragma unroll 1
        for (int j = 0; j < kU; ++j) {
            const int i = u0 + j;
            float z = b2[i];
#pragma unroll
            for (int k = 0; k < kH; ++k) z = fmaf(w2[i * kH + k], h1[k], z);
            l_h2[lane * kRow + i] = tanhf(z);
        }
    }
    __syncthreads();
    const float ACAS2D_C4* w3 = w3s + lr.at(kH);
    const float ACAS2D_C4* b3 = b3s + lr.at(1);
    float out = b3[0];                                              // (every wave: all of them need d loss / d output)
    for (int i = 0; i < kH; ++i) out = fmaf(w3[i], l_h2[lane * kRow + i], out);

    float dout, dls, pg_s, vf_s, kl_s, cf_s;
    if constexpr (Opts)
        loss_grad<Guard, true>(is_actor, live, out, act + s, old_logp + s, adv + s, ret + s, a_mean, a_std, lr.log_std(), B,
                               clip_x, lr.vf_coef(), dout, dls, pg_s, vf_s, kl_s, cf_s, old_val_s, clip_x);
    else
        loss_grad<Guard>(is_actor, live, out, act + s, old_logp + s, adv + s, ret + s, a_mean, a_std, lr.log_std(), B,
                         lr.clip_range(), lr.vf_coef(), dout, dls, pg_s, vf_s, kl_s, cf_s);
    if (w == 0) l_do[lane] = dout;
    if constexpr (Guard) {
        if (is_actor && w == kWaves - 1) {                             // (uniform over the wave)
            const float klsum = wave_sum(kl_s), cfsum = wave_sum(cf_s);
            if (lane == 0) { atomicAdd(lr.diag() + 0, klsum); atomicAdd(lr.diag() + 1, cfsum); }
        }
    }

    // ---- backward to the pre-activations: dz2 = dout w3 (1 - h2^2), dh1 = W2^T dz2, dz1 = dh1 (1 - h1^2)
#pragma unroll
    for (int j = 0; j < kU; ++j) {
        const float h2 = l_h2[lane * kRow + u0 + j];
        l_dz2[lane * kRow + u0 + j] = dout * w3[u0 + j] * (1.0f - h2 * h2);
    }
    __syncthreads();
    {
        const float ACAS2D_C4* w2 = w2s + lr.at(kH * kH);
        float dh1[kU];
#pragma unroll
        for (int j = 0; j < kU; ++j) dh1[j] = 0.0f;
#pragma unroll 1
        for (int i = 0; i < kH; ++i) {
            const float dz2 = l_dz2[lane * kRow + i];
#pragma unroll
            for (int j = 0; j < kU; ++j) dh1[j] = fmaf(w2[i * kH + u0 + j], dz2, dh1[j]);
        }
#pragma unroll
        for (int j = 0; j < kU; ++j) {
            const float h1 = l_h1[lane * kRow + u0 + j];
            l_dz1[lane * kRow + u0 + j] = dh1[j] * (1.0f - h1 * h1);
        }
    }
    __syncthreads();

    // ---- weight gradients: the lane takes a column, the wave rows u0 .. u0 + 15, summed over the 64 samples
    float* const grad = lr.grad();
    float* g = grad + (is_actor ? 0 : net_size(D));
    {
        float acc[kU];
#pragma unroll
        for (int j = 0; j < kU; ++j) acc[j] = 0.0f;
#pragma unroll 2
        for (int q = 0; q < 64; ++q) {
            const float h1 = l_h1[q * kRow + lane];
#pragma unroll
            for (int j = 0; j < kU; ++j) acc[j] = fmaf(l_dz2[q * kRow + u0 + j], h1, acc[j]);
        }
#pragma unroll
        for (int j = 0; j < kU; ++j) atomicAdd(g + off_w2(D) + (u0v + j) * kH + lane, acc[j]);
    }
    for (int c0 = 0; c0 < D; c0 += 64) {
        const int c = c0 + lane;
        const bool col = c < D;
        const float* xc = l_x + (col ? c : D - 1);                    // (a lane past the last column re-reads it, adds nothing)
        float acc[kU];
#pragma unroll
        for (int j = 0; j < kU; ++j) acc[j] = 0.0f;
#pragma unroll 2
        for (int q = 0; q < 64; ++q) {
            const float x = xc[q * XS];
#pragma unroll
            for (int j = 0; j < kU; ++j) acc[j] = fmaf(l_dz1[q * kRow + u0 + j], x, acc[j]);
        }
        if (col) {
#pragma unroll
            for (int j = 0; j < kU; ++j) atomicAdd(g + (u0v + j) * D + c, acc[j]);
        }
    }
    // ---- the vectors, one wave each: b2, b1, w3, and the scalars
    if (w == 0) {
        float bsum = 0.0f;
        for (int q = 0; q < 64; ++q) bsum += l_dz2[q * kRow + lane];
        atomicAdd(g + off_b2(D) + lane, bsum);
    } else if (w == 1) {
        float bsum = 0.0f;
        for (int q = 0; q < 64; ++q) bsum += l_dz1[q * kRow + lane];
        atomicAdd(g + off_b1(D) + lane, bsum);
    } else if (w == 2) {
        float w3sum = 0.0f;
        for (int q = 0; q < 64; ++q) w3sum = fmaf(l_do[q], l_h2[q * kRow + lane], w3sum);
        atomicAdd(g + off_w3(D) + lane, w3sum);
    } else {
        const float dsum = wave_sum(dout), lsum = wave_sum(dls), pgsum = wave_sum(pg_s), vfsum = wave_sum(vf_s);
        if (lane == 0) {
            atomicAdd(g + off_b3(D), dsum);
            if (is_actor) { atomicAdd(grad + 2 * net_size(D), lsum); atomicAdd(lr.stats() + 0, pgsum); }
            else atomicAdd(lr.stats() + 1, vfsum);
        }
    }
}

// the 13 [K][...] stacks as the two networks' rows and log_std: a workgroup reads the row it works on (blockIdx.y)
struct SetNets { NetW n[2]; const float* log_std; };

inline SetNets set_nets_of(const Acas2dPpoUpdateSet& u) {
    const ParamPtrs q = param_ptrs(u);
    return SetNets{{{q.p[0], q.p[1], q.p[2], q.p[3], q.p[4], q.p[5]}, {q.p[6], q.p[7], q.p[8], q.p[9], q.p[10], q.p[11]}},
                   q.p[12]};
}

// member blockIdx.z of the set as grad_wide's Learner: the [K][...] stacks and what moves them to the member.  Every
// pointer of the member is a sum formed where grad_wide asks for it (the comment above grad_wide says why), diag() among
// them; diag_all is the guarded kernels' alone, old_val / clip_range_vf / scale the Opts kernels' (acas2d_ppo_sb3.hip).
struct SetMember {
    const SetNets& nets;
    const int64_t* idx_all;
    const float* hyper;                      // hyper[k]: clip_range, vf_coef, ... (grad_narrow_member, acas2d_ppo.hpp)
    float *grad_all, *stats_all;
    int B, total;                            // rows of a minibatch, floats of a gradient block
    float* diag_all = nullptr;               // diag[k], the KL / clip statistics: Guard only
    const float* old_val = nullptr;          // Opts only: the rollout's values, the value clips [K], the factors [K][4]
    const float* clip_range_vf = nullptr;
    const float* scale = nullptr;
    __device__ __forceinline__ size_t m() const { return blockIdx.z; }
    __device__ __forceinline__ NetW net() const { return nets.n[blockIdx.y]; }
    __device__ __forceinline__ size_t at(int per_member) const { return m() * (size_t)per_member; }
    __device__ __forceinline__ const int64_t* idx() const { return idx_all + m() * (size_t)B; }
    __device__ __forceinline__ const float* log_std() const { return nets.log_std + m(); }
    __device__ __forceinline__ float clip_range() const { return ((const float ACAS2D_C4*)hyper)[m() * 8]; }
    __device__ __forceinline__ float vf_coef() const { return ((const float ACAS2D_C4*)hyper)[m() * 8 + 1]; }
    __device__ __forceinline__ float* grad() const { return grad_all + m() * (size_t)total; }
    __device__ __forceinline__ float* stats() const { return stats_all + m() * 8; }
    __device__ __forceinline__ float* diag() const { return diag_all + m() * 8; }
    // ONE float32 product: hyper[k][0] * scale[k][1] (actor) or clip_range_vf[k] * scale[k][2] (critic).  The member
    // number passes through an empty asm, so that these addresses are not common subexpressions of the later ones.
    __device__ __forceinline__ float clip_x(bool is_actor) const {
        uint32_t k = blockIdx.z;
        asm volatile("" : "+s"(k));
        const float ACAS2D_C4* sc = (const float ACAS2D_C4*)scale + (size_t)k * 4;
        return is_actor ? ((const float ACAS2D_C4*)hyper)[(size_t)k * 8] * sc[1]
                        : ((const float ACAS2D_C4*)clip_range_vf)[k] * sc[2];
    }
};

// SetMember for the Opts kernels (acas2d_ppo_sb3.hip).  The three option pointers are three more kernel arguments than
// layer 1 has SGPRs for, so this learner forms the pointers that only the tail of grad_wide uses (log_std, grad, stats,
// diag) and vf_coef ONCE, in the kernel's prologue, and pins them in VGPRs, of which these kernels use 94 to 98 of 256; the
// atomics take a VGPR address as well as a scalar one.
struct OptsMember : SetMember {
    const float* log_std_v;
    float *grad_v, *stats_v, *diag_v;
    float vf_coef_v;
    __device__ __forceinline__ explicit OptsMember(const SetMember& b)
        : SetMember(b), log_std_v(b.log_std()), grad_v(b.grad()), stats_v(b.stats()), diag_v(b.diag()), vf_coef_v(b.vf_coef()) {
        asm volatile("" : "+v"(log_std_v), "+v"(grad_v), "+v"(stats_v), "+v"(diag_v), "+v"(vf_coef_v));
    }
    __device__ __forceinline__ const float* log_std() const { return log_std_v; }
    __device__ __forceinline__ float vf_coef() const { return vf_coef_v; }
    __device__ __forceinline__ float* grad() const { return grad_v; }
    __device__ __forceinline__ float* stats() const { return stats_v; }
    __device__ __forceinline__ float* diag() const { return diag_v; }
};

}  // namespace wide
}  // namespace ppo
}  // namespace acas2d
