// acas2d_ppo.hpp -- what the two translation units of the PPO minibatch update share: the flat gradient / moment
// layout, the network's pointer block, the wave reduction, and the apply launch (norm, clip_grad_norm_, Adam), which
// is width-agnostic and lives once, in acas2d_ppo.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

}  // namespace ppo

// ppo_apply_kernel on the 13 parameter tensors of `u` (acas2d_ppo.hip); ACAS2D_OK or ACAS2D_EHIP with the error set
int launch_ppo_apply(const Acas2dPpoUpdate& u, hipStream_t stream);

}  // namespace acas2d
