// float32 instantiation (throughput mode, FAST formulation).  Built with -ffp-contract=off like the
// float64 one: only the fma()s written in the source fuse, so every instantiation (work shape, rollout,
// policy variant) rounds alike -- measured free (7.13 us either way at 65 536 x 8).
#define ACAS2D_PACKED_SHAPES(X) X(1, 1) X(2, 1) X(3, 1) X(4, 1) X(8, 1) X(4, 2) X(2, 4) X(4, 4) X(4, 8) X(4, 16) X(8, 8) X(2, 32)
namespace acas2d {
using Elem = float;
constexpr bool kFast = true;
}
#include "acas2d_launch.inl"

// the set collectors exist in float32 only
namespace acas2d {
template decltype(launch_collect_set<float>) launch_collect_set<float>;
template decltype(launch_collect_set_group<float>) launch_collect_set_group<float>;
}
ACAS2D_INSTANTIATE_SCORING
// evaluation and campaign under sensor noise and actuator disturbance: float32 only, behind every other kernel of the unit
ACAS2D_INSTANTIATE_SCORING_DISTURBED
// (training under the same noise: the disturbed set collector is acas2d_collect_disturbed.hip)

#ifdef ACAS2D_STAMPS
extern "C" int acas2d_debug_set_stamps_f32(unsigned long long* buf) {
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(acas2d::g_stamps), &buf, sizeof(buf));
}
#endif
