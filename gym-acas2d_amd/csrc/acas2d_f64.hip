// float64 instantiation (parity mode, EXACT formulation).  Built with -ffp-contract=off: the only
// fused multiply-adds are the explicit ones that mirror the reference's OpenBLAS ddot
// (kinematics.py:11,77).
#define ACAS2D_PACKED_SHAPES(X) X(1, 1) X(3, 1) X(2, 1) X(4, 1) X(2, 4) X(4, 2) X(4, 4) X(4, 8) X(2, 32) X(4, 16)
namespace acas2d {
using Elem = double;
constexpr bool kFast = false;
}
#include "acas2d_launch.inl"
ACAS2D_INSTANTIATE_SCORING
