// The set collector under time-correlated and biased errors (acas2d_collect_set_correlated_f32, _group_f32;
// collect_set_correlated_kernel, Mode::CollectSet with DIST and CORR): float32, FAST formulation, the float32 unit's flags and
// its list of work shapes -- of which the collector takes the nine of the in-kernel policy: (1,1) (2,1) (3,1) (4,1) (8,1) thread
// per env, (4,2) (4,4) (4,8) (4,16) group-cooperative.  A unit of its own for the reason acas2d_collect_disturbed.hip is one:
// every kernel of every other unit keeps its place in its unit and the local labels of its assembly
// (profiles/collect_correlated_isa.txt).
#define ACAS2D_PACKED_SHAPES(X) X(1, 1) X(2, 1) X(3, 1) X(4, 1) X(8, 1) X(4, 2) X(2, 4) X(4, 4) X(4, 8) X(4, 16) X(8, 8) X(2, 32)
#define ACAS2D_LAUNCHERS_BY_NAME
namespace acas2d {
using Elem = float;
constexpr bool kFast = true;
}
#include "acas2d_launch.inl"

ACAS2D_INSTANTIATE_COLLECT_CORRELATED
