// The evaluator with statistics and the Monte Carlo campaign under a pilot response delay and an actuation lag
// (acas2d_evaluate_policies_delayed_f32, acas2d_monte_carlo_delayed_f32 and their _group_f32 entries;
// eval_stats_delayed_kernel, monte_carlo_delayed_kernel: Mode::Eval with STATS, DIST, CORR and RESP): float32, FAST formulation, the
// float32 unit's flags and its list of work shapes -- of which the two take the nine of the in-kernel policy: (1,1) (2,1) (3,1)
// (4,1) (8,1) thread per env, (4,2) (4,4) (4,8) (4,16) group-cooperative.  A unit of its own for the reason
// acas2d_scoring_correlated.hip is one: every existing unit ends with the kernels it ended with (profiles/response_isa.txt).
#define ACAS2D_PACKED_SHAPES(X) X(1, 1) X(2, 1) X(3, 1) X(4, 1) X(8, 1) X(4, 2) X(2, 4) X(4, 4) X(4, 8) X(4, 16) X(8, 8) X(2, 32)
#define ACAS2D_LAUNCHERS_BY_NAME
namespace acas2d {
using Elem = float;
constexpr bool kFast = true;
}
#include "acas2d_launch.inl"

ACAS2D_INSTANTIATE_SCORING_DELAYED
