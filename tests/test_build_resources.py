"""Build-time guard (CPU, hipcc cross-compiles without a GPU): register allocation of every kernel.

A change that let hipcc hoist the in-kernel policy's weight loads out of the step loop once cost 7x
without a single wrong bit -- 4 878 SGPR spills to VGPR lanes in one kernel, nothing in any parity
test.  The code-object metadata shows that kind of accident at once."""
import re

import pytest

import helpers as H

# Mangled step_kernel<T, C, G, PACKED, FAST, Mode> names, anchored at the end of the template arguments ("EEEv"); the
# Mode values are acas2d_kernels.hpp's.  The headline pair: step_kernel<float, 4, 2, true, true,
# Mode::Step / Mode::Arena>.
HEADLINE = re.compile(r"_ZN6acas2d11step_kernelIfLi4ELi2ELb1ELb1ELNS_4ModeE[12]EEEv")
# The float32 kernels with two aircraft per lane that hold the small stack slot below: step_kernel<float, 2, G, true,
# true, M> for (G, M) = (4, Step), (4, Arena), (32, Step), (32, Arena), (32, Rollout).
TWO_PER_LANE = tuple("_ZN6acas2d11step_kernelIfLi2ELi%dELb1ELb1ELNS_4ModeE%dEEEv" % gm
                     for gm in ((4, 1), (4, 2), (32, 1), (32, 2), (32, 3)))


@H.needs_hipcc
@pytest.mark.parametrize("unit", ("acas2d_f32.hip", "acas2d_f64.hip"))
def test_no_kernel_spills_or_uses_scratch(unit, tmp_path):
    text, kernels = H.kernel_metadata(tmp_path, unit)
    assert len(kernels) >= 40
    if unit == "acas2d_f32.hip":                                                # the patterns below select what they name
        assert len([k for k in kernels if HEADLINE.match(k.name)]) == 2
    for k in kernels:
        name = k.name
        assert k.field("vgpr_spill_count") == 0, name
        if k.field("private_segment_fixed_size") != 0:                          # no scratch memory at all ...
            # ... except a small frame the register allocator reserved and then did not need (SGPR pressure: the
            # generic-walk reset_kernel, the float64 actor-critic rollouts -- not the per-step kernels): no instruction
            # may touch it.  One known exception, NON-default work shapes with two aircraft per lane (ACAS2D_SHAPE="2,4" /
            # "2,32", shape-sweep tests only): hipcc gathers four pinned launch constants into a vector there and pulls
            # operand pairs out of it through a 16-byte stack slot (4 instructions).
            code = text[text.index("\n" + name + ":"):text.index(".end_amdhsa_kernel", text.index("\n" + name + ":"))]
            touched = len(re.findall(r"\b(scratch_|buffer_)(load|store)", code))
            if name.startswith(TWO_PER_LANE):
                assert k.field("private_segment_fixed_size") <= 32 and touched <= 4, (name, touched)
            else:
                assert k.field("private_segment_fixed_size") <= 128 and touched == 0, (name, touched)
            assert not HEADLINE.match(name)                                     # the headline kernels: no frame at all
        assert k.field("sgpr_spill_count") < 400, (name, k.field("sgpr_spill_count"))
        if HEADLINE.match(name):                                                # the headline kernels: >= 4 waves / SIMD
            assert k.field("vgpr_count") <= 128, k.field("vgpr_count")


@H.needs_hipcc
def test_ppo_update_kernels_stay_in_registers(tmp_path):
    """csrc/acas2d_ppo.hip keeps three 64-entry per-lane vectors in registers (h1, dh1, a gradient row): a spill to
    scratch there would cost far more than any wrong bit would show."""
    _, kernels = H.kernel_metadata(tmp_path, "acas2d_ppo.hip")
    assert len(kernels) == 6                                     # five observation widths + the apply kernel
    for k in kernels:
        assert k.field("vgpr_spill_count") == 0 and k.field("sgpr_spill_count") == 0, k.name
        assert k.field("private_segment_fixed_size") == 0 and k.field("vgpr_count") <= 256, k.name
