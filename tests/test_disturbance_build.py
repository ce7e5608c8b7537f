"""The kernels of the disturbance model (eval_stats_disturbed_kernel, monte_carlo_disturbed_kernel and
disturbance_draw_kernel, instantiated at the end of csrc/acas2d_f32.hip) stay in registers: from the code-object metadata of
the unit compiled with the flags the Makefile gives it (helpers.kernel_metadata), no VGPR spill and no private segment at
all -- and the thread-per-env kernels keep two waves per SIMD (at most 256 VGPRs), as the kernels they derive from."""
import re

import helpers as H

SHAPES = ("Li1ELi1E", "Li2ELi1E", "Li3ELi1E", "Li4ELi1E", "Li8ELi1E", "Li4ELi2E", "Li4ELi4E", "Li4ELi8E", "Li4ELi16E")


@H.needs_hipcc
def test_disturbed_kernels_stay_in_registers(tmp_path):
    _, kernels = H.kernel_metadata(tmp_path, "acas2d_f32.hip")
    new = [k for k in kernels if "disturb" in k.name]
    names = [k.name for k in new]
    for family in ("eval_stats_disturbed_kernelIf", "monte_carlo_disturbed_kernelIf"):        # float32, every shape of the siblings
        assert sorted(re.search(family + r"(Li\d+ELi\d+E)", n).group(1) for n in names if family in n) == sorted(SHAPES), family
    assert sum("disturbance_draw_kernelIf" in n for n in names) == 1 and len(new) == 2 * len(SHAPES) + 1
    # ... and they are the LAST kernels of the unit: every other kernel keeps its place and its local labels
    assert [k.name for k in kernels[-len(new):]] == names
    for k in new:
        assert k.field("vgpr_spill_count") == 0 and k.field("private_segment_fixed_size") == 0, k.name
        assert k.field("vgpr_count") <= 256, (k.name, k.field("vgpr_count"))
