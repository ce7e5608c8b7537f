"""The encounter search's kernels (csrc/acas2d_search.hip) stay in registers: from the code-object metadata of the unit
compiled with the flags the Makefile gives it (helpers.kernel_metadata), no VGPR spill, no SGPR spill and no private
segment at all."""
import helpers as H


@H.needs_hipcc
def test_search_kernels_stay_in_registers(tmp_path):
    _, kernels = H.kernel_metadata(tmp_path, "acas2d_search.hip")
    names = sorted(k.name for k in kernels)
    assert len(names) == 5 and sum("encounter_sample_kernel" in n for n in names) == 2
    assert sum("encounter_select_kernel" in n for n in names) == 2 and sum("encounter_refit_kernel" in n for n in names) == 1
    for k in kernels:
        assert k.field("vgpr_spill_count") == 0 and k.field("sgpr_spill_count") == 0, k.name
        assert k.field("private_segment_fixed_size") == 0, k.name
