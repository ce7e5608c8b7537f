"""The kernels of the disturbed set collector (collect_set_disturbed_kernel, csrc/acas2d_collect_disturbed.hip) from the
code-object metadata of the unit compiled with the flags the Makefile gives it (helpers.kernel_metadata), as
test_disturbance_build.py reads the evaluator's: the nine kernels exist and nothing else does, none spills a VGPR or has a
private segment, and each takes at most 256 VGPRs (two waves per SIMD).

The undisturbed collectors they derive from take 277 - 338 registers thread per env: what holds the disturbed ones to 256 is in
csrc/acas2d_step_body.inl behind `LEAN`.  Observed (vgpr_count; in brackets the undisturbed sibling):
    (1,1) 238 (277)   (2,1) 243 (294)   (3,1) 244 (294)   (4,1) 247 (314)   (8,1) 254 (338)
    (4,2) 249 (278)   (4,4) 236 (253)   (4,8) 230 (260)   (4,16) 172 (242)"""
import re

import pytest

import helpers as H

SHAPES = ((1, 1), (2, 1), (3, 1), (4, 1), (8, 1), (4, 2), (4, 4), (4, 8), (4, 16))
_META = {}


def kernels_of(tmp_path_factory):
    if "k" not in _META:                                      # one compilation for the module
        _META["k"] = H.kernel_metadata(tmp_path_factory.mktemp("collect_disturbed"), "acas2d_collect_disturbed.hip")[1]
    return _META["k"]


def by_shape(kernels):
    out = {}
    for k in kernels:
        m = re.match(r"_ZN6acas2d28collect_set_disturbed_kernelIfLi(\d+)ELi(\d+)ELb1E", k.name)
        if m:
            out[int(m.group(1)), int(m.group(2))] = k
    return out


@H.needs_hipcc
def test_nine_kernels_none_spills(tmp_path_factory):
    kernels = kernels_of(tmp_path_factory)
    found = by_shape(kernels)
    assert sorted(found) == sorted(SHAPES) and len(kernels) == len(SHAPES)        # the unit holds nothing else
    for shape, k in sorted(found.items()):
        print("collect_set_disturbed_kernel<float, %d, %d>: vgpr %d sgpr %d sgpr spills %d"
              % (shape + (k.field("vgpr_count"), k.field("sgpr_count"), k.field("sgpr_spill_count"))))
        assert k.field("vgpr_spill_count") == 0 and k.field("private_segment_fixed_size") == 0, shape
        assert k.field("sgpr_spill_count") < 400, shape                              # the float32 unit's own limit


@H.needs_hipcc
@pytest.mark.parametrize("shape", SHAPES, ids=["%d,%d" % s for s in SHAPES])
def test_at_most_256_vgprs(tmp_path_factory, shape):
    k = by_shape(kernels_of(tmp_path_factory))[shape]
    assert k.field("vgpr_count") <= 256, (k.name, k.field("vgpr_count"))
