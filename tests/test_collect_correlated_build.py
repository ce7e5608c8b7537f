"""The kernels of the correlated set collector (collect_set_correlated_kernel, csrc/acas2d_collect_correlated.hip) from the
code-object metadata of the unit compiled with the flags the Makefile gives it (helpers.kernel_metadata), as
test_collect_disturbed_build.py reads the white sibling's: the nine kernels exist and nothing else does, none spills a VGPR or
has a private segment, and each takes at most 256 VGPRs (two waves per SIMD) -- every shape is held to it, none is excepted.

The error state lies in the wave's LDS during the launch and its addresses in device memory are formed where
they are used (4.2r).  Observed (vgpr_count; in brackets the white sibling, collect_set_disturbed_kernel):
    (1,1) 239 (238)   (2,1) 244 (243)   (3,1) 245 (244)   (4,1) 248 (247)   (8,1) 255 (254)
    (4,2) 246 (249)   (4,4) 246 (236)   (4,8) 243 (230)   (4,16) 205 (172)"""
import re

import pytest

import helpers as H

SHAPES = ((1, 1), (2, 1), (3, 1), (4, 1), (8, 1), (4, 2), (4, 4), (4, 8), (4, 16))
_META = {}


def kernels_of(tmp_path_factory, unit):
    if unit not in _META:                                     # one compilation per unit for the module
        _META[unit] = H.kernel_metadata(tmp_path_factory.mktemp(unit[7:-4]), unit)[1]
    return _META[unit]


def by_shape(kernels, stem):
    out = {}
    for k in kernels:
        m = re.match(r"_ZN6acas2d\d+%sIfLi(\d+)ELi(\d+)ELb1E" % stem, k.name)
        if m:
            out[int(m.group(1)), int(m.group(2))] = k
    return out


def correlated(tmp_path_factory):
    return kernels_of(tmp_path_factory, "acas2d_collect_correlated.hip")


@H.needs_hipcc
def test_nine_kernels_none_spills(tmp_path_factory):
    kernels = correlated(tmp_path_factory)
    found = by_shape(kernels, "collect_set_correlated_kernel")
    assert sorted(found) == sorted(SHAPES) and len(kernels) == len(SHAPES)        # the unit holds nothing else
    for shape, k in sorted(found.items()):
        assert k.field("vgpr_spill_count") == 0 and k.field("private_segment_fixed_size") == 0, shape
        assert k.field("sgpr_spill_count") < 400, shape                              # the float32 unit's own limit


@H.needs_hipcc
@pytest.mark.parametrize("shape", SHAPES, ids=["%d,%d" % s for s in SHAPES])
def test_at_most_256_vgprs(tmp_path_factory, shape):
    k = by_shape(correlated(tmp_path_factory), "collect_set_correlated_kernel")[shape]
    assert k.field("vgpr_count") <= 256, (k.name, k.field("vgpr_count"))


@H.needs_hipcc
def test_table_beside_the_white_siblings(tmp_path_factory):
    """The table of DESIGN.md 4.2r (pytest -s shows it).  The sibling's unit still holds its nine kernels."""
    corr = by_shape(correlated(tmp_path_factory), "collect_set_correlated_kernel")
    white = by_shape(kernels_of(tmp_path_factory, "acas2d_collect_disturbed.hip"), "collect_set_disturbed_kernel")
    assert sorted(white) == sorted(SHAPES)
    print("\n<float, C, G, fast>   VGPRs (sibling)   SGPR spills (sibling)   VGPR spills   scratch")
    for s in SHAPES:
        c, w = corr[s], white[s]
        print("float, %2d, %2d, fast     %3d (%3d)          %3d (%3d)              %d            %d"
              % (s + (c.field("vgpr_count"), w.field("vgpr_count"), c.field("sgpr_spill_count"), w.field("sgpr_spill_count"),
                      c.field("vgpr_spill_count"), c.field("private_segment_fixed_size"))))
