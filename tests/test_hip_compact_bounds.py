"""GPU: ap_from_bands_kernel and ap_gate_kernel in the bounds build (csrc/wh_device.h, wh::ckp: every global and LDS
buffer of the two kernels is a checked pointer under -DWH_BOUNDS=1).  They live in wh_apbands.hip, so the variant is the one
tests/test_hip_bounds.py runs (wh_api, wh_d4c and wh_apbands instrumented, among others).  The inputs of
tests/test_hip_compact.py's bitwise and end-to-end tests: zero out-of-range records, and D4C's bits still."""
import pytest

import _variants as V

pytestmark = pytest.mark.gpu

report = V.report_fixture("bounds", "_compact_bounds_script.py")


def test_variant_is_a_bounds_build(report):
    assert report["bounds_build"] is True


def test_expansion_stays_inside_its_buffers(report):
    names = [c["name"] for c in report["cases"]]
    assert names == ["syn16k", "syn48k", "ragged", "facade requiem=False", "facade requiem=True"]
    bad = [c for c in report["cases"] if c["flags"] != [0] * 16 or c["record"] != [0, 0, 0, 0] or not c["equal"]]
    assert bad == []
