"""GPU: interp_contour_kernel, regrid_plan_kernel and regrid_rows_kernel in the bounds build (csrc/wh_device.h, wh::ckp:
every global and LDS buffer of the three kernels is a checked pointer under -DWH_BOUNDS=1).  A variant of its own (wh_api
and wh_regrid instrumented) runs the inputs of tests/test_hip_regrid.py's kernel tests — every K, both base alignments on
either side, the four grid conversions, the gate rule — and of tests/test_hip_contour.py: zero out-of-range records, and
np.interp's values still."""
import pytest

import _variants as V

pytestmark = pytest.mark.gpu

report = V.report_fixture("regrid_bounds", "_regrid_bounds_script.py")


def test_variant_is_a_bounds_build(report):
    assert report["bounds_build"] is True


def test_kernels_stay_inside_their_buffers(report):
    assert len(report["cases"]) == 5 * 4 + 4 * 2 + 2
    bad = [c for c in report["cases"] if c["flags"] != [0] * 16 or c["record"] != [0, 0, 0, 0] or not c["equal"]]
    assert bad == []
