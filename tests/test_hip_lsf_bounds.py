"""GPU: lpc_levinson_kernel, lsf_from_lpc_kernel and lsf_envelope_kernel in the bounds build (csrc/wh_device.h, wh::ckp:
every buffer of the three kernels is a checked pointer under -DWH_BOUNDS=1 — the rows in and out with their leading
dimensions, the grid and bin tables, the per-lane LDS columns of the recursion, the series coefficients and the bracket
slots).  A variant of its own (wh_api and wh_lsf instrumented) runs the case list of tests/test_hip_lsf.py, the
refinement predictors and the degenerate rows: zero out-of-range records, and the reference's bits still."""
import pytest

import _variants as V

pytestmark = pytest.mark.gpu

report = V.report_fixture("lsf_bounds", "_lsf_bounds_script.py")


def test_variant_is_a_bounds_build(report):
    assert report["bounds_build"] is True


def test_kernels_stay_inside_their_buffers(report):
    import _lsf_cases as lc

    assert len(report["cases"]) == len(lc.kernel_cases()) + 2
    bad = [c for c in report["cases"] if c["flags"] != [0] * 16 or c["record"] != [0, 0, 0, 0] or not c["equal"]
           or not c["lsf_flag_as_expected"]]
    assert bad == []
