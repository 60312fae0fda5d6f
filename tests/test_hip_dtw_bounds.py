"""GPU: dtw_recurrence_kernel, dtw_backtrack_kernel and dtw_reverse_kernel in the bounds build (csrc/wh_device.h, wh::ckp:
every global and LDS buffer of the three kernels is a checked pointer under -DWH_BOUNDS=1 — the staged rows and the top
line in LDS, the feature rows, the back-pointer words, the strip line, the paths, the maps, the costs and the pair table).
A variant of its own (wh_api and wh_dtw instrumented) runs the shape list of tests/test_hip_dtw.py: zero out-of-range
records, and the reference's bits still."""
import pytest

import _variants as V

pytestmark = pytest.mark.gpu

report = V.report_fixture("dtw_bounds", "_dtw_bounds_script.py")


def test_variant_is_a_bounds_build(report):
    assert report["bounds_build"] is True


def test_kernels_stay_inside_their_buffers(report):
    import _dtw_cases as dc

    assert len(report["cases"]) == len(dc.kernel_cases())
    bad = [c for c in report["cases"] if c["flags"] != [0] * 16 or c["record"] != [0, 0, 0, 0] or not c["equal"]]
    assert bad == []
