"""GPU: lsf_repair_kernel and lsf_distortion_kernel in the bounds build (csrc/wh_device.h, wh::ckp: every buffer of the
two kernels is a checked pointer under -DWH_BOUNDS=1 — the angles in and out with their leading dimensions, the per-frame
counts, the LDS tile of the repair; the two row matrices, the two index lists, the bin table, the staged roots and the
pairs' sums of the distortion).  A variant of its own (wh_api and wh_lsf_chain instrumented) runs the case lists of
tests/test_hip_lsf_chain.py: zero out-of-range records, and the shipped library's bits."""
import pytest

import _variants as V

pytestmark = pytest.mark.gpu

reports = V.report_fixture("lsf_chain_bounds", "_lsf_chain_bounds_script.py", shipped=True)


def test_variant_is_a_bounds_build(reports):
    assert reports[0]["bounds_build"] is True and reports[1]["bounds_build"] is False


def test_kernels_stay_inside_their_buffers(reports):
    import _lsf_chain_cases as cc

    checked, shipped = reports
    assert len(checked["cases"]) == 2 * len(cc.repair_cases()) + len(cc.ORDERS) + len(cc.dist_cases()) + 1
    bad = [c for c in checked["cases"] if c["flags"] != [0] * 16 or c["record"] != [0, 0, 0, 0] or c["bad"]]
    assert bad == []
    # the shipped library's bits: the digests of every case's outputs agree
    assert [c["name"] for c in checked["cases"]] == [c["name"] for c in shipped["cases"]]
    assert [c["digest"] for c in checked["cases"]] == [c["digest"] for c in shipped["cases"]]
