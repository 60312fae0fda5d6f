"""GPU: gmm_rows_kernel, gmm_stats_kernel and gmm_combine_kernel in the bounds build (csrc/wh_device.h, wh::ckp: every
global buffer of the kernels is a checked pointer under -DWH_BOUNDS=1 — the rows, the tables, gamma, best, the partial
sums in the context's scratch and every output).  A variant of its own (wh_api and wh_gmm instrumented) runs the shape list
of tests/test_hip_gmm.py (tests/_gmm_cases.py) in a child process: zero out-of-range records, zero flags, and the results
of the shipped library bit for bit."""
import pytest

import _variants as V

pytestmark = pytest.mark.gpu

report = V.report_fixture("gmm_bounds", "_gmm_bounds_script.py")


def test_variant_is_a_bounds_build(report):
    assert report["bounds_build"] is True


def test_kernels_stay_inside_their_buffers(report):
    import _gmm_cases as gc

    assert [c["name"] for c in report["cases"]] == [r.name for r in gc.all_runs()]
    bad = [c for c in report["cases"] if c["flags"] != [0] * 16 or c["record"] != [0, 0, 0, 0]]
    assert bad == []


def test_results_equal_the_shipped_library(report):
    import _gmm_cases as gc
    from world import _hip

    assert not _hip.bounds_build()
    rt = _hip.Runtime.get()
    shipped = {r.name: gc.digest(r.fn(rt)) for r in gc.all_runs()}
    differ = [c["name"] for c in report["cases"] if c["digest"] != shipped[c["name"]]]
    assert differ == []
