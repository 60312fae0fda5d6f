"""GPU: specfilter_kernel and specfilter_gather_kernel in the bounds build (csrc/wh_device.h, wh::ckp: every buffer of the
two kernels is a checked pointer under -DWH_BOUNDS=1 — the waveform, the row map, the gain rows with their leading
dimensions, the bin table, the twiddles, the chain's two LDS buffers, the staged roots, the run's sums, the overlap-add
rows and the output).  A variant of its own (wh_api and wh_specfilter instrumented) runs the case list of
tests/test_hip_specfilter.py: zero out-of-range records, and the shipped library's bits."""
import pytest

import _variants as V

pytestmark = pytest.mark.gpu

reports = V.report_fixture("specfilter_bounds", "_specfilter_bounds_script.py", shipped=True)


def test_variant_is_a_bounds_build(reports):
    assert reports[0]["bounds_build"] is True and reports[1]["bounds_build"] is False


def test_kernels_stay_inside_their_buffers(reports):
    import _specfilter_cases as sc

    checked, shipped = reports
    assert len(checked["cases"]) == len(sc.all_cases())
    bad = [c for c in checked["cases"] if c["flags"] != [0] * 16 or c["record"] != [0, 0, 0, 0] or c["bad"]]
    assert bad == []
    # the shipped library's bits: the digests of every case's outputs agree
    assert [c["name"] for c in checked["cases"]] == [c["name"] for c in shipped["cases"]]
    assert [c["digest"] for c in checked["cases"]] == [c["digest"] for c in shipped["cases"]]
