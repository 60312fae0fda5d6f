"""GPU: psola_marks_kernel, psola_smarks_kernel and psola_ola_kernel in the bounds build (csrc/wh_device.h, wh::ckp: every
buffer of the three kernels is a checked pointer under -DWH_BOUNDS=1 — the waveform, the three tracks, the marks and their
periods, the synthesis marks, the selection, the flips, the counts, the grain records, the output, and in LDS the template,
the candidate region and the waves' winners).  A variant of its own (wh_api and wh_psola instrumented) runs the case list of
tests/test_hip_psola.py, the hostile tracks and the source maps at the ends of the int64 range included: zero out-of-range
records, and the shipped library's bits."""
import pytest

import _variants as V

pytestmark = pytest.mark.gpu

reports = V.report_fixture("psola_bounds", "_psola_bounds_script.py", shipped=True)


def test_variant_is_a_bounds_build(reports):
    assert reports[0]["bounds_build"] is True and reports[1]["bounds_build"] is False


def test_kernels_stay_inside_their_buffers(reports):
    import _psola_cases as pc

    checked, shipped = reports
    assert len(checked["cases"]) == len(pc.all_cases())
    bad = [c for c in checked["cases"] if c["flags"] != [0] * 16 or c["record"] != [0, 0, 0, 0] or c["bad"]]
    assert bad == []
    # the shipped library's bits: the digests of every case's outputs agree
    assert [c["name"] for c in checked["cases"]] == [c["name"] for c in shipped["cases"]]
    assert [c["digest"] for c in checked["cases"]] == [c["digest"] for c in shipped["cases"]]
