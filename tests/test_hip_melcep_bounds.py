"""GPU: specfilter_kernel's kind 2 (wh_melcep_filter) in the bounds build — the existing specfilter_bounds variant
(tests/_variants.py: wh_api and wh_specfilter under -DWH_BOUNDS=1, every buffer of the kernels a checked pointer: the
waveform, the row map, the rows with their leading dimensions, the two warp tables, the twiddles, the chain's two LDS
buffers, the staged row difference, the run's sums, the overlap-add rows and the output).  Six cases of
tests/_melcep_cases.py: zero out-of-range records, and the shipped library's bits."""
import pytest

import _variants as V

pytestmark = pytest.mark.gpu

reports = V.report_fixture("specfilter_bounds", "_melcep_bounds_script.py", shipped=True)


def test_variant_is_a_bounds_build(reports):
    assert reports[0]["bounds_build"] is True and reports[1]["bounds_build"] is False


def test_kernels_stay_inside_their_buffers(reports):
    import _melcep_cases as mc

    checked, shipped = reports
    assert len(checked["cases"]) == len(mc.bounds_cases()) == 6
    bad = [c for c in checked["cases"] if c["flags"] != [0] * 16 or c["record"] != [0, 0, 0, 0] or c["bad"]]
    assert bad == []
    assert [c["name"] for c in checked["cases"]] == [c["name"] for c in shipped["cases"]]
    assert [c["digest"] for c in checked["cases"]] == [c["digest"] for c in shipped["cases"]]
