"""The case list of tests/test_hip_exemplar.py under the bounds build of csrc/wh_exemplar.hip (every global and LDS access
of its kernels compared with the range it may touch): no out-of-range record, no flag, the reference's results, and the
shipped library's bytes."""
import pytest

import _variants as V

pytestmark = pytest.mark.gpu

report = V.report_fixture("exemplar_bounds", "_exemplar_bounds_script.py", shipped=True)


def test_the_variant_is_a_bounds_build(report):
    checked, shipped = report
    assert checked["bounds_build"] and not shipped["bounds_build"]
    assert len(checked["cases"]) == len(shipped["cases"]) > 60


def test_no_access_out_of_range_no_flag_and_the_reference(report):
    for c in report[0]["cases"]:
        assert c["record"][0] == 0, (c["name"], c["record"])
        assert c["flags"] == [0] * 16 and c["bad"] == [], (c["name"], c["flags"], c["bad"])


def test_the_shipped_library_gives_the_same_bytes(report):
    checked, shipped = report
    for a, b in zip(checked["cases"], shipped["cases"]):
        assert a["name"] == b["name"] and a["digest"] == b["digest"], a["name"]
        assert b["bad"] == [] and b["flags"] == [0] * 16
