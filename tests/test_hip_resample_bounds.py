"""GPU: resample_kernel in the bounds build (csrc/wh_device.h, wh::ckp: every global and LDS buffer of the kernel is a
checked pointer under -DWH_BOUNDS=1).  A variant of its own (wh_api and wh_resample instrumented) runs the short
lengths at every kernel path — filter rows in registers, through L1, input spans beyond LDS, the 1280-factor and 4096
bounds — and a mixed batch of 12 utterances at 6 rates: zero out-of-range records, and scipy's results still."""
import pytest

import _variants as V
from world._hip import FLAG_OOB

pytestmark = pytest.mark.gpu

report = V.report_fixture("resample_bounds", "_resample_bounds_script.py")


def test_variant_is_a_bounds_build(report):
    assert report["bounds_build"] is True


def test_short_lengths_at_every_path_stay_inside_their_buffers(report):
    bad = [c for c in report["cases"] if c["flags"][FLAG_OOB] or c["record"] != [0, 0, 0, 0] or not c["equal"]]
    assert len(report["cases"]) == 88 and bad == []


def test_mixed_batch_stays_inside_its_buffers(report):
    m = report["mixed"]
    assert m["flags"][FLAG_OOB] == 0 and m["record"] == [0, 0, 0, 0] and m["equal"], m
