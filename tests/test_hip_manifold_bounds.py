"""GPU: dense_stack_kernel in the bounds build (csrc/wh_device.h, wh::ckp: every global and LDS buffer of the kernel is
a checked pointer under -DWH_BOUNDS=1).  A variant of its own (wh_api and wh_manifold instrumented) runs the random
stacks of tests/test_hip_manifold.py at the tile edges, a tap with segments and kept columns, the TIMIT networks on the
stored MCEP and a ragged batch with window 2: zero out-of-range records, and the same results still."""
import pytest

import _variants as V
from world._hip import FLAG_OOB

pytestmark = pytest.mark.gpu

report = V.report_fixture("manifold_bounds", "_manifold_bounds_script.py")


def test_variant_is_a_bounds_build(report):
    assert report["bounds_build"] is True


def test_every_case_stays_inside_its_buffers(report):
    bad = [c for c in report["cases"] if c["flags"][FLAG_OOB] or c["record"] != [0, 0, 0, 0] or not c["ok"]]
    assert len(report["cases"]) == 43 and bad == []
