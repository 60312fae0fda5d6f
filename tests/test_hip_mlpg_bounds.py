"""GPU: delta_features_kernel and mlpg_kernel in the bounds build (csrc/wh_device.h, wh::ckp: every global buffer of the two
kernels is a checked pointer under -DWH_BOUNDS=1 — the frame offsets and the frame-to-utterance table, the tracks, the
means, the variances, the multipliers in the context's scratch, the output and the pivots).  A variant of its own
(wh_api and wh_mlpg instrumented) runs the shape list of tests/test_hip_mlpg.py and the ragged batches: zero out-of-range
records, and the reference's bits still."""
import pytest

import _variants as V

pytestmark = pytest.mark.gpu

report = V.report_fixture("mlpg_bounds", "_mlpg_bounds_script.py")


def test_variant_is_a_bounds_build(report):
    assert report["bounds_build"] is True


def test_kernels_stay_inside_their_buffers(report):
    import _mlpg_cases as mc

    assert len(report["cases"]) == len(mc.kernel_cases()) + 2
    bad = [c for c in report["cases"] if c["flags"] != [0] * 16 or c["record"] != [0, 0, 0, 0] or not c["equal"]]
    assert bad == []
