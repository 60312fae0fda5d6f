"""GPU: delta_features_kernel and mlpg_kernel in the bounds build (csrc/wh_device.h, wh::ckp: every global buffer of the two
kernels is a checked pointer under -DWH_BOUNDS=1 — the frame offsets and the frame-to-utterance table, the tracks, the
means, the variances, the multipliers in the context's scratch, the output and the pivots).  A variant of its own
(wh_api and wh_mlpg instrumented) runs the shape list of tests/test_hip_mlpg.py and the ragged batches: zero out-of-range
records, and the reference's bits still."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BOUNDS_TUS = ("wh_api", "wh_mlpg")
VARIANT = os.path.join(ROOT, "python-world_amd", "lib", "variants", "libworld_hip_mlpg_bounds.so")


def build_variant():
    spec = "mlpg_bounds=" + ";".join("%s:-DWH_BOUNDS=1" % tu for tu in BOUNDS_TUS)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "build_variants.py"), spec], capture_output=True,
                       text=True, timeout=1500)
    assert r.returncode == 0 and "mlpg_bounds ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.fixture(scope="module")
def report():
    lib = os.path.join(ROOT, "python-world_amd", "lib", "libworld_hip.so")
    if not os.path.exists(VARIANT) or os.path.getmtime(VARIANT) < os.path.getmtime(lib):
        build_variant()
    env = dict(os.environ, WH_LIB=VARIANT)
    r = subprocess.run([sys.executable, os.path.join(HERE, "_mlpg_bounds_script.py")], capture_output=True, text=True,
                       env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("BOUNDS_JSON ")][-1]
    return json.loads(line[len("BOUNDS_JSON "):])


def test_variant_is_a_bounds_build(report):
    assert report["bounds_build"] is True


def test_kernels_stay_inside_their_buffers(report):
    import _mlpg_cases as mc

    assert len(report["cases"]) == len(mc.kernel_cases()) + 2
    bad = [c for c in report["cases"] if c["flags"] != [0] * 16 or c["record"] != [0, 0, 0, 0] or not c["equal"]]
    assert bad == []
