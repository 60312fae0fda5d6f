"""GPU: interp_contour_kernel, regrid_plan_kernel and regrid_rows_kernel in the bounds build (csrc/wh_device.h, wh::ckp:
every global and LDS buffer of the three kernels is a checked pointer under -DWH_BOUNDS=1).  A variant of its own (wh_api
and wh_regrid instrumented) runs the inputs of tests/test_hip_regrid.py's kernel tests — every K, both base alignments on
either side, the four grid conversions, the gate rule — and of tests/test_hip_contour.py: zero out-of-range records, and
np.interp's values still."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BOUNDS_TUS = ("wh_api", "wh_regrid")
VARIANT = os.path.join(ROOT, "python-world_amd", "lib", "variants", "libworld_hip_regrid_bounds.so")


def build_variant():
    spec = "regrid_bounds=" + ";".join("%s:-DWH_BOUNDS=1" % tu for tu in BOUNDS_TUS)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "build_variants.py"), spec], capture_output=True,
                       text=True, timeout=1500)
    assert r.returncode == 0 and "regrid_bounds ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.fixture(scope="module")
def report():
    lib = os.path.join(ROOT, "python-world_amd", "lib", "libworld_hip.so")
    if not os.path.exists(VARIANT) or os.path.getmtime(VARIANT) < os.path.getmtime(lib):
        build_variant()
    env = dict(os.environ, WH_LIB=VARIANT)
    r = subprocess.run([sys.executable, os.path.join(HERE, "_regrid_bounds_script.py")], capture_output=True, text=True,
                       env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("BOUNDS_JSON ")][-1]
    return json.loads(line[len("BOUNDS_JSON "):])


def test_variant_is_a_bounds_build(report):
    assert report["bounds_build"] is True


def test_kernels_stay_inside_their_buffers(report):
    assert len(report["cases"]) == 5 * 4 + 4 * 2 + 2
    bad = [c for c in report["cases"] if c["flags"] != [0] * 16 or c["record"] != [0, 0, 0, 0] or not c["equal"]]
    assert bad == []
