"""GPU: lpc_levinson_kernel, lsf_from_lpc_kernel and lsf_envelope_kernel in the bounds build (csrc/wh_device.h, wh::ckp:
every buffer of the three kernels is a checked pointer under -DWH_BOUNDS=1 — the rows in and out with their leading
dimensions, the grid and bin tables, the per-lane LDS columns of the recursion, the series coefficients and the bracket
slots).  A variant of its own (wh_api and wh_lsf instrumented) runs the case list of tests/test_hip_lsf.py, the
refinement predictors and the degenerate rows: zero out-of-range records, and the reference's bits still."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BOUNDS_TUS = ("wh_api", "wh_lsf")
VARIANT = os.path.join(ROOT, "python-world_amd", "lib", "variants", "libworld_hip_lsf_bounds.so")


def build_variant():
    spec = "lsf_bounds=" + ";".join("%s:-DWH_BOUNDS=1" % tu for tu in BOUNDS_TUS)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "build_variants.py"), spec], capture_output=True,
                       text=True, timeout=1500)
    assert r.returncode == 0 and "lsf_bounds ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.fixture(scope="module")
def report():
    lib = os.path.join(ROOT, "python-world_amd", "lib", "libworld_hip.so")
    if not os.path.exists(VARIANT) or os.path.getmtime(VARIANT) < os.path.getmtime(lib):
        build_variant()
    env = dict(os.environ, WH_LIB=VARIANT)
    r = subprocess.run([sys.executable, os.path.join(HERE, "_lsf_bounds_script.py")], capture_output=True, text=True,
                       env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("BOUNDS_JSON ")][-1]
    return json.loads(line[len("BOUNDS_JSON "):])


def test_variant_is_a_bounds_build(report):
    assert report["bounds_build"] is True


def test_kernels_stay_inside_their_buffers(report):
    import _lsf_cases as lc

    assert len(report["cases"]) == len(lc.kernel_cases()) + 2
    bad = [c for c in report["cases"] if c["flags"] != [0] * 16 or c["record"] != [0, 0, 0, 0] or not c["equal"]
           or not c["lsf_flag_as_expected"]]
    assert bad == []
