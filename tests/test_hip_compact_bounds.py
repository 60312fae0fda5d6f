"""GPU: ap_from_bands_kernel and ap_gate_kernel in the bounds build (csrc/wh_device.h, wh::ckp: every global and LDS
buffer of the two kernels is a checked pointer under -DWH_BOUNDS=1).  They live in wh_apbands.hip, so the variant is the one
tests/test_hip_bounds.py builds (wh_api, wh_d4c and wh_apbands instrumented, among others).  The inputs of
tests/test_hip_compact.py's bitwise and end-to-end tests: zero out-of-range records, and D4C's bits still."""
import json
import os
import subprocess
import sys

import pytest

from test_hip_bounds import VARIANT, _build_variant

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def report():
    lib = os.path.join(ROOT, "python-world_amd", "lib", "libworld_hip.so")
    if not os.path.exists(VARIANT) or os.path.getmtime(VARIANT) < os.path.getmtime(lib):
        _build_variant()
    env = dict(os.environ, WH_LIB=VARIANT)
    r = subprocess.run([sys.executable, os.path.join(HERE, "_compact_bounds_script.py")], capture_output=True, text=True,
                       env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("BOUNDS_JSON ")][-1]
    return json.loads(line[len("BOUNDS_JSON "):])


def test_variant_is_a_bounds_build(report):
    assert report["bounds_build"] is True


def test_expansion_stays_inside_its_buffers(report):
    names = [c["name"] for c in report["cases"]]
    assert names == ["syn16k", "syn48k", "ragged", "facade requiem=False", "facade requiem=True"]
    bad = [c for c in report["cases"] if c["flags"] != [0] * 16 or c["record"] != [0, 0, 0, 0] or not c["equal"]]
    assert bad == []
