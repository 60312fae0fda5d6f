"""GPU: wsola_search_kernel and wsola_ola_kernel in the bounds build (csrc/wh_device.h, wh::ckp: every buffer of the two
kernels is a checked pointer under -DWH_BOUNDS=1 — the waveform, the position list, the list of frame starts, the shifts,
the window table, the output, and in LDS the template, the candidate region and the waves' winners).  A variant of its own
(wh_api and wh_wsola instrumented) runs the case list of tests/test_hip_wsola.py: zero out-of-range records, and the shipped
library's bits."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BOUNDS_TUS = ("wh_api", "wh_wsola")
VARIANT = os.path.join(ROOT, "python-world_amd", "lib", "variants", "libworld_hip_wsola_bounds.so")


def build_variant():
    spec = "wsola_bounds=" + ";".join("%s:-DWH_BOUNDS=1" % tu for tu in BOUNDS_TUS)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "build_variants.py"), spec], capture_output=True,
                       text=True, timeout=1500)
    assert r.returncode == 0 and "wsola_bounds ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def _run(lib):
    env = dict(os.environ)
    env.pop("WH_LIB", None)
    if lib:
        env["WH_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.join(HERE, "_wsola_bounds_script.py")], capture_output=True, text=True,
                       env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("BOUNDS_JSON ")][-1]
    return json.loads(line[len("BOUNDS_JSON "):])


@pytest.fixture(scope="module")
def reports():
    lib = os.path.join(ROOT, "python-world_amd", "lib", "libworld_hip.so")
    if not os.path.exists(VARIANT) or os.path.getmtime(VARIANT) < os.path.getmtime(lib):
        build_variant()
    return _run(VARIANT), _run(None)


def test_variant_is_a_bounds_build(reports):
    assert reports[0]["bounds_build"] is True and reports[1]["bounds_build"] is False


def test_kernels_stay_inside_their_buffers(reports):
    import _wsola_cases as wc

    checked, shipped = reports
    assert len(checked["cases"]) == len(wc.all_cases())
    bad = [c for c in checked["cases"] if c["flags"] != [0] * 16 or c["record"] != [0, 0, 0, 0] or c["bad"]]
    assert bad == []
    # the shipped library's bits: the digests of every case's outputs agree
    assert [c["name"] for c in checked["cases"]] == [c["name"] for c in shipped["cases"]]
    assert [c["digest"] for c in checked["cases"]] == [c["digest"] for c in shipped["cases"]]
