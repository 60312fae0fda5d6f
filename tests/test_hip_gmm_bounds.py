"""GPU: gmm_rows_kernel, gmm_stats_kernel and gmm_combine_kernel in the bounds build (csrc/wh_device.h, wh::ckp: every
global buffer of the kernels is a checked pointer under -DWH_BOUNDS=1 — the rows, the tables, gamma, best, the partial
sums in the context's scratch and every output).  A variant of its own (wh_api and wh_gmm instrumented) runs the shape list
of tests/test_hip_gmm.py (tests/_gmm_cases.py) in a child process: zero out-of-range records, zero flags, and the results
of the shipped library bit for bit."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BOUNDS_TUS = ("wh_api", "wh_gmm")
VARIANT = os.path.join(ROOT, "python-world_amd", "lib", "variants", "libworld_hip_gmm_bounds.so")


def build_variant():
    spec = "gmm_bounds=" + ";".join("%s:-DWH_BOUNDS=1" % tu for tu in BOUNDS_TUS)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "build_variants.py"), spec], capture_output=True,
                       text=True, timeout=1500)
    assert r.returncode == 0 and "gmm_bounds ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.fixture(scope="module")
def report():
    lib = os.path.join(ROOT, "python-world_amd", "lib", "libworld_hip.so")
    if not os.path.exists(VARIANT) or os.path.getmtime(VARIANT) < os.path.getmtime(lib):
        build_variant()
    env = dict(os.environ, WH_LIB=VARIANT)
    r = subprocess.run([sys.executable, os.path.join(HERE, "_gmm_bounds_script.py")], capture_output=True, text=True,
                       env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("BOUNDS_JSON ")][-1]
    return json.loads(line[len("BOUNDS_JSON "):])


def test_variant_is_a_bounds_build(report):
    assert report["bounds_build"] is True


def test_kernels_stay_inside_their_buffers(report):
    import _gmm_cases as gc

    assert [c["name"] for c in report["cases"]] == [r.name for r in gc.all_runs()]
    bad = [c for c in report["cases"] if c["flags"] != [0] * 16 or c["record"] != [0, 0, 0, 0]]
    assert bad == []


def test_results_equal_the_shipped_library(report):
    import _gmm_cases as gc
    from world import _hip

    assert not _hip.bounds_build()
    rt = _hip.Runtime.get()
    shipped = {r.name: gc.digest(r.fn(rt)) for r in gc.all_runs()}
    differ = [c["name"] for c in report["cases"] if c["digest"] != shipped[c["name"]]]
    assert differ == []
