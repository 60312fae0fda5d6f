"""Helper of tests/test_hip_gmm_bounds.py: runs in a process whose WH_LIB is the bounds build
(tools/build_variants.py gmm_bounds=wh_api:-DWH_BOUNDS=1;wh_gmm:-DWH_BOUNDS=1: the kernels of csrc/wh_gmm.hip index their
global buffers through wh::ckp there).  The runs of tests/test_hip_gmm.py (tests/_gmm_cases.py); per run the flags, the
out-of-range record and a digest of the results.  Prints one JSON line."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "python-world_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import _gmm_cases as gc
    from world import _hip

    rt = _hip.Runtime.get()
    out = {"bounds_build": _hip.bounds_build(), "cases": []}
    for run in gc.all_runs():
        got = run.fn(rt)
        fl = rt.take_flags()
        out["cases"].append({"name": run.name, "digest": gc.digest(got), "flags": fl, "record": list(_hip.bounds_last())})
    print("BOUNDS_JSON " + json.dumps(out))


if __name__ == "__main__":
    main()
