"""Helper of tests/test_hip_dtw_bounds.py: runs in a process whose WH_LIB is the bounds build
(tools/build_variants.py dtw_bounds=wh_api:-DWH_BOUNDS=1;wh_dtw:-DWH_BOUNDS=1: the three kernels of csrc/wh_dtw.hip index
their global and LDS buffers through wh::ckp there).  The shape list of tests/test_hip_dtw.py (tests/_dtw_cases.py).
Prints one JSON line."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "python-world_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import _dtw_cases as dc
    from world import _hip

    rt = _hip.Runtime.get()
    out = {"bounds_build": _hip.bounds_build(), "cases": []}
    for case in dc.kernel_cases():
        bad = dc.compare(dc.run(rt, case), case)
        fl = rt.take_flags()
        out["cases"].append({"name": case.name, "equal": not bad, "flags": fl, "record": list(_hip.bounds_last()),
                             "first": bad[:3]})
    print("BOUNDS_JSON " + json.dumps(out))


if __name__ == "__main__":
    main()
