"""Helper of tests/test_hip_mlpg_bounds.py: runs in a process whose WH_LIB is the bounds build
(tools/build_variants.py mlpg_bounds=wh_api:-DWH_BOUNDS=1;wh_mlpg:-DWH_BOUNDS=1: the two kernels of csrc/wh_mlpg.hip index
their global buffers through wh::ckp there).  The shape list of tests/test_hip_mlpg.py (tests/_mlpg_cases.py) and its two
ragged batches.  Prints one JSON line."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "python-world_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import _mlpg_cases as mc
    from world import _hip

    rt = _hip.Runtime.get()
    out = {"bounds_build": _hip.bounds_build(), "cases": []}
    for case in mc.kernel_cases() + (mc.RAGGED, mc.RAGGED_L2):
        bad = mc.compare(mc.run(rt, case), case)
        fl = rt.take_flags()
        out["cases"].append({"name": case.name, "equal": not bad, "flags": fl, "record": list(_hip.bounds_last()),
                             "first": bad[:3]})
    print("BOUNDS_JSON " + json.dumps(out))


if __name__ == "__main__":
    main()
