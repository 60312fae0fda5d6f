"""Helper of tests/test_hip_specfilter_bounds.py: runs in a process whose WH_LIB is the bounds build
(tools/build_variants.py specfilter_bounds=wh_api:-DWH_BOUNDS=1;wh_specfilter:-DWH_BOUNDS=1: the two kernels of
csrc/wh_specfilter.hip index their global buffers, the tables and their LDS through wh::ckp there), or without WH_LIB in
one that loads the shipped library.  The case list of tests/test_hip_specfilter.py (tests/_specfilter_cases.py).  Prints
one JSON line: per case what differs from the reference, the deferred flags, the out-of-range record and a digest of the
outputs' bytes."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "python-world_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import numpy as np

    import _specfilter_cases as sc
    from world import _hip

    rt = _hip.Runtime.get()
    out = {"bounds_build": _hip.bounds_build(), "cases": []}
    for case in sc.all_cases():
        got = sc.run(rt, case)
        bad = sc.compare_case(case, got)[0]
        digest = hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in got["y"])).hexdigest()
        out["cases"].append({"name": case.name, "bad": bad, "flags": rt.take_flags(), "record": list(_hip.bounds_last()),
                             "digest": digest})
    print("BOUNDS_JSON " + json.dumps(out))


if __name__ == "__main__":
    main()
