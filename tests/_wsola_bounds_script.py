"""Helper of tests/test_hip_wsola_bounds.py: runs in a process whose WH_LIB is the bounds build
(tools/build_variants.py wsola_bounds=wh_api:-DWH_BOUNDS=1;wh_wsola:-DWH_BOUNDS=1: the two kernels of csrc/wh_wsola.hip
index their global buffers, the window table and their LDS through wh::ckp there), or without WH_LIB in one that loads the
shipped library.  The case list of tests/test_hip_wsola.py (tests/_wsola_cases.py).  Prints one JSON line: per case what
differs from the reference, the deferred flags, the out-of-range record and a digest of the outputs' bytes."""
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

    import _wsola_cases as wc
    from world import _hip

    rt = _hip.Runtime.get()
    out = {"bounds_build": _hip.bounds_build(), "cases": []}
    for case in wc.all_cases():
        got = wc.run(rt, case)
        bad = wc.compare_case(case, got)
        digest = hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in got["y"] + got["delta"])).hexdigest()
        out["cases"].append({"name": case.name, "bad": bad, "flags": rt.take_flags(), "record": list(_hip.bounds_last()),
                             "digest": digest})
    print("BOUNDS_JSON " + json.dumps(out))


if __name__ == "__main__":
    main()
