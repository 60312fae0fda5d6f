"""Helper of tests/test_hip_regrid_bounds.py: runs in a process whose WH_LIB is the bounds build
(tools/build_variants.py regrid_bounds=wh_api:-DWH_BOUNDS=1;wh_regrid:-DWH_BOUNDS=1: interp_contour_kernel,
regrid_plan_kernel and regrid_rows_kernel index their global and LDS buffers through wh::ckp there).  The inputs of
tests/test_hip_regrid.py's kernel tests and of tests/test_hip_contour.py's.  Prints one JSON line."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "python-world_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import _regrid_cases as rc
    import test_hip_contour as tc
    from world import _hip

    rt = _hip.Runtime.get()
    out = {"bounds_build": _hip.bounds_build(), "cases": []}

    def record(name, equal):
        fl = rt.take_flags()
        out["cases"].append({"name": name, "equal": bool(equal), "flags": fl, "record": list(_hip.bounds_last())})

    for k in rc.SHAPE_K:
        src, dst, rows = rc.shape_case(k)
        ref = rc.ref_batch(src, dst, rows)
        for out_shift in (0, 1):
            for in_shift in (0, 1):
                got = rc.regrid(rt, src, dst, rows, in_shift=in_shift, out_shift=out_shift)
                record("shape K=%d out+%d in+%d" % (k, out_shift, in_shift), np.array_equal(got, ref))
    rng = np.random.RandomState(2)
    for name, src, dst in rc.conversion_cases():
        rows = rng.rand(sum(len(t) for t in src), 513) + 0.05
        record("grid " + name, np.array_equal(rc.regrid(rt, src, dst, rows), rc.ref_batch(src, dst, rows)))
        gate = (rows[:, 0] > 0.4).astype(np.float64)
        record("gate " + name, np.array_equal(rc.regrid(rt, src, dst, gate, positive=True),
                                              rc.ref_batch(src, dst, gate, positive=True)))
    tp, knots = tc._frames_and_knots()
    for rule in (False, True):
        got, vuv = rc.contour(rt, tp, knots, voiced_rule=rule)
        ref = np.concatenate([np.interp(t, kt, kv) for t, (kt, kv) in zip(tp, knots)])  # (every knot value is > 0)
        record("contour voiced_rule=%s" % rule, np.array_equal(got, ref) and (vuv is None or bool(np.all(vuv == 1))))
    print("BOUNDS_JSON " + json.dumps(out))


if __name__ == "__main__":
    main()
