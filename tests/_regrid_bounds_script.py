"""Helper of tests/test_hip_regrid_bounds.py: runs in a process whose WH_LIB is the bounds build (tests/_variants.py,
regrid_bounds: interp_contour_kernel, regrid_plan_kernel and regrid_rows_kernel index their global and LDS buffers through
wh::ckp there).  The inputs of tests/test_hip_regrid.py's kernel tests and of tests/test_hip_contour.py's."""
import numpy as np

import _variants as V


def main():
    import _regrid_cases as rc
    import test_hip_contour as tc
    from world import _hip

    rt = _hip.Runtime.get()
    rep = V.Report(rt)
    for k in rc.SHAPE_K:
        src, dst, rows = rc.shape_case(k)
        ref = rc.ref_batch(src, dst, rows)
        for out_shift in (0, 1):
            for in_shift in (0, 1):
                got = rc.regrid(rt, src, dst, rows, in_shift=in_shift, out_shift=out_shift)
                rep.case("shape K=%d out+%d in+%d" % (k, out_shift, in_shift), equal=bool(np.array_equal(got, ref)))
    rng = np.random.RandomState(2)
    for name, src, dst in rc.conversion_cases():
        rows = rng.rand(sum(len(t) for t in src), 513) + 0.05
        rep.case("grid " + name, equal=bool(np.array_equal(rc.regrid(rt, src, dst, rows), rc.ref_batch(src, dst, rows))))
        gate = (rows[:, 0] > 0.4).astype(np.float64)
        rep.case("gate " + name, equal=bool(np.array_equal(rc.regrid(rt, src, dst, gate, positive=True),
                                                           rc.ref_batch(src, dst, gate, positive=True))))
    tp, knots = tc._frames_and_knots()
    for rule in (False, True):
        got, vuv = rc.contour(rt, tp, knots, voiced_rule=rule)
        ref = np.concatenate([np.interp(t, kt, kv) for t, (kt, kv) in zip(tp, knots)])  # (every knot value is > 0)
        rep.case("contour voiced_rule=%s" % rule, equal=bool(np.array_equal(got, ref) and (vuv is None or bool(np.all(vuv == 1)))))
    rep.emit()


if __name__ == "__main__":
    main()
