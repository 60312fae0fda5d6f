"""Helper of tests/test_hip_lsf_chain_bounds.py: runs in a process whose WH_LIB is the bounds build (tests/_variants.py,
lsf_chain_bounds: the two kernels of csrc/wh_lsf_chain.hip index their global buffers, the bin table and their LDS through
wh::ckp there), or without WH_LIB in one that loads the shipped library.  The case lists of tests/test_hip_lsf_chain.py
(tests/_lsf_chain_cases.py): every repair case out of place and in place, every kind of row, every distortion case and the
pairs with indices out of range.  Per case what differs from the reference, the deferred flags, the out-of-range record
and a digest of the outputs' bytes."""
import _variants as V


def main():
    import numpy as np

    import _lsf_chain_cases as cc
    import _lsf_chain_reference as cref
    from world import _hip

    rt = _hip.Runtime.get()
    rep = V.Report(rt)
    for case in cc.repair_cases() + tuple(cc.all_kinds_case(p) for p in cc.ORDERS):
        w, _ = cc.repair_rows_of(case)
        want, changed = cc.repair_reference(case)
        gap, hi = cref.gap_hi(case.gap)
        for in_place in ((True,) if "every kind" in case.name else (False, True)):
            got = cc.run_repair(rt, w, gap, hi, case.pad, in_place)
            rep.case("%s%s" % (case.name, " in place" if in_place else ""), bad=cc.compare_repair(got, want, changed),
                     digest=V.digest([got["out"], got["changed"]]))
    for case in cc.dist_cases():
        rows_a, rows_b, idx_a, idx_b = cc.dist_inputs(case)
        want, b1, b2 = cc.dist_reference(case)
        got = cc.run_distortion(rt, rows_a, rows_b, case.k_bins, idx_a, idx_b, case.pad)
        rep.case(case.name, bad=cc.compare_distortion(got, want, b1, b2)[0], digest=V.digest([got["out"]]))
    case = cc.dist_cases()[12]
    rows_a, rows_b, idx_a, idx_b = cc.dist_inputs(case)
    idx_a, idx_b = np.array(idx_a), np.array(idx_b)
    idx_a[0], idx_b[-1] = len(rows_a), -1
    got = cc.run_distortion(rt, rows_a, rows_b, case.k_bins, idx_a, idx_b, 1)
    bad = [] if got["rc"] == 0 and got["guards"] and np.isnan(got["out"][[0, -1]]).all() else ["indices out of range"]
    rep.case("indices out of range", bad=bad, digest=V.digest([got["out"]]))
    rep.emit()


if __name__ == "__main__":
    main()
