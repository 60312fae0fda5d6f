"""Helper of tests/test_hip_exemplar_bounds.py: runs in a process whose WH_LIB is the bounds build (exemplar_bounds in
the table of tests/_variants.py: the kernels of csrc/wh_exemplar.hip index their global buffers and their LDS
through wh::ckp there), or without WH_LIB in one that loads the shipped library.  The case list of
tests/test_hip_exemplar.py (tests/_exemplar_cases.py).  Per case what differs from the reference, the deferred flags, the
out-of-range record and a digest of the outputs' bytes."""
import _variants as V


def main():
    import _exemplar_cases as xc
    from world import _hip

    rt = _hip.Runtime.get()
    rep = V.Report(rt)
    for case in xc.knn_cases():
        for splits in (xc.knn_splits(case) if case.name in xc.SPLIT_CASES else (0,)):
            got = xc.knn_run(rt, case, splits=splits)
            rep.case("knn %s splits=%d" % (case.name, splits), bad=xc.knn_compare(case, got), digest=V.digest([got["idx"], got["dist"]]))
    for case in xc.sel_cases():
        got = xc.sel_run(rt, case)
        rep.case("select " + case.name, bad=xc.sel_compare(case, got), digest=V.digest([got[k] for k in ("sel", "slot", "total", "acc")]))
    rep.emit()


if __name__ == "__main__":
    main()
