"""Helper of tests/test_hip_specfilter_bounds.py: runs in a process whose WH_LIB is the bounds build (tests/_variants.py,
specfilter_bounds: the two kernels of csrc/wh_specfilter.hip index their global buffers, the tables and their LDS through
wh::ckp there), or without WH_LIB in one that loads the shipped library.  The case list of tests/test_hip_specfilter.py
(tests/_specfilter_cases.py).  Per case what differs from the reference, the deferred flags, the out-of-range record and a
digest of the outputs' bytes."""
import _variants as V


def main():
    import _specfilter_cases as sc
    from world import _hip

    rt = _hip.Runtime.get()
    rep = V.Report(rt)
    for case in sc.all_cases():
        got = sc.run(rt, case)
        rep.case(case.name, bad=sc.compare_case(case, got)[0], digest=V.digest(got["y"]))
    rep.emit()


if __name__ == "__main__":
    main()
