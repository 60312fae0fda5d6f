"""Helper of tests/test_hip_melcep_bounds.py: runs in a process whose WH_LIB is the bounds build (tests/_variants.py,
specfilter_bounds: the kernels of csrc/wh_specfilter.hip index their global buffers, the tables and their LDS through
wh::ckp there), or without WH_LIB in one that loads the shipped library.  Six cases of tests/_melcep_cases.py
(bounds_cases: one per transform length, one without a denominator, the ragged one).  Per case what differs from the
reference, the deferred flags, the out-of-range record and a digest of the outputs' bytes."""
import _variants as V


def main():
    import _melcep_cases as mc
    from world import _hip

    rt = _hip.Runtime.get()
    rep = V.Report(rt)
    for case in mc.bounds_cases():
        got = mc.run(rt, case)
        rep.case(case.name, bad=mc.compare_case(case, got)[0], digest=V.digest(got["y"]))
    rep.emit()


if __name__ == "__main__":
    main()
