"""Helper of tests/test_hip_wsola_bounds.py: runs in a process whose WH_LIB is the bounds build (tests/_variants.py,
wsola_bounds: the two kernels of csrc/wh_wsola.hip index their global buffers, the window table and their LDS through
wh::ckp there), or without WH_LIB in one that loads the shipped library.  The case list of tests/test_hip_wsola.py
(tests/_wsola_cases.py).  Per case what differs from the reference, the deferred flags, the out-of-range record and a
digest of the outputs' bytes."""
import _variants as V


def main():
    import _wsola_cases as wc
    from world import _hip

    rt = _hip.Runtime.get()
    rep = V.Report(rt)
    for case in wc.all_cases():
        got = wc.run(rt, case)
        rep.case(case.name, bad=wc.compare_case(case, got), digest=V.digest(got["y"] + got["delta"]))
    rep.emit()


if __name__ == "__main__":
    main()
