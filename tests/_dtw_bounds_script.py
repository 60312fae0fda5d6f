"""Helper of tests/test_hip_dtw_bounds.py: runs in a process whose WH_LIB is the bounds build (tests/_variants.py,
dtw_bounds: the three kernels of csrc/wh_dtw.hip index their global and LDS buffers through wh::ckp there).  The shape list
of tests/test_hip_dtw.py (tests/_dtw_cases.py)."""
import _variants as V


def main():
    import _dtw_cases as dc
    from world import _hip

    rt = _hip.Runtime.get()
    rep = V.Report(rt)
    for case in dc.kernel_cases():
        bad = dc.compare(dc.run(rt, case), case)
        rep.case(case.name, equal=not bad, first=bad[:3])
    rep.emit()


if __name__ == "__main__":
    main()
