"""Helper of tests/test_hip_psola_bounds.py: runs in a process whose WH_LIB is the bounds build (tests/_variants.py,
psola_bounds: the three kernels of csrc/wh_psola.hip index their global buffers, the grain records and their LDS through
wh::ckp there), or without WH_LIB in one that loads the shipped library.  The case list of tests/test_hip_psola.py
(tests/_psola_cases.py), the hostile tracks included.  Per case what differs from the reference, the deferred flags, the
out-of-range record and a digest of the outputs' bytes."""
import _variants as V


def main():
    import _psola_cases as pc
    from world import _hip

    rt = _hip.Runtime.get()
    rep = V.Report(rt)
    for case in pc.all_cases():
        got = pc.run(rt, case)
        rep.case(case.name, bad=pc.compare_case(case, got), digest=V.digest([a for k in pc.FIELDS for a in got.get(k, [])]))
    rep.emit()


if __name__ == "__main__":
    main()
