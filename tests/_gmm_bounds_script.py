"""Helper of tests/test_hip_gmm_bounds.py: runs in a process whose WH_LIB is the bounds build (tests/_variants.py,
gmm_bounds: the kernels of csrc/wh_gmm.hip index their global buffers through wh::ckp there).  The runs of
tests/test_hip_gmm.py (tests/_gmm_cases.py); per run the flags, the out-of-range record and a digest of the results."""
import _variants as V


def main():
    import _gmm_cases as gc
    from world import _hip

    rt = _hip.Runtime.get()
    rep = V.Report(rt)
    for run in gc.all_runs():
        rep.case(run.name, digest=gc.digest(run.fn(rt)))
    rep.emit()


if __name__ == "__main__":
    main()
