"""Helper of tests/test_hip_mlpg_bounds.py: runs in a process whose WH_LIB is the bounds build (tests/_variants.py,
mlpg_bounds: the two kernels of csrc/wh_mlpg.hip index their global buffers through wh::ckp there).  The shape list of
tests/test_hip_mlpg.py (tests/_mlpg_cases.py) and its two ragged batches."""
import _variants as V


def main():
    import _mlpg_cases as mc
    from world import _hip

    rt = _hip.Runtime.get()
    rep = V.Report(rt)
    for case in mc.kernel_cases() + (mc.RAGGED, mc.RAGGED_L2):
        bad = mc.compare(mc.run(rt, case), case)
        rep.case(case.name, equal=not bad, first=bad[:3])
    rep.emit()


if __name__ == "__main__":
    main()
