"""Helper of tests/test_hip_lsf_bounds.py: runs in a process whose WH_LIB is the bounds build (tests/_variants.py,
lsf_bounds: the three kernels of csrc/wh_lsf.hip index their global buffers, their tables and their LDS through wh::ckp
there).  The case list of tests/test_hip_lsf.py (tests/_lsf_cases.py), the refinement predictors and the degenerate rows."""
import _variants as V


def main():
    import _lsf_cases as lc
    from world import _hip

    rt = _hip.Runtime.get()
    rep = V.Report(rt)

    def record(name, bad, expect_lsf_flag):
        # WH_FLAG_LSF is these inputs' expected answer, not a finding: reported on its own and cleared from the flags
        c = rep.case(name, equal=not bad, first=bad[:3])
        c["lsf_flag_as_expected"] = int(c["flags"][_hip.FLAG_LSF] != 0) == expect_lsf_flag
        c["flags"][_hip.FLAG_LSF] = 0

    for case in lc.kernel_cases():
        record(case.name, lc.compare(lc.run(rt, case), lc.reference(case)), 0)
    a, _, _ = lc.refinement_predictors()
    x, level = lc.refinement_reference()
    record("refinement", lc.compare(lc.run_lsf(rt, a, pad=2), {"x": x, "level": level}, ("x", "level")), 1)
    r, _ = lc.degenerate_rows()
    want = lc.stages(r, 24, 129)
    got = lc.run_levinson(rt, r, 24, pad=1)
    got.update({k: v for k, v in lc.run_lsf(rt, want["a"]).items() if k != "guards"})
    got.update({k: v for k, v in lc.run_envelope(rt, want["ex"], 129).items() if k != "guards"})
    record("degenerate rows", lc.compare(got, want), 1)
    rep.emit()


if __name__ == "__main__":
    main()
