"""Helper of tests/test_hip_lsf_bounds.py: runs in a process whose WH_LIB is the bounds build
(tools/build_variants.py lsf_bounds=wh_api:-DWH_BOUNDS=1;wh_lsf:-DWH_BOUNDS=1: the three kernels of csrc/wh_lsf.hip index
their global buffers, their tables and their LDS through wh::ckp there).  The case list of tests/test_hip_lsf.py
(tests/_lsf_cases.py), the refinement predictors and the degenerate rows.  Prints one JSON line."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "python-world_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import _lsf_cases as lc
    from world import _hip

    rt = _hip.Runtime.get()
    out = {"bounds_build": _hip.bounds_build(), "cases": []}

    def record(name, bad, expect_lsf_flag):
        fl = rt.take_flags()
        lsf_flag = int(fl[_hip.FLAG_LSF] != 0)
        fl[_hip.FLAG_LSF] = 0
        out["cases"].append({"name": name, "equal": not bad, "flags": fl, "lsf_flag_as_expected": lsf_flag == expect_lsf_flag,
                             "record": list(_hip.bounds_last()), "first": bad[:3]})

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
    print("BOUNDS_JSON " + json.dumps(out))


if __name__ == "__main__":
    main()
