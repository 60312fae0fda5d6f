"""Helper of tests/test_hip_resample_bounds.py: runs in a process whose WH_LIB is the bounds build of wh_resample
(tools/build_variants.py resample_bounds=wh_api:-DWH_BOUNDS=1;wh_resample:-DWH_BOUNDS=1).  Prints one JSON line."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "python-world_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    from scipy import signal

    from world import _hip
    from world.resample import resample_device, resample_poly

    out = {"bounds_build": _hip.bounds_build()}
    rt = _hip.Runtime.get()
    rng = np.random.RandomState(7)
    cases = []
    # short lengths at every kernel variant: rows in registers (P <= 24, 32, 48, 64), through L1, span beyond LDS
    for up, down in ((160, 441), (1, 3), (3, 1), (2, 3), (1, 2), (1, 6), (1280, 147), (147, 1280), (1, 4096), (4096, 1),
                     (4095, 4096)):
        for n in (1, 2, 37, 63, 64, 65, 1000, 20000 if up * 20000 // down < 10 ** 7 else 300):
            x = rng.randn(n)
            ok = bool(np.array_equal(resample_poly(x, up, down), signal.resample_poly(x, up, down)))
            fl = rt.take_flags()
            cases.append({"up": up, "down": down, "n": n, "equal": ok, "flag": fl[_hip.FLAG_OOB],
                          "record": list(_hip.bounds_last())})
    # the mixed batch: 12 utterances at 6 rates, empty and one-sample ones among them
    rates = (44100, 48000, 22050, 24000, 8000, 96000)
    xs, fss = [], []
    for u in range(12):
        fs = rates[u % 6]
        xs.append(rng.randn([fs, 37, fs // 3, 1, 2 * fs, 0][u // 2 % 6]))
        fss.append(fs)
    off = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    ups = [16000 // np.gcd(16000, f) for f in fss]
    downs = [f // np.gcd(16000, f) for f in fss]
    y_d, yo = resample_device(rt, rt.to_device(np.concatenate(xs)), off, ups, downs)
    y = y_d.cpu().numpy()
    eq = all(np.array_equal(y[yo[u]:yo[u + 1]], signal.resample_poly(xs[u], 16000, fss[u])) for u in range(12))
    fl = rt.take_flags()
    out["mixed"] = {"equal": bool(eq), "flag": fl[_hip.FLAG_OOB], "record": list(_hip.bounds_last())}
    out["cases"] = cases
    print("BOUNDS_JSON " + json.dumps(out))


if __name__ == "__main__":
    main()
