"""Helper of tests/test_hip_resample_bounds.py: runs in a process whose WH_LIB is the bounds build of wh_resample
(tests/_variants.py, resample_bounds).  The short lengths at every kernel path and a mixed batch."""
import numpy as np

import _variants as V


def main():
    from scipy import signal

    from world import _hip
    from world.resample import resample_device, resample_poly

    rt = _hip.Runtime.get()
    rep = V.Report(rt)
    rng = np.random.RandomState(7)
    # short lengths at every kernel variant: rows in registers (P <= 24, 32, 48, 64), through L1, span beyond LDS
    for up, down in ((160, 441), (1, 3), (3, 1), (2, 3), (1, 2), (1, 6), (1280, 147), (147, 1280), (1, 4096), (4096, 1),
                     (4095, 4096)):
        for n in (1, 2, 37, 63, 64, 65, 1000, 20000 if up * 20000 // down < 10 ** 7 else 300):
            x = rng.randn(n)
            ok = bool(np.array_equal(resample_poly(x, up, down), signal.resample_poly(x, up, down)))
            rep.case("%d/%d n=%d" % (up, down, n), up=up, down=down, n=n, equal=ok)
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
    rep.set("mixed", rep.record("mixed", equal=bool(eq)))
    rep.emit()


if __name__ == "__main__":
    main()
