"""The case table of tests/test_hip_timebase.py: (name, fs, tp, f0, vuv) and the property each case exists for, as a
predicate on the REFERENCE's result alone (tests/_timebase_reference.py) — tests/test_timebase_reference_host.py
asserts every predicate without a GPU, so that a case cannot rot into testing nothing.

Frame times start within [0, 3 / fs]: a later start makes the reference index outside its phase array, an earlier one
makes NumPy wrap a negative index where the device clamps; neither is behaviour worth matching."""
import collections

import numpy as np

Case = collections.namedtuple("Case", "name fs tp f0 vuv why holds")
FusedCase = collections.namedtuple("FusedCase", "name fs fft_size tp f0 vuv why holds")

_memo = {}


def _grid(n, ms=5.0, t0=0.0):
    return t0 + np.arange(n) * ms / 1000.0


def _const(name, fs, hz, n, why, holds, ms=5.0, t0=0.0):
    return Case(name, fs, _grid(n, ms, t0), np.full(n, float(hz)), np.ones(n), why, holds)


def _seam(r):
    return int(np.sum(r["at"] % 1024 == 1023))


def _build():
    rng = np.random.RandomState(20240611)
    cases = []
    add = cases.append
    add(Case("two_frames_unvoiced", 16000, _grid(2), np.zeros(2), np.zeros(2), "ny = 81, two pulses",
             lambda r: r["ny"] == 81 and r["count"] == 2 and not r["vuv"].any()))
    add(Case("unvoiced_40", 16000, _grid(40), np.zeros(40), np.zeros(40), "the default f0 alone",
             lambda r: not r["vuv_s"].any() and r["count"] > 90))
    add(_const("const_40hz", 16000, 40, 60, "long noise runs", lambda r: r["noise_size"].max() >= 399))
    add(_const("const_71hz", 16000, 71, 60, "a period that is no multiple of the sample",
               lambda r: len(set(r["noise_size"][:-1].tolist())) >= 2))
    add(_const("const_500hz", 16000, 500, 60, "the default f0, voiced", lambda r: r["vuv"].all() and r["count"] > 140))
    add(_const("const_1500hz_8k", 8000, 1500, 60, "5 to 6 samples per pulse",
               lambda r: set(r["noise_size"][:-1].tolist()) == {5, 6}))
    add(_const("const_3999hz", 16000, 3999, 60, "noise_size 4 and 5: a period that slips by a sample",
               lambda r: set(r["noise_size"][:-1].tolist()) == {4, 5}))
    add(_const("const_7000hz", 16000, 7000, 60, "noise_size 2 and 3: max(3, .) bites; a crossing on the last pair ny - 2",
               lambda r: set(r["noise_size"][:-1].tolist()) == {2, 3} and r["at"][-1] == r["ny"] - 2 and
               r["draws"] > int(r["noise_size"].sum()) + 3))
    add(_const("nyquist_half_turns", 16000, 8000, 20, "phase steps of exactly pi: |d wrap| == pi is NOT a pulse (> pi)",
               lambda r: int(np.sum(np.abs(np.diff(r["wrap"])) == np.pi)) >= 5 and r["noise_size"][:-1].min() == 1))
    for div in (32, 64, 128, 256):
        add(_const("const_fs_%d" % div, 16000, 16000.0 / div, 400,
                   "crossings on the 1024-sample seam, decided by the scan's last bit", lambda r: _seam(r) >= 1))
    add(_const("const_441hz_44k", 44100, 441, 40, "a rate whose step is no binary fraction",
               lambda r: r["count"] > 80))
    n = 80
    add(Case("chirp_55_1900", 16000, _grid(n), np.geomspace(55.0, 1900.0, n), np.ones(n),
             "crossings at both ends of the seam",
             lambda r: _seam(r) >= 1 and int(np.sum(r["at"] % 1024 == 0)) >= 1))
    n = 80
    add(Case("alternating_vuv", 16000, _grid(n), np.where(np.arange(n) % 2 == 0, 180.0, 0.0),
             (np.arange(n) % 2 == 0).astype(np.float64), "voicing flips every frame",
             lambda r, n=n: 0 < r["vuv"].sum() < r["count"] and int(np.sum(np.diff(r["vuv_s"].astype(int)) != 0)) >= n - 2))
    add(Case("fractional_vuv", 16000, _grid(n), 150.0 + 60.0 * rng.rand(n), rng.uniform(0.05, 0.95, n),
             "vuv in (0, 1), as regridding leaves it", lambda r: 0 < r["vuv"].sum() < r["count"]))
    steps = rng.randint(1, 13, size=59) / 1000.0
    tp_u = np.concatenate([[0.0], np.cumsum(steps)])
    add(Case("uneven_grid", 16000, tp_u, 120.0 + 80.0 * rng.rand(60), (rng.rand(60) > 0.25).astype(np.float64),
             "the guessed segment of lerp_segment misses", lambda r: len(set(np.round(np.diff(tp_u), 6).tolist())) >= 8))
    add(Case("stretched_grid", 16000, _grid(60) * 1.7, 110.0 + 50.0 * np.sin(np.arange(60) / 5.0), np.ones(60),
             "an even grid that is no multiple of the sample", lambda r: r["count"] > 40))
    add(Case("period_1ms_48k", 48000, _grid(150, 1.0), 200.0 + 100.0 * np.sin(np.arange(150) / 9.0), np.ones(150),
             "many frames per pulse", lambda r: r["count"] > 20 and r["ny"] == 7153))
    add(_const("start_3_samples", 16000, 130, 60, "tp[0] = 3 / fs: pidx = crossing + 4",
               lambda r: np.all(r["pidx"] - r["at"] == 4), t0=3.0 / 16000))
    add(_const("start_half_sample", 16000, 130, 200, "tp[0] = 0.5 / fs: the ROUND_HALF_UP ties fall both ways",
               lambda r: set((r["pidx"] - r["at"] - 1).tolist()) == {0, 1}, t0=0.5 / 16000))
    f_on = np.full(60, 200.0)  # a period of 80 samples = one frame; the first frame's f0 puts the wraps behind samples 80 k
    f_on[0] = 7800.0 / 40.5
    add(Case("frames_on_samples", 16000, _grid(60), f_on, np.ones(60),
             "samples and pulses ON frame times (t == tp[k]): one frame, weight -1",
             lambda r: int(np.sum(np.isin(r["t"], _grid(60)))) >= 50 and int(np.sum(np.isin(r["time"], _grid(60)))) >= 50
             and int(r["same"].sum()) >= 50))
    f_last = np.full(57, 400.0)  # 57 frames: np.arange gives a sample BEHIND the last frame (ny = 80 * 56 + 2)
    f_last[-1] = 0.5
    add(Case("negative_last_increment", 16000, _grid(57), f_last, np.ones(57),
             "the last sample's extrapolated increment is negative (the scan's addends are documented non-negative)",
             lambda r: r["t"][-1] > _grid(57)[-1] and r["phase"][-1] < r["phase"][-2] and r["count"] == 111))
    f_60 = np.full(60, 400.0)  # the same contour over 60 frames: the last sample lies ON the last frame, 117 pulses
    f_60[-1] = 0.5
    add(Case("low_last_frame", 16000, _grid(60), f_60, np.ones(60), "f0 falls from 400 to 0.5 Hz inside the last frame",
             lambda r: r["count"] == 117 and r["noise_size"].max() > 60))
    n = 3500
    f_long = 100.0 + 60.0 * np.sin(np.arange(n) / 53.0)
    v_long = ((np.arange(n) // 150) % 3 != 2).astype(np.float64)
    add(Case("long_tile_parallel", 16000, _grid(n), f_long * v_long, v_long, "more than 64 x 4096 samples: the tile-parallel scan",
             lambda r: r["ny"] > 64 * 4096 and 0 < r["vuv"].sum() < r["count"] and _seam(r) >= 1))
    return cases


def _build_fused():
    out = []
    fs, fft = 16000, 1024
    lim = 3.0 * fs / (fft - 3.0)
    below = np.nextafter(lim, 0.0)
    above = np.nextafter(lim, np.inf)
    n = 48
    f = np.full(n, 140.0)
    f[4:40:6] = below
    f[5:40:6] = lim
    f[6:40:6] = above
    f[7:40:6] = 0.5 * lim
    out.append(FusedCase("around_the_limit", fs, fft, _grid(n), f, np.ones(n),
                         "voiced frames below, at and just above 3 fs / (fft_size - 3)",
                         lambda f0, vuv, fin: np.any((f0 < lim) & (fin == 500.0)) and np.any((f0 == lim) & (fin == lim))
                         and np.any((f0 == above) & (fin == above))))
    rng = np.random.RandomState(5)
    v = (rng.rand(n) > 0.4).astype(np.float64)
    f = 90.0 + 100.0 * rng.rand(n)  # non-zero everywhere, also where vuv == 0
    f[::7] = 20.0                  # and below the limit on voiced and unvoiced frames alike
    out.append(FusedCase("unvoiced_with_f0", fs, fft, _grid(n), f, v, "vuv == 0 with a non-zero f0 reads as 0",
                         lambda f0, vuv, fin: np.any((vuv == 0) & (f0 > 0) & (fin == 0)) and
                         np.any((vuv == 1) & (f0 < lim) & (fin == 500.0))))
    f = np.where(v == 0, 0.0, 120.0 + 40.0 * np.sin(np.arange(n) / 4.0))
    out.append(FusedCase("invariant", fs, fft, _grid(n), f, v, "the fused rule changes nothing: both forms give the same bits",
                         lambda f0, vuv, fin: np.array_equal(f0, fin)))
    fs, fft = 48000, 2048
    lim48 = 3.0 * fs / (fft - 3.0)
    f = np.full(n, 95.0)
    f[3::5] = np.nextafter(lim48, 0.0)
    f[4::5] = lim48
    out.append(FusedCase("around_the_limit_48k", fs, fft, _grid(n), f, np.ones(n), "the same at another rate and transform length",
                         lambda f0, vuv, fin: np.any((f0 < lim48) & (fin == 500.0)) and np.any((f0 == lim48) & (fin == lim48))))
    return out


def cases():
    if "c" not in _memo:
        _memo["c"] = _build()
    return _memo["c"]


def fused_cases():
    if "f" not in _memo:
        _memo["f"] = _build_fused()
    return _memo["f"]


def names():
    return [c.name for c in cases()]


def by_name(name):
    return {c.name: c for c in cases()}[name]


NO_PULSE = Case("no_pulse", 16000, np.array([0.0, 0.001]), np.zeros(2), np.zeros(2),
                "17 samples, no phase wrap: the reference asserts", None)


# ---- the exact scan's patterns (tests/test_hip_cumsum.py on the device, tests/test_exact_scan_model.py on its model) -----

def _late_tie(total):
    """an addend that is 1.5 ulp of the running sums in the binade of 0.75 * total: an exact rounding tie there"""
    k = int(np.floor(np.log2(0.75 * total)))
    return 3.0 * 2.0 ** (k - 53)


def scan_patterns(n, zeros=5000):
    """(name, non-negative float64[n]) — what the tile-parallel scan has to get right: exact ties early and late in the
    sequence, a carry of zero across whole tiles, 15 decades of magnitudes, and the constant increment of the unvoiced
    default.  ``zeros``: leading zeros of the zero-carry pattern (more than a tile of the scan under test)."""
    rng = np.random.RandomState(4242)
    out = []
    x = np.full(n, 0.75)
    x[1::2] = 2.0 ** -45 * 3                     # ties while the sum is in [2^8, 2^9): the front of the sequence
    out.append(("ties_a", x))
    x = np.full(n, 0.75)
    x[1::2] = _late_tie(0.375 * n)               # the same, in the binade the sum ends in
    out.append(("ties_a_late", x))
    y = np.ones(n)
    y[::3] = 2.0 ** -42                          # ulp of sums in [2^10, 2^11) is 2^-42: half-ulp ties need 2^-43
    y[1::3] = 2.0 ** -43
    out.append(("ties_b", y))
    y = np.ones(n)
    t = _late_tie(n / 3.0)
    y[::3] = t / 1.5                             # one ulp and half an ulp of the binade the sum ends in
    y[1::3] = t / 3.0
    out.append(("ties_b_late", y))
    out.append(("leading_zeros", np.concatenate([np.zeros(zeros), rng.uniform(0, 1e-3, n - zeros)])))
    out.append(("decades", 10.0 ** rng.uniform(-12, 3, n)))
    out.append(("unvoiced_default", np.full(n, 2 * np.pi * 500 / 16000.0)))
    return out
