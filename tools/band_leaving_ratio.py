#!/usr/bin/env python3
"""How large is a bin that leaves the smoothing window inside a run, against what the window still holds?  CPU, oracle only.

The kernels' rectangular smoothing (csrc/wh_spectral.h: BandWindow) slides one windowed sum along a thread-owned run of
bins; a bin that has left the window leaves up to 2^-53 of its own size in the sum for the rest of the run.  Relative to
the output of bin k0 + r that is 2^-53 times  max |v[i]|, i among the r elements that have left  /  |band(k0 + r)|  per
departure.  This script hooks the oracle's cumsum_band_mean — every smoothing of CheapTrick and D4C goes through it —
runs the 16 and 48 kHz fixtures and the click-train inputs of tests/test_hip_d4c.py::test_d4c_rank_select_wide_dynamic_range
through the oracle, and prints the largest such ratio per smoothing call site, with the run lengths the kernels use.

    python tools/band_leaving_ratio.py        (writes what profiles/r16_band_leaving_ratio.txt holds)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import _spectral_reference as S  # noqa: E402
from oracle import aperiodicity as oap  # noqa: E402
from oracle import common as C  # noqa: E402
from oracle import envelope as oenv  # noqa: E402

D4C_FT = {512: 256, 1024: 128, 2048: 256, 4096: 512, 8192: 512}
worst = {}
label = [""]
stage = [""]
real = C.cumsum_band_mean


def run_length(n):
    k = n // 2 + 1
    ft = (256 if n >= 2048 else 128) if stage[0] == "cheaptrick" else D4C_FT[n]
    return (k + ft - 1) // ft


def hooked(spec_full, fs, fft_size, width):
    out = real(spec_full, fs, fft_size, width)
    n, k_bins = fft_size, fft_size // 2 + 1
    kr = run_length(n)
    k = np.arange(k_bins)
    r = k % kr
    top = 0.0
    for row in range(spec_full.shape[0]):
        b_lo = S.band_constants(n, fs, float(width[row]) / 2)[0]
        v = np.abs(spec_full[row]) * (fs / n)
        left = np.zeros(k_bins)
        for back in range(1, kr):  # element k + b_lo + 1 - back has left the window of bin k if the run began `back` or more bins ago
            left = np.maximum(left, np.where(r >= back, v[(k + b_lo + 1 - back) & (n - 1)], 0.0))
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(left > 0, left / np.abs(out[row]), 0.0)
        top = max(top, float(np.nanmax(ratio)))
    seq[0] += 1
    key = (label[0], stage[0], (seq[0] - 1) % 3 + 1 if stage[0] != "cheaptrick" else 1)  # (d4c: three smoothings per pass)
    worst[key] = max(worst.get(key, 0.0), top)
    return out


seq = [0]


def measure(name, x, fs, f0, vuv, tp, with_envelope=True):
    label[0] = name
    if with_envelope:
        stage[0], seq[0] = "cheaptrick", 0
        oenv.cheaptrick_np(x, fs, f0.copy(), vuv, tp, want_ps=False)
    stage[0], seq[0] = "d4c", 0
    oap.d4c_np(x, fs, f0.copy(), vuv, tp)
    stage[0], seq[0] = "d4c_requiem", 0
    oap.d4c_requiem_np(x, fs, f0.copy(), vuv, tp)


def main():
    C.cumsum_band_mean = hooked
    for tag in ("syn16k", "syn48k"):
        g = dict(np.load(os.path.join(ROOT, "tests", "golden", "golden_%s.npz" % tag)))
        measure(tag, g["x"], int(g["fs"]), g["stonemask_f0"], g["dio_vuv"], g["tp"])
    for fs in (16000, 48000):
        n = int(0.5 * fs)
        t = np.arange(n) / fs
        rng = np.random.RandomState(5)
        clicks = np.zeros(n)
        clicks[:: int(fs / 110)] = 0.8
        soft = np.convolve(clicks, np.hanning(9), mode="same") + 1e-6 * rng.randn(n)
        clicks = clicks + 1e-5 * rng.randn(n)
        burst = 1e-6 * rng.randn(n)
        nb = int(0.025 * fs)
        burst[n // 2:n // 2 + nb] += 0.5 * np.sin(2 * np.pi * 200.0 * t[:nb])
        for name, x in (("clicks", clicks), ("soft clicks", soft), ("burst", burst)):
            nf = C.frame_count(len(x), fs, 5)
            measure("%s %d Hz" % (name, fs), x, fs, np.full(nf, 115.0), np.ones(nf), C.frame_times(nf, 5))
    print("# largest |bin that has left the window inside its run| / |output of the bin being written|, per input and smoothing;")
    print("# times 2^-53 = %.2e per departure (at most run length - 1 of them) it is the relative residue the sliding sum can hold;" % S.U)
    print("# d4c's three calls: power (width cf), group delay (cf / 2), group delay (cf)")
    for (name, stg, call), ratio in worst.items():
        print("%-22s %-12s call %d  ratio %.3e  residue <= %.1e" % (name, stg, call, ratio, ratio * S.U * 8))


if __name__ == "__main__":
    main()
