"""The contract of wh_spectral_filter (include/world_hip.h) in plain NumPy: a recording filtered window
by window with the minimum-phase spectrum of per-frame gain rows, overlap-added.

Per utterance: x[0 .. ny), F gain rows, transform length N, K = N / 2 + 1, an integer hop H >= 1 with 2 H - 1 <= N.

    windows    W = ceil(ny / H) + 1, w = 0 .. W-1; window w starts at the 0-based sample s_w = w H - H (its centre w H - 1 is
               the reference's geometry, world/synthesisRequiem.py:84);
               win[j] = 0.5 - 0.5 cospi(2 (j + 1) / (2 H)), j < 2 H - 1, so that win[j] + win[j + H] = 1.
    row map    window w uses gain row map[w]; the default is the frame nearest in time,
               min(F - 1, max(0, floor((w H - 1) * 1000 / (fs * frame_period) + 0.5))).
    segment    seg[j] = x[s_w + j] * win[j] where 0 <= s_w + j < ny, else 0, zero-padded to N: nothing is clipped.
    gain       h[k], k < K, the half log power ratio of row r = map[w]:
               spectrum:  h = (log|num[r][k]| - log|den[r][k]|) / 2;   no den: h = log|num[r][k]| / 2.
               lsf:       rows [log E, x_1 .. x_p], x = cos w; A2 per bin as _lsf_chain_reference.a2 forms it;
                          h = ((logE_n - logE_d) - log(A2_n / A2_d)) / 2;   no den: h = (logE_n - log A2_n) / 2.
               G = the minimum-phase spectrum of h: cepstrum of the mirrored h, fold, exp.
    response   r_w = irfft(rfft(seg) * G), N real taps, circular;
               y[t] = sum over the windows with 0 <= t - s_w < N of r_w[t - s_w], 0 <= t < ny; other taps are dropped.

The order of that sum and the fusing inside the transforms are not part of the contract; results are compared at the
tolerances below (compare())."""
import numpy as np

import _lsf_chain_reference as cref

# relative RMS against this reference: the bound the suite holds the chain to (tests/test_hip_requiem.py)
RMS_BOUND = 1e-9
# per sample, relative to max|y|: 8 x the worst value measured on an MI355X over tests/_specfilter_cases.py
# (1.26e-15, N = 2048 at hop 1024; DESIGN section 19 has the table)
SAMPLE_BOUND = 8 * 1.26e-15
# unit gain, |y - x| relative to max|x|: 8 x the worst value measured on an MI355X (3.73e-16; this reference itself: 6.0e-16)
UNIT_BOUND = 8 * 3.73e-16

MUTANTS = ("start_off_by_one", "not_halved", "max_phase", "swapped", "last_window_missing", "clip")


def n_windows(ny, hop):
    return 0 if ny <= 0 else -(-int(ny) // int(hop)) + 1


def hann(hop):
    j = np.arange(2 * int(hop) - 1, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(np.pi * (2.0 * (j + 1.0) / (2.0 * float(hop))))


def window_map(ny, n_frames, hop, fs, frame_period):
    w = np.arange(n_windows(ny, hop), dtype=np.float64)
    r = np.floor((w * float(hop) - 1.0) * 1000.0 / (float(fs) * float(frame_period)) + 0.5)
    return np.minimum(n_frames - 1, np.maximum(0, r)).astype(np.int32)


def gain_spectrum(num, den=None, mutant=None):
    """h [F][K] from power-spectrum rows [F][K]."""
    with np.errstate(all="ignore"):
        ln = np.log(np.abs(np.asarray(num, dtype=np.float64)))
        ld = 0.0 if den is None else np.log(np.abs(np.asarray(den, dtype=np.float64)))
        if mutant == "swapped":
            ln, ld = ld, ln
        h = ln - ld
        return h if mutant == "not_halved" else h / 2


def gain_lsf(num, k_bins, den=None):
    """h [F][K] from rows [log E, x_1 .. x_p] (cosines)."""
    num = np.asarray(num, dtype=np.float64)
    with np.errstate(all="ignore"):
        if den is None:
            return (num[:, :1] - np.log(cref.a2(num[:, 1:], k_bins))) / 2
        den = np.asarray(den, dtype=np.float64)
        return ((num[:, :1] - den[:, :1]) - np.log(cref.a2(num[:, 1:], k_bins) / cref.a2(den[:, 1:], k_bins))) / 2


def min_phase(h, n, mutant=None):
    """Rows h [R][K] -> the minimum-phase half spectra [R][K] (world/synthesisRequiem.py:112-118)."""
    h = np.asarray(h, dtype=np.float64)
    with np.errstate(all="ignore"):
        ceps = np.fft.fft(np.concatenate([h, h[:, -2:0:-1]], axis=1), axis=1).real
        folded = np.zeros_like(ceps)
        if mutant == "max_phase":
            folded[:, 1:n // 2 + 1] = ceps[:, 1:n // 2 + 1] * 2
        else:
            folded[:, n // 2:] = ceps[:, n // 2:] * 2
        folded[:, 0] = ceps[:, 0]
        return np.exp(np.fft.ifft(folded, axis=1))[:, :n // 2 + 1]


def filter_rows(x, h, wmap, hop, n, mutant=None):
    """One utterance: x [ny] through the gain rows h [F][K] under the row map: y [ny]."""
    x = np.asarray(x, dtype=np.float64)
    ny, hop = len(x), int(hop)
    y = np.zeros(ny)
    n_win = n_windows(ny, hop)
    if n_win == 0:
        return y
    wmap = np.asarray(wmap)
    assert len(wmap) == n_win and 2 * hop - 1 <= n
    win = hann(hop)
    start = np.arange(n_win) * hop - hop + (1 if mutant == "start_off_by_one" else 0)
    g = start[:, None] + np.arange(2 * hop - 1)[None, :]
    seg = np.zeros((n_win, n))
    if mutant == "clip":
        seg[:, :2 * hop - 1] = x[np.clip(g, 0, ny - 1)] * win[None, :]
    else:
        ok = (g >= 0) & (g < ny)
        seg[:, :2 * hop - 1] = np.where(ok, x[np.clip(g, 0, ny - 1)], 0.0) * win[None, :]
    with np.errstate(all="ignore"):
        resp = np.fft.irfft(np.fft.rfft(seg, axis=1) * min_phase(h, n, mutant)[wmap], n, axis=1)
    for w in range(n_win - (1 if mutant == "last_window_missing" else 0)):
        t = start[w] + np.arange(n)
        if mutant == "clip":
            np.add.at(y, np.clip(t, 0, ny - 1), resp[w])
        else:
            ok = (t >= 0) & (t < ny)
            y[t[ok]] += resp[w][ok]
    return y


def filter_spectrum(x, num, den, wmap, hop, n, mutant=None):
    return filter_rows(x, gain_spectrum(num, den, mutant), wmap, hop, n, mutant)


def filter_lsf(x, num, den, wmap, hop, n):
    return filter_rows(x, gain_lsf(num, n // 2 + 1, den), wmap, hop, n)


def errors(got, want):
    """(relative RMS, worst sample relative to max|want|) over the finite samples of ``want``; (0, 0) for an empty or
    all-zero reference that the result equals."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if want.size == 0:
        return 0.0, 0.0
    d = got - want
    scale_rms, scale_max = np.sqrt(np.mean(want ** 2)), np.max(np.abs(want))
    if scale_max == 0.0:
        return (0.0, 0.0) if not np.any(d) else (np.inf, np.inf)
    return float(np.sqrt(np.mean(d ** 2)) / scale_rms), float(np.max(np.abs(d)) / scale_max)


def compare(got, want):
    """[] when ``got`` is ``want`` within both bounds, else what is wrong."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return ["shape %s against %s" % (got.shape, want.shape)]
    if not np.all(np.isfinite(got)):
        return ["%d samples are not finite" % int(np.sum(~np.isfinite(got)))]
    rms, worst = errors(got, want)
    bad = []
    if not rms <= RMS_BOUND:
        bad.append("relative RMS %.3g over %.3g" % (rms, RMS_BOUND))
    if not worst <= SAMPLE_BOUND:
        bad.append("worst sample %.3g of max|y| over %.3g" % (worst, SAMPLE_BOUND))
    return bad
