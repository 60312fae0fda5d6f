"""The contract of the mel-cepstrum with an all-pass warp (world/melcep.py, wh_melcep_filter: include/world_hip.h, DESIGN
section 23) in plain NumPy — the SPTK convention.

Rows c[0 .. m], 1 <= m <= 64, code a POWER spectrum row P[k], k < K = N / 2 + 1, on the axis

    beta(w) = w + 2 atan2(alpha sin w, 1 - alpha cos w),   beta_k = beta(pi k / (K - 1)),   -1 < alpha < 1:
    log P[k] = 2 sum_j c[j] cos(j beta_k).

    coding    q = irfft(log P)[0 .. N/2], q[0] and q[N/2] halved, c = freqt(q, m, alpha) (SPTK's recursion, below).
    MCD       per pair of rows, (10 / ln 10) sqrt(2 sum_{j >= 1} (a[j] - b[j])^2).
    filter    the windows, row map, segment, response and overlap-add of tests/_specfilter_reference.py with the gain
              G_w[k] = exp(sum_j d[j] cos(j beta_k)) cis(-sum_j d[j] sin(j beta_k)), d = num[r] - den[r] (no den: num[r]):
              exp(sum_j d[j] z~^-j) is minimum phase as it stands, so nothing is folded.

gain_rows forms the two sums directly (the kernel runs a Clenshaw recurrence: its order of operations is not part of the
contract)."""
import numpy as np

from _specfilter_reference import errors, hann, n_windows, window_map  # noqa: F401  (the geometry is the spectral filter's)

# sp2mc(mc2sp(c)) against c, max|difference| / max|c|: 8 x the worst value over the grid of
# tests/test_melcep_reference_host.py (N, m, alpha) in {512, 1024, 2048, 4096} x {1, 24, 39, 59, 64} x {0, .42, .554, -.3}
# The worst is at N = 512, m = 64, alpha = 0.554 and is not rounding: the unwarped cepstrum of a warped row never ends,
# and irfft folds what lies beyond N / 2 back (8.8e-13 at m = 59 of the same N and alpha).  Every other shape of the grid
# returns the rows to ROUND_TRIP_ROUNDING_WORST.
ROUND_TRIP_WORST = 9.57e-9
ROUND_TRIP_BOUND = 8 * ROUND_TRIP_WORST
ROUND_TRIP_ROUNDING_WORST = 3.0e-16
# filter_melcep against _specfilter_reference.filter_spectrum on the materialised envelopes, relative RMS: 8 x the worst
# value over the cases of the same test (3.50e-15 at N = 2048, m = 60, alpha = 0.55 with a denominator; closed form
# against cepstral fold, everything else is shared)
FOLD_GAP_WORST = 3.50e-15
FOLD_GAP_BOUND = 8 * FOLD_GAP_WORST
# wh_melcep_filter against filter_melcep, per sample relative to max|y|: 8 x the worst value measured on an MI355X over
# tests/_melcep_cases.py (SAMPLE_WORST, set by SAMPLE_WORST_CASE; DESIGN section 23 has the table)
SAMPLE_WORST = 3.67e-15
SAMPLE_WORST_CASE = "m=64 N=4096"
SAMPLE_BOUND = 8 * SAMPLE_WORST

MUTANTS = ("max_phase", "not_halved", "doubled", "swapped", "neg_alpha", "seed_off_by_one")


def beta(w, alpha):
    w = np.asarray(w)
    return w + 2 * np.arctan2(alpha * np.sin(w), 1 - alpha * np.cos(w))


def warped_axis(k_bins, alpha, dtype=np.float64):
    w = np.arange(k_bins, dtype=dtype) * (np.pi if dtype == np.float64 else np.arctan(dtype(1)) * 4) / dtype(k_bins - 1)
    return beta(w, dtype(alpha))


def freqt(q, m, alpha):
    """q [..., L] -> c [..., m + 1]: the coefficients of sum_n q[n] z^-n in powers of z~^-1, SPTK's recursion."""
    q = np.asarray(q)
    alpha = q.dtype.type(alpha)
    g = np.zeros(q.shape[:-1] + (m + 1,), dtype=q.dtype)
    for i in range(q.shape[-1] - 1, -1, -1):
        d = g.copy()
        g[..., 0] = q[..., i] + alpha * d[..., 0]
        g[..., 1] = (1 - alpha * alpha) * d[..., 0] + alpha * d[..., 1]
        for j in range(2, m + 1):
            g[..., j] = d[..., j - 1] + alpha * (d[..., j] - g[..., j - 1])
    return g


def _irfft_half(lp):
    """irfft(lp)[..., 0 .. N/2] in lp's own precision (np.fft for float64, the cosine sum itself otherwise)."""
    k_bins = lp.shape[-1]
    n = 2 * (k_bins - 1)
    if lp.dtype == np.float64:
        return np.fft.irfft(lp, n, axis=-1)[..., :k_bins]
    t = lp.dtype.type
    pi = np.arctan(t(1)) * 4
    kn = (np.arange(k_bins)[:, None] * np.arange(k_bins)[None, :]) % n  # (exact integers: the angle is reduced first)
    basis = np.cos(kn.astype(t) * (2 * pi / t(n)))
    wgt = np.full(k_bins, 2, dtype=t)
    wgt[0] = wgt[-1] = 1
    return (lp * wgt) @ basis / t(n)


def sp2mc(p, m, alpha, mutant=None):
    """Power-spectrum rows [..., K] -> mel-cepstra [..., m + 1], in p's precision."""
    p = np.asarray(p)
    q = _irfft_half(np.log(p))
    if mutant != "q0_not_halved":
        q[..., 0] = q[..., 0] / 2
    q[..., -1] = q[..., -1] / 2
    return freqt(q, m, alpha)


def log_spectrum(c, k_bins, alpha):
    c = np.asarray(c)
    b = warped_axis(k_bins, alpha, c.dtype.type)
    return 2 * (c @ np.cos(np.arange(c.shape[-1], dtype=c.dtype)[:, None] * b[None, :]))


def mc2sp(c, k_bins, alpha):
    return np.exp(log_spectrum(c, k_bins, alpha))


def mcd_db(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return 10.0 / np.log(10.0) * np.sqrt(2.0 * np.sum((a[..., 1:] - b[..., 1:]) ** 2, axis=-1))


def gain_rows(num, den, k_bins, alpha, mutant=None):
    """G [F][K] complex from rows [F][m + 1]."""
    num = np.asarray(num, dtype=np.float64)
    d = num if den is None else num - np.asarray(den, dtype=np.float64)
    if mutant == "swapped":
        d = -d
    if mutant == "seed_off_by_one":  # a recurrence seeded one step late never sees d[m]
        d = d[:, :-1]
    b = warped_axis(k_bins, -alpha if mutant == "neg_alpha" else alpha)
    jb = np.arange(d.shape[1], dtype=np.float64)[:, None] * b[None, :]
    with np.errstate(all="ignore"):
        re, im = d @ np.cos(jb), d @ np.sin(jb)
        if mutant == "not_halved":
            re, im = 2 * re, 2 * im
        if mutant == "doubled":
            re, im = re / 2, im / 2
        if mutant == "max_phase":
            im = -im
        return np.exp(re) * (np.cos(im) - 1j * np.sin(im))


def filter_gain(x, gain, wmap, hop, n):
    """One utterance: x [ny] through the gains G [F][K] (complex half spectra) under the row map: y [ny].  The windows are
    _specfilter_reference.filter_rows's."""
    x = np.asarray(x, dtype=np.float64)
    ny, hop = len(x), int(hop)
    y = np.zeros(ny)
    n_win = n_windows(ny, hop)
    if n_win == 0:
        return y
    wmap = np.asarray(wmap)
    assert len(wmap) == n_win and 2 * hop - 1 <= n
    start = np.arange(n_win) * hop - hop
    g = start[:, None] + np.arange(2 * hop - 1)[None, :]
    seg = np.zeros((n_win, n))
    ok = (g >= 0) & (g < ny)
    seg[:, :2 * hop - 1] = np.where(ok, x[np.clip(g, 0, ny - 1)], 0.0) * hann(hop)[None, :]
    with np.errstate(all="ignore"):
        resp = np.fft.irfft(np.fft.rfft(seg, axis=1) * gain[wmap], n, axis=1)
    for w in range(n_win):
        t = start[w] + np.arange(n)
        ok = (t >= 0) & (t < ny)
        y[t[ok]] += resp[w][ok]
    return y


def filter_melcep(x, num, den, wmap, hop, n, alpha, mutant=None):
    return filter_gain(x, gain_rows(num, den, n // 2 + 1, alpha, mutant), wmap, hop, n)


def random_rows(rng, frames, m):
    """c[0] ~ N(0, 2), c[j] ~ N(0, 1) / j."""
    c = rng.randn(frames, m + 1)
    c[:, 0] *= 2.0
    c[:, 1:] /= np.arange(1, m + 1)[None, :]
    return c
