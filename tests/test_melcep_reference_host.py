"""CPU: tests/_melcep_reference.py, the NumPy statement of the mel-cepstrum with an all-pass warp and of
wh_melcep_filter's gain, checked on its own — coding a decoded row returns it, the closed-form gain is the cepstral fold
of tests/_specfilter_reference.py on the materialised envelopes, alpha = 0 is the plain cepstrum, every mutant of the
contract is caught — and the host tables of world/melcep.py against it in long double."""
import numpy as np
import pytest

import _melcep_reference as mref
import _specfilter_reference as sref

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)

FFT_SIZES = (512, 1024, 2048, 4096)
ORDERS = (1, 24, 39, 59, 64)
ALPHAS = (0, 0.42, 0.554, -0.3)

# (N, m, alpha, hop, ny): the shapes of the closed form against the fold
FOLD_CASES = ((1024, 24, .42, 80, 1500), (1024, 40, .42, 80, 900), (2048, 60, .55, 240, 3000), (512, 40, .42, 40, 700),
              (4096, 64, .554, 480, 4000), (1024, 1, -.3, 1, 40), (512, 39, 0, 256, 1200))


def test_coding_a_decoded_row_returns_it():
    """sp2mc(mc2sp(c)) == c.  The unwarped cepstrum of a warped row is infinitely long and irfft folds it at N / 2: at
    N = 512 with alpha = 0.554 the fold is visible for m = 59 (8.8e-13) and sets the worst value at m = 64; every other
    shape of the grid returns the rows to rounding (ROUND_TRIP_ROUNDING_WORST)."""
    worst, where, worst_rounding = 0.0, None, 0.0
    for n in FFT_SIZES:
        for m in ORDERS:
            for alpha in ALPHAS:
                c = mref.random_rows(np.random.RandomState(n + m), 8, m)
                back = mref.sp2mc(mref.mc2sp(c, n // 2 + 1, alpha), m, alpha)
                e = float(np.max(np.abs(back - c)) / np.max(np.abs(c)))
                if e > worst:
                    worst, where = e, (n, m, alpha)
                if not (n == 512 and alpha == 0.554 and m >= 59):
                    worst_rounding = max(worst_rounding, e)
    print("melcep round trip: worst %.3g at (N, m, alpha) = %s; without the folded shapes %.3g" % (worst, where, worst_rounding))
    assert worst <= mref.ROUND_TRIP_BOUND
    assert worst_rounding <= 8 * mref.ROUND_TRIP_ROUNDING_WORST


def test_the_closed_form_is_the_fold_on_the_materialised_envelopes():
    worst = 0.0
    for n, m, alpha, hop, ny in FOLD_CASES:
        for with_den in (True, False):
            rng = np.random.RandomState(n + m)
            f = sref.n_windows(ny, hop)
            x = rng.randn(ny)
            num, den = mref.random_rows(rng, f, m), mref.random_rows(rng, f, m)
            k = n // 2 + 1
            y = mref.filter_melcep(x, num, den if with_den else None, np.arange(f), hop, n, alpha)
            want = sref.filter_spectrum(x, mref.mc2sp(num, k, alpha), mref.mc2sp(den, k, alpha) if with_den else None, np.arange(f), hop, n)
            worst = max(worst, sref.errors(y, want)[0])
    print("melcep closed form against the fold: worst relative RMS %.3g" % worst)
    assert worst <= mref.FOLD_GAP_BOUND


def test_alpha_zero_is_the_plain_cepstrum():
    rng = np.random.RandomState(3)
    p = np.exp(rng.randn(5, 257))
    q = np.fft.irfft(np.log(p), 512, axis=1)
    for m in (1, 24, 64):
        want = q[:, :m + 1].copy()
        want[:, 0] /= 2
        assert np.array_equal(mref.sp2mc(p, m, 0.0), want)  # (freqt at alpha = 0 moves numbers and computes none)
    c = mref.random_rows(rng, 4, 24)
    w = np.pi * np.arange(257) / 256
    assert np.allclose(mref.log_spectrum(c, 257, 0.0), 2 * c @ np.cos(np.arange(25)[:, None] * w[None, :]), rtol=0, atol=1e-13)
    assert np.array_equal(mref.beta(w, 0.0), w)


def test_the_warp_is_a_monotone_map_of_the_axis_onto_itself():
    for alpha in (0.42, 0.554, -0.3):
        b = mref.warped_axis(1025, alpha)
        assert b[0] == 0.0 and abs(b[-1] - np.pi) < 4 * EPS and np.all(np.diff(b) > 0)
        assert (b[512] > np.pi / 2) == (alpha > 0)  # a positive alpha stretches the low frequencies


def test_mcd_of_a_known_difference():
    a = np.zeros((3, 25))
    b = np.zeros((3, 25))
    b[0, 0] = 5.0           # c[0] does not count
    b[1, 1] = 1.0
    b[2, 1:] = 0.1
    want = 10 / np.log(10) * np.sqrt(2 * np.array([0.0, 1.0, 24 * 0.01]))
    assert np.allclose(mref.mcd_db(a, b), want, rtol=4 * EPS, atol=0)
    assert abs(mref.mcd_db(a, b)[1] - 6.141851463713754) < 1e-14


def test_mutants_are_caught():
    n, m, alpha, hop, ny = 1024, 24, 0.42, 80, 1500
    rng = np.random.RandomState(11)
    f = sref.n_windows(ny, hop)
    x = rng.randn(ny)
    num, den = mref.random_rows(rng, f, m), mref.random_rows(rng, f, m)
    want = mref.filter_melcep(x, num, den, np.arange(f), hop, n, alpha)
    assert mref.MUTANTS == ("max_phase", "not_halved", "doubled", "swapped", "neg_alpha", "seed_off_by_one")
    for mutant in mref.MUTANTS:
        y = mref.filter_melcep(x, num, den, np.arange(f), hop, n, alpha, mutant)
        rms, worst = sref.errors(y, want)
        assert rms > 1e4 * sref.RMS_BOUND and worst > 1e4 * mref.SAMPLE_BOUND, (mutant, rms, worst)
    # coding: q[0] not halved doubles c[0] and, through freqt, moves every other coefficient
    p = mref.mc2sp(num, n // 2 + 1, alpha)
    bad = mref.sp2mc(p, m, alpha, mutant="q0_not_halved")
    assert np.max(np.abs(bad - num)) / np.max(np.abs(num)) > 1e4 * mref.ROUND_TRIP_BOUND
    assert np.max(np.abs(mref.sp2mc(p, m, alpha) - num)) / np.max(np.abs(num)) <= mref.ROUND_TRIP_BOUND


@pytest.mark.parametrize("k_bins, order, alpha", [(257, 24, 0.42), (257, 64, 0.554), (513, 1, -0.3), (513, 39, 0.0), (513, 59, 0.554)])
def test_encode_table_is_sp2mc_row_by_row(k_bins, order, alpha):
    """Row k of the table is sp2mc of the spectrum whose logarithm is the k-th unit row, in long double.  The table is
    float64: freqt's recursion is a contraction by |alpha| per step, so the roundings of its N / 2 + 1 steps sum to at
    most eps / (1 - |alpha|)^2 of the largest coefficient (5 eps at 0.554), and the real transform that follows adds
    eps log2 N of the row's norm (10 eps, the norm being below the row's largest entry times sqrt(m + 1) <= 8.1):
    64 eps of the largest entry bounds both with a factor of four in hand."""
    from world import melcep

    ref = mref.sp2mc(np.exp(np.eye(k_bins, dtype=LD)), order, alpha)
    table = melcep.encode_table(k_bins, order, alpha).w
    assert table.shape == (k_bins, order + 1) and ref.dtype == LD
    err = float(np.max(np.abs(table - ref)) / np.max(np.abs(ref)))
    print("melcep encode_table K=%d m=%d alpha=%g: %.3g of the largest entry" % (k_bins, order, alpha, err))
    assert err <= 64 * EPS
    # and the product it stands for: log P rows through the table against sp2mc itself
    c = mref.random_rows(np.random.RandomState(k_bins + order), 6, order)
    lp = mref.log_spectrum(c, k_bins, alpha)
    assert np.max(np.abs(lp @ table - mref.sp2mc(np.exp(lp), order, alpha))) <= 64 * EPS * np.max(np.abs(lp)) * np.sum(np.abs(table), axis=0).max()


@pytest.mark.parametrize("k_bins, order, alpha", [(257, 24, 0.42), (513, 64, 0.554), (1025, 59, -0.3), (2049, 1, 0.0)])
def test_decode_table_is_mc2sp(k_bins, order, alpha):
    """2 cos(j beta_k) against long double: the argument j beta is rounded (beta itself to 2 eps pi, the product once
    more), the cosine once: 2 (3 j pi + 1) eps."""
    from world import melcep

    table = melcep.decode_table(order, alpha, k_bins).w
    j = np.arange(order + 1, dtype=LD)[:, None]
    ref = 2 * np.cos(j * mref.warped_axis(k_bins, alpha, LD)[None, :])
    assert table.shape == (order + 1, k_bins)
    assert np.all(np.abs(table - ref) <= 2 * (3 * np.pi * np.arange(order + 1)[:, None] + 1) * EPS)
    c = mref.random_rows(np.random.RandomState(order), 4, order)
    # the exponent of either side errs by sum_j |c[j]| x that entry bound (+ the sum's own roundings): relative in exp
    tol = 2 * (np.abs(c) @ (2 * (3 * np.pi * np.arange(order + 1) + 1) * EPS)).max() + 4 * (order + 1) * EPS * np.abs(c @ table).max()
    assert np.max(np.abs(np.exp(c @ table) / mref.mc2sp(c, k_bins, alpha) - 1)) <= tol
    cos_b, sin_b = melcep.warp_tables(k_bins, alpha)
    b = mref.warped_axis(k_bins, alpha, LD)
    assert np.max(np.abs(cos_b - np.cos(b))) <= 4 * np.pi * EPS and np.max(np.abs(sin_b - np.sin(b))) <= 4 * np.pi * EPS
    assert cos_b[0] == 1.0 and cos_b[-1] == -1.0 and sin_b[0] == 0.0 and sin_b[-1] == 0.0
