"""CPU: (a) the comparator of tests/_feature_reference.py checked on itself — a plain float64 np.dot of every shape
tests/test_hip_feature_matmul.py runs stays within the derived bound, and five ways a kernel could be wrong are rejected;
(b) the host tables behind the feature heads and warp_spectrum (world/features.py, world/_tables.py), which restate
np.fft.irfft / rfft, np.interp and the mel filterbank as matrices and gather tables, against a NumPy restatement of the
reference's own expressions (world/main.py:191-196, 275-358) at sizes and rates the fixtures do not have."""
import numpy as np
import pytest

import _feature_reference as R

# ---- a. the comparator ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("shape", R.all_shapes(), ids=lambda s: "%dx%dx%d" % s)
def test_float64_dot_stays_within_the_bound(shape):
    """The reference alone passes: integers come out exact, Gaussian data within the bound (prologue 0, epilogue 0)."""
    n_rows, ka, nw = shape
    A, W, exact = R.integer_data(shape)
    assert np.array_equal(R.emulate(A, ka, ka, None, 1.0, W, 0, 0), exact.astype(np.float64))
    rng = np.random.RandomState(ka + nw)
    A, W = rng.standard_normal(A.shape), rng.standard_normal(W.shape)
    worst = R.check("np.dot", R.emulate(A, ka, ka, None, 1.0, W, 0, 0), A, ka, ka, None, 1.0, W, 0, 0)
    assert worst > 0 or ka == 1  # a bound nothing ever approaches would check nothing: some rounding must show


@pytest.mark.parametrize("shape", R.PAIR_SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("epi", R.EPILOGUES)
@pytest.mark.parametrize("pro", R.PROLOGUES)
def test_float64_pairs_stay_within_the_bound(shape, pro, epi):
    n_rows, ka, nw = shape
    A, P, pscale, W = R.pair_data(shape, pro, epi)
    got = R.emulate(A, ka, ka, P, pscale, W, pro, epi)
    assert np.all(np.isfinite(got))
    R.check("np.dot", got, A, ka, ka, P, pscale, W, pro, epi)
    acc, _, S = R.ref_product(A, ka, ka, P, pscale, W, pro, epi)
    if epi == 1:
        assert np.all(got[:, ::3] == np.log(R.EPS)) and np.all(acc[:, 1] > 0)  # the substitution ran, the rest is a real log
    if epi == 2:
        assert float(np.max(np.abs(acc))) <= 30
    if epi == 3:
        neg = acc < -((ka + 8) * R.U) * S
        assert neg.any() and np.all(got[neg] == 0.0) and (acc > 0).any()


def test_strided_rows_are_read_like_the_kernel_reads_them():
    rng = np.random.RandomState(3)
    n_rows, ka, lda = 5, 7, 11
    buf = np.full(n_rows * lda, np.nan)
    A = rng.standard_normal((n_rows, ka))
    for f in range(n_rows):
        buf[f * lda:f * lda + ka] = A[f]
    W = rng.standard_normal((ka, 3))
    for flat in (buf, buf[:(n_rows - 1) * lda + ka]):
        acc, out, S = R.ref_product(flat, ka, lda, None, 1.0, W, 0, 0)
        assert acc.shape == (n_rows, 3) and np.array_equal(acc, R.ref_product(A, ka, ka, None, 1.0, W, 0, 0)[0])
        assert np.array_equal(R.emulate(flat, ka, lda, None, 1.0, W, 0, 0), np.dot(A, W))


MUTATIONS = [
    ("term", 0, 0, ("term", 70, 20)),       # one k term of one row
    ("term-last-k", 0, 0, ("term", 128, 32)),  # the single term of the last, padded strip, in the last row
    ("strip", 0, 0, ("strip", 1)),
    ("strip", 2, 0, ("strip", 0)),
    ("column", 0, 0, ("column", 63)),       # the last column of the first 64-column block takes the next block's first
    ("rows", 0, 0, ("rows", 100)),
    ("rows", 1, 3, ("rows", 0)),
    ("no_eps", 1, 1, ("no_eps",)),
    ("no_eps", 0, 1, ("no_eps",)),
]


@pytest.mark.parametrize("name,pro,epi,mutation", MUTATIONS, ids=["%s-p%de%d" % m[:3] for m in MUTATIONS])
def test_comparator_rejects_a_wrong_product(name, pro, epi, mutation):
    n_rows, ka, nw = R.CENTRE
    A, P, pscale, W = R.pair_data(R.CENTRE, pro, epi)
    acc, out, S = R.ref_product(A, ka, ka, P, pscale, W, pro, epi)
    bnd = R.bound(acc, S, ka, epi)
    good, _ = R.compare(R.emulate(A, ka, ka, P, pscale, W, pro, epi), out, bnd)
    bad, at = R.compare(R.emulate(A, ka, ka, P, pscale, W, pro, epi, mutation), out, bnd)
    print("%s: unmutated %.3g, mutated %.3g at %s" % (name, good, bad, at))
    assert good <= 1.0 < bad
    if mutation[0] == "term":
        assert at[0] == mutation[1]      # the comparator names the row that lost its term
    if mutation[0] == "column":
        assert at[1] == mutation[1]
    if mutation[0] == "rows":
        assert at[0] in (mutation[1], mutation[1] + 16)
    with pytest.raises(AssertionError, match="row %d column %d" % at):
        R.check(name, R.emulate(A, ka, ka, P, pscale, W, pro, epi, mutation), A, ka, ka, P, pscale, W, pro, epi)


# ---- b. the host tables ----------------------------------------------------------------------------------------------------
def hz2mel(hz):
    return 2595 * np.log10(1 + hz / 700.)


def mel2hz(mel):
    return 700 * (10 ** (mel / 2595.0) - 1)


def ref_filterbanks(nfilt, nfft, samplerate, lowfreq, highfreq):
    """world/main.py:275-303, loops and all."""
    highfreq = highfreq or samplerate / 2
    edges = np.floor((nfft + 1) * mel2hz(np.linspace(hz2mel(lowfreq), hz2mel(highfreq), nfilt + 2)) / samplerate)
    fbank = np.zeros([nfilt, nfft // 2 + 1])
    for j in range(nfilt):
        for i in range(int(edges[j]), int(edges[j + 1])):
            fbank[j, i] = (i - edges[j]) / (edges[j + 1] - edges[j])
        for i in range(int(edges[j + 1]), int(edges[j + 2])):
            fbank[j, i] = (edges[j + 2] - i) / (edges[j + 2] - edges[j + 1])
    return fbank


def ref_lfbank(spec, prefac=0.97, fs=16000, nfilt=32, lowfreq=0, highfreq=None, dtype=np.float64):
    """world/main.py:305-322.  ``dtype=np.longdouble`` evaluates the product and the log in extended precision (the tables
    stay the float64 ones the reference builds)."""
    from scipy.signal import freqz

    d = spec.shape[1]
    nfft = (d - 1) * 2
    _, h = freqz([1, -prefac], [1], d)
    spec = spec.astype(dtype) * np.abs(h).astype(dtype)
    pspec = dtype(1 / nfft) * np.square(spec)
    fb = ref_filterbanks(nfilt, nfft, fs, lowfreq, highfreq)
    feat = np.dot(pspec, fb.T.astype(dtype))
    feat = np.where(feat == 0, dtype(np.finfo(float).eps), feat)
    return np.log(feat)


def ref_mcep(spec, n0=12, fs=16000, lowhz=0, highhz=8000):
    """world/main.py:324-341."""
    xl = np.log(spec)
    d = spec.shape[1]
    melpoints = np.linspace(hz2mel(lowhz), hz2mel(highhz), d)
    bins = np.floor(((d - 1) * 2 + 1) * mel2hz(melpoints) / fs)
    xml = np.array([np.interp(bins, np.arange(d), s) for s in xl])
    return np.fft.irfft(xml)[:, :n0]


def ref_imcep_log(cepstrum, fft_size):
    """world/main.py:343-357: decode_mcep before its np.exp."""
    n0 = cepstrum.shape[1]
    yc = np.zeros((cepstrum.shape[0], fft_size))
    yc[:, :n0] = cepstrum
    yc[:, :-n0:-1] = yc[:, 1:n0]
    yl = np.fft.rfft(yc).real
    melpoints = np.linspace(hz2mel(0), hz2mel(8000), int(fft_size // 2 + 1))
    bins = np.floor(fft_size * mel2hz(melpoints) / 16000)
    return np.array([np.interp(np.arange(int(fft_size // 2 + 1)), bins, s) for s in yl])


def random_spectrum(n_frames, d, seed):
    """Magnitudes with log spectra uniform in [-12, 3]."""
    return np.exp(np.random.RandomState(seed).uniform(-12.0, 3.0, size=(n_frames, d)))


MCEP_D = (3, 9, 17, 257, 513, 1025, 2049)
N0 = (1, 2, 12, 13, 40, 64, 65)
MCEP_RATES = ((16000, 0, 8000), (8000, 0, 8000), (8000, 0, 4000), (22050, 50, 11025), (48000, 0, 8000), (48000, 0, 24000),
              (96000, 0, 8000))
IMCEP_FFT = (4, 16, 32, 512, 1024, 2048, 4096)
LFBANK_D = (257, 513, 1025, 2049)
NFILT = (20, 32, 40, 64, 65, 80)
LFBANK_ARGS = ((0.97, 16000, 0, None), (0.9, 16000, 100, 6000), (0.97, 48000, 50, 20000))  # prefac, fs, lowfreq, highfreq


@pytest.mark.parametrize("d", MCEP_D)
def test_mcep_matrix_against_interp_and_irfft(d):
    """Measured worst |difference| over the whole grid: 9.8e-15 (NumPy's FFT against a dense cosine product — no kernel in
    it); asserted 1e-13."""
    from world.features import _mcep_matrix

    spec = random_spectrum(5, d, d)
    worst, cases = 0.0, 0
    for n0 in N0:
        if n0 > 2 * (d - 1):
            continue
        for fs, lo, hi in MCEP_RATES:
            got = np.log(spec) @ _mcep_matrix(d, n0, fs, lo, hi).w
            ref = ref_mcep(spec, n0, fs, lo, hi)
            assert got.shape == ref.shape == (5, n0)
            err = float(np.max(np.abs(got - ref)))
            assert err < 1e-13, (d, n0, fs, lo, hi, err)
            worst, cases = max(worst, err), cases + 1
    print("D = %d: %d cases, worst |matrix - interp + irfft| %.3g" % (d, cases, worst))
    assert cases >= 14


def test_mcep_grid_has_the_clamped_warp():
    """(8000, 0, 8000) asks for twice the Nyquist frequency: the warp positions run past the last bin, where np.interp
    returns the last value and the matrix must gather bin D - 1."""
    d = 513
    bins = np.floor(((d - 1) * 2 + 1) * mel2hz(np.linspace(hz2mel(0), hz2mel(8000), d)) / 8000)
    assert bins[-1] > d - 1 and np.sum(bins > d - 1) > 100


@pytest.mark.parametrize("fft_size", IMCEP_FFT)
def test_imcep_matrix_against_rfft_and_interp(fft_size):
    """Measured worst |difference| of the log spectra over the whole grid: 2.9e-13 (sigma-0.5 cepstra; again NumPy's FFT
    against a dense product); asserted 1e-11, the suite's tolerance for log-domain quantities."""
    from world.features import _imcep_matrix

    worst, cases = 0.0, 0
    for n0 in N0:
        if n0 > fft_size // 2:
            continue
        cep = 0.5 * np.random.RandomState(fft_size + n0).standard_normal((5, n0))
        got = cep @ _imcep_matrix(n0, fft_size).w
        ref = ref_imcep_log(cep, fft_size)
        assert got.shape == ref.shape == (5, fft_size // 2 + 1)
        err = float(np.max(np.abs(got - ref)))
        assert err < 1e-11, (fft_size, n0, err)
        worst, cases = max(worst, err), cases + 1
    print("fft_size = %d: %d cases, worst |matrix - rfft + interp| %.3g" % (fft_size, cases, worst))
    assert cases >= 2


@pytest.mark.parametrize("d", LFBANK_D)
def test_lfbank_tables_against_the_filterbank_loops(d):
    """The tables are the reference's own float64 numbers (the filterbank bit for bit), so the two float64 products differ
    by summation order alone: asserted 1e-11 in the log domain, measured 3.6e-15 over this grid."""
    from world.features import _lfbank_tables, get_filterbanks

    spec = random_spectrum(5, d, 7 * d)
    spec[2] = 0.0  # an all-zero frame: every energy is the substituted eps
    worst = 0.0
    for nfilt in NFILT:
        for prefac, fs, lo, hi in LFBANK_ARGS:
            absh, fbt, scale = _lfbank_tables(d, prefac, fs, nfilt, lo, hi)
            assert np.array_equal(fbt.w, ref_filterbanks(nfilt, 2 * (d - 1), fs, lo, hi).T)
            assert np.array_equal(fbt.w, get_filterbanks(nfilt, 2 * (d - 1), fs, lo, hi).T)
            got = R.emulate(spec, d, d, absh, scale, fbt.w, 1, 1)
            ref = ref_lfbank(spec, prefac, fs, nfilt, lo, hi)
            assert got.shape == ref.shape == (5, nfilt) and np.all(np.isfinite(ref))
            assert np.all(got[2] == np.log(np.finfo(float).eps))
            err = float(np.max(np.abs(got - ref)))
            assert err < 1e-11, (d, nfilt, prefac, fs, lo, hi, err)
            worst = max(worst, err)
    print("D = %d: worst |log energy from the tables - reference expression| %.3g" % (d, worst))


WARP_K = (2, 3, 5, 257, 513, 1025, 2049, 4097, 16385)
WARP_FACTORS = (1.0, 1.1, 0.9, 0.5, 2.0, 3.0, 0.25, 1e-3, 50.0, 1 + 1e-12)


def warp_frames(n_frames, k_bins, seed):
    """Finite positive spectra in e^[-20, 5] with one exact zero and one denormal per call."""
    rng = np.random.RandomState(seed)
    s = np.exp(rng.uniform(-20.0, 5.0, size=(n_frames, k_bins)))
    s[n_frames // 2, k_bins // 2] = 0.0
    s[0, k_bins - 1] = 5e-324
    return s


def ref_warp(frames, factor):
    """world/main.py:191-196 on frame-major rows."""
    k = frames.shape[1]
    xp = np.arange(0, k) / k
    return np.array([np.interp(xp ** factor, xp, s) for s in frames])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("k_bins", WARP_K)
def test_warp_tables_with_the_kernels_arithmetic_equal_interp_bit_for_bit(k_bins):
    from world._tables import warp_tables

    frames = warp_frames(3, k_bins, k_bins)
    for factor in WARP_FACTORS:
        j, dx, den = warp_tables(k_bins, factor)
        assert j.dtype == np.int32 and j.min() >= 0 and j.max() <= k_bins - 1
        assert np.all(j[den != 0] <= k_bins - 2)  # what wh_warp_spectrum checks before the kernel reads row[j + 1]
        jn = np.minimum(j.astype(np.int64) + 1, k_bins - 1)
        with np.errstate(divide="ignore", invalid="ignore"):
            lerp = (frames[:, jn] - frames[:, j]) / den * dx + frames[:, j]
        got = np.where(den == 0, frames[:, j], lerp)
        assert np.array_equal(bits(got), bits(ref_warp(frames, factor))), (k_bins, factor)


# ---- the 16-bit PCM conversion of csrc/wh_modify.hip, restated ------------------------------------------------------------
def ref_pcm16(y):
    """(y * 2**15).astype(np.int16) as the reference's platform evaluates it (example/prosody.py:57), restated in int64:
    truncate toward zero, clamp to int32, keep the low 16 bits; NaN -> 0."""
    v = np.asarray(y, dtype=np.float64) * 32768.0
    t = np.clip(np.trunc(np.where(np.isnan(v), 0.0, v)), -2147483648.0, 2147483647.0).astype(np.int64)
    return (t & 0xFFFF).astype(np.uint16).view(np.int16)


def pcm_inputs():
    """What tests/test_hip_modifier_kernels.py converts: k / 32768 and its two FP64 neighbours for 2000 seeded k, the values
    that leave int16, the non-finite ones, and the eight of tests/test_hip_modifiers.py."""
    rng = np.random.RandomState(16)
    k = rng.randint(-32768, 32769, size=2000).astype(np.float64)
    k[:4] = (-32768, 32768, 0, 32767)
    x = k / 32768
    edge = np.array([1.0, 1 + 2.0 ** -15, 2.0, 1e300, np.inf])
    listed = np.array([-1.0, 0.99999, -0.5, 0.0, 3.1e-5, -3.1e-5, 0.25 + 1e-6, -0.25 - 1e-6])  # tests/test_hip_modifiers.py
    return np.concatenate([x, np.nextafter(x, -np.inf), np.nextafter(x, np.inf), edge, -edge, [np.nan, -0.0], listed])


def test_the_pcm_restatement_is_numpys_cast_where_that_is_defined():
    y = pcm_inputs()
    inside = np.abs(y * 32768.0) < 32768  # (beyond int16 the cast is the platform's: the restatement states it)
    assert inside.sum() > 3000
    assert np.array_equal(ref_pcm16(y[inside]), (y[inside] * 2 ** 15).astype(np.int16))
    named = ref_pcm16(np.array([1.0, -1.0, 1 + 2.0 ** -15, -(1 + 2.0 ** -15), 2.0, -2.0, 1e300, -1e300, np.inf, -np.inf, np.nan]))
    assert named.tolist() == [-32768, -32768, -32767, 32767, 0, 0, -1, 0, -1, 0, 0]
