"""CPU: tests/_specfilter_reference.py, the NumPy statement of wh_spectral_filter's contract, checked on its own — unit
gain returns the recording, a CheapTrick spectrogram without a denominator reproduces the Requiem filter of the oracle
where the two geometries share their windows, the row map is the nearest frame at every rate, kind 'lsf' is kind
'spectrum' on the materialised envelopes, the comparison rejects six mutants of the contract — and the host side of
world/specfilter.py: tables, argument checks, exports."""
import os

import numpy as np
import pytest

import _lsf_reference as lref
import _specfilter_cases as sc
import _specfilter_reference as sref

FS, HOP, N = 22050, 110, 1024


@pytest.fixture(scope="module")
def recording():
    """The first 1.5 s of tests/golden/test-mwm.wav with the oracle's CheapTrick spectrogram under the fixture's DIO contour."""
    from scipy.io import wavfile

    from oracle import envelope

    fs, xi = wavfile.read(os.path.join(os.path.dirname(__file__), "golden", "test-mwm.wav"))
    assert fs == FS
    x = (xi / (2 ** 15 - 1))[:int(1.5 * FS)]
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "golden_mwm.npz"))
    nf = int(len(x) / FS * 1000 / 5) + 1
    tp = np.arange(nf) * 5 / 1000
    spec, _, _ = envelope.cheaptrick_np(x, FS, np.array(g["dio_f0"][:nf]), np.array(g["dio_vuv"][:nf]), tp, want_ps=False)
    return x, np.ascontiguousarray(spec.T), tp


def test_unit_gain_returns_the_recording(recording):
    x = recording[0]
    for hop, n in ((HOP, N), (1, 512), (512, 1024)):
        xs = x[:4000] if hop == 1 else x
        w = sref.n_windows(len(xs), hop)
        y = sref.filter_rows(xs, np.zeros((1, n // 2 + 1)), np.zeros(w, dtype=np.int32), hop, n)
        assert np.max(np.abs(y - xs)) <= 1e-15 * np.max(np.abs(xs)), hop  # (measured: 6.0e-16 at hop 110)
    win = sref.hann(HOP)
    assert np.max(np.abs(win[:HOP - 1] + win[HOP:] - 1.0)) < 1e-15 and abs(win[HOP - 1] - 1.0) < 1e-15


def test_cheaptrick_rows_reproduce_the_requiem_filter(recording):
    """num = the CheapTrick spectrogram, no den, the identity map: the oracle's requiem_filter on the samples that its
    frames 2 .. F-2 and these windows 1 .. F-3 cover alike, [N - H, (F - 3) H)."""
    from oracle import resynth

    x, spec, tp = recording
    f = len(tp)
    wmap = np.minimum(np.arange(sref.n_windows(len(x), HOP)), f - 1)
    y = sref.filter_spectrum(x, spec, None, wmap, HOP, N)
    want = resynth.requiem_filter(x, spec.T, tp, f, FS)
    lo, hi = N - HOP, (f - 3) * HOP
    assert hi - lo > 20000
    assert np.max(np.abs(y[lo:hi] - want[lo:hi])) <= 4e-15 * np.max(np.abs(want))  # (measured: 4.4e-16 absolute)


@pytest.mark.parametrize("fs", [16000, 22050, 44100, 48000])
def test_row_map_is_the_nearest_frame(fs, recording):
    from world import specfilter

    hop = specfilter.default_hop(fs, 5)
    assert hop == {16000: 80, 22050: 110, 44100: 220, 48000: 240}[fs]
    ny = int(1.5 * fs)
    f = int(ny / fs * 1000 / 5) + 1
    got = specfilter.window_map(ny, f, hop, fs, 5)
    assert got.dtype == np.int32 and np.array_equal(got, sref.window_map(ny, f, hop, fs, 5))
    t_frames = np.arange(f) * 0.005
    identity = np.minimum(np.arange(len(got)), f - 1)
    for w in range(len(got)):
        t = (w * hop - 1) / fs
        d = np.abs(t_frames - t)
        # nearest, ties (centres half a period from two frames) to the later frame
        assert d[got[w]] <= d.min() + 1e-12, (fs, w)
    if fs in (16000, 48000):
        assert np.array_equal(got, identity)
    if fs == 22050:
        assert len(recording[0]) == ny
        assert int(np.nonzero(got != identity)[0][0]) == 217


def test_kind_lsf_is_kind_spectrum_on_the_envelopes():
    rng = np.random.RandomState(3)
    for p, n in ((2, 512), (24, 1024), (40, 1024), (64, 2048)):
        k = n // 2 + 1
        num, den = sc.lsf_rows(5, p, rng), sc.lsf_rows(5, p, rng)
        as_radians = lambda r: np.concatenate([r[:, :1], np.arccos(r[:, 1:])], axis=1)  # noqa: E731
        sn, sd = lref.ilsf_rows(as_radians(num), k), lref.ilsf_rows(as_radians(den), k)
        x = rng.randn(700)
        wmap = np.minimum(np.arange(sref.n_windows(700, 80)), 4)
        a = sref.filter_lsf(x, num, den, wmap, 80, n)
        b = sref.filter_spectrum(x, sn, sd, wmap, 80, n)
        assert sref.compare(a, b) == [], p
        a = sref.filter_lsf(x, num, None, wmap, 80, n)
        b = sref.filter_spectrum(x, sn, None, wmap, 80, n)
        assert sref.compare(a, b) == [], p


@pytest.mark.parametrize("mutant", sref.MUTANTS)
def test_the_comparison_rejects_mutants(mutant):
    case = sc.kind_cases()[0]  # ragged three, spectrum with den
    inp = sc.inputs(case)
    want = sc.reference(case)[0]
    fo = inp["frame_off"]
    got = sref.filter_spectrum(inp["x"][0], inp["num"][fo[0]:fo[1]], inp["den"][fo[0]:fo[1]], inp["maps"][0], case.hops[0],
                               case.n, mutant=mutant)
    assert sref.compare(want, want) == []
    assert sref.compare(got, want) != []
    # and a difference of one part in 1e8 on one sample
    off = np.array(want)
    off[len(off) // 2] += 1e-8 * np.max(np.abs(want))
    assert sref.compare(off, want) != []


def test_taps_and_window_samples_outside_are_dropped():
    """A click at the last sample: a clipped window would read it again and again; here it is read where it lies only."""
    x = np.zeros(300)
    x[-1] = 1.0
    w = sref.n_windows(300, 80)
    y = sref.filter_rows(x, np.zeros((1, 513)), np.zeros(w, dtype=np.int32), 80, 1024)
    assert np.max(np.abs(y - x)) < 1e-15


def test_argument_checks_and_tables():
    from world import _hip, specfilter

    assert "wh_spectral_filter" in _hip.SIGNATURES and len(_hip.SIGNATURES["wh_spectral_filter"][1]) == 18
    assert specfilter.n_windows(0, 80) == 0 and specfilter.n_windows(1, 80) == 2 and specfilter.n_windows(80, 80) == 2
    assert specfilter.n_windows(81, 80) == 3 and specfilter.default_hop(16000, 0.01) == 1
    assert len(specfilter.window_map(0, 0, 80, 16000, 5)) == 0
    with pytest.raises(ValueError):
        specfilter.window_map(10, 0, 80, 16000, 5)
    ok = dict(x_off=[0, 200, 200], frame_off=[0, 4, 4], hops=[80, 80], maps=[np.arange(4), np.zeros(0, dtype=np.int32)],
              fft_size=1024, kind="spectrum", cols_num=513)
    assert specfilter.check_filter_args(**ok) == (0, 513)
    assert specfilter.check_filter_args(**dict(ok, kind="lsf", cols_num=41, cols_den=41)) == (1, 40)
    for bad in (dict(hops=[513, 80]), dict(hops=[0, 80]), dict(hops=[80.5, 80]), dict(maps=[np.array([0, 1, 2, 4]), np.zeros(0, int)]),
                dict(maps=[np.array([0, -1, 2, 3]), np.zeros(0, int)]), dict(maps=[np.arange(3), np.zeros(0, int)]),
                dict(maps=[np.arange(4.0), np.zeros(0, int)]), dict(fft_size=1000), dict(fft_size=256), dict(fft_size=8192),
                dict(kind="mcep"), dict(cols_num=257), dict(cols_den=512), dict(kind="lsf", cols_num=40),
                dict(kind="lsf", cols_num=67), dict(kind="lsf", cols_num=41, cols_den=25), dict(x_off=[0, 200]),
                dict(x_off=[0, 200, 100])):
        with pytest.raises(ValueError):
            specfilter.check_filter_args(**dict(ok, **bad))


def test_facade_exports():
    from world import gmm, main, specfilter

    w = main.World()
    assert callable(w.filter_waveform) and callable(w.convert_waveform)
    with pytest.raises(NotImplementedError):
        w.filter_waveform(16000, np.zeros(10), {}, devices=[0])
    with pytest.raises(NotImplementedError):
        w.convert_waveform(16000, np.zeros(10), {}, None, devices=[0])
    assert callable(gmm.convert_waveform) and callable(specfilter.differential_device) and callable(specfilter.filter_device)
