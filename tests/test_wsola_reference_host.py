"""CPU: tests/_wsola_reference.py, the NumPy statement of wh_wsola's contract, checked on its own — against the same
contract as scalar loops on tiny inputs, against six mutants that must each be told apart, and by its properties on the
first 1.5 s of tests/golden/test-mwm.wav and on seeded noise: ratio 1 returns the recording with every shift 0, the output
length is exact, a stretch keeps the pitch and stretch + scipy.signal.resample_poly moves it by the ratio (the oracle's DIO).

The mutants of the SUM (fused, pairwise) are told apart where the contract states the order: by the bits of the scores.  A
shift — and through it y — depends on a score's last bits only at a near tie, which neither speech nor noise offers; the
other four mutants are told apart by the outputs, the shifts and y.

The pitch figures of this reference (H = 176, D = 110; median f0_out / f0_in over the frames voiced in both, and those
frames over the source's voiced frames) are printed by test_pitch_figures and recorded in DESIGN section 20."""
import os

import numpy as np
import pytest

import _wsola_reference as wref

FS, HOP, TOL = 22050, 176, 110


@pytest.fixture(scope="module")
def speech():
    from scipy.io import wavfile

    fs, xi = wavfile.read(os.path.join(os.path.dirname(__file__), "golden", "test-mwm.wav"))
    assert fs == FS
    x = (xi / (2 ** 15 - 1))[:int(1.5 * FS)]
    x.setflags(write=False)
    return x


def _stretch(x, ratio, hop=HOP, tol=TOL, mutant=None):
    n_out = int(np.floor(ratio * len(x) + 0.5))
    return wref.wsola(x, n_out, wref.positions(n_out, hop, ratio), hop, tol, mutant)


def test_vector_form_equals_the_scalar_loops():
    rng = np.random.RandomState(1)
    for hop, tol, n, n_out in ((1, 0, 7, 9), (1, 2, 9, 6), (2, 1, 11, 14), (3, 3, 17, 25), (5, 2, 23, 18), (4, 6, 30, 31), (3, 1, 0, 5),
                               (2, 2, 1, 4)):
        for kind in ("noise", "integers"):
            x = rng.randn(n) if kind == "noise" else rng.randint(-2, 3, size=n).astype(np.float64)
            m = wref.n_frames(n_out, hop)
            for pos in (wref.positions(n_out, hop, 0.8), rng.randint(-2 * hop - tol - 3, n + 3, size=m)):
                y, d = wref.wsola(x, n_out, pos, hop, tol)
                ys, ds = wref.wsola_scalar(x, n_out, pos, hop, tol)
                assert d.tobytes() == ds.tobytes() and y.tobytes() == ys.tobytes(), (hop, tol, n, kind)
                assert d[0] == 0 and np.all(np.abs(d) <= tol)


def test_sum_mutants_change_the_scores():
    rng = np.random.RandomState(2)
    t, region = rng.randn(2 * 80 - 1), rng.randn(2 * 80 - 1 + 2 * 40)
    want = wref.scores(t, region, 40)
    for mutant in ("fused_sum", "pairwise_sum"):
        got = wref.scores(t, region, 40, mutant)
        assert np.allclose(got, want, rtol=1e-12, atol=1e-14) and got.tobytes() != want.tobytes(), mutant


def test_choice_and_read_mutants_change_the_outputs(speech):
    # an integer-valued signal of period 5: the scores of shifts 5 apart are the same bits
    x = np.tile(np.array([3.0, -1.0, 2.0, 0.0, -2.0]), 40)
    hop, tol, n_out = 8, 7, 150
    pos = wref.positions(n_out, hop, 1.25) + 2
    y, d = wref.wsola(x, n_out, pos, hop, tol)
    ym, dm = wref.wsola(x, n_out, pos, hop, tol, "ties_lowest_index")
    assert np.all(np.abs(d[3:-3]) <= 2) and d.tobytes() != dm.tobytes()
    # a rising level: without the normalisation the louder candidate wins
    rng = np.random.RandomState(3)
    x = rng.randn(4000) * np.linspace(0.2, 3.0, 4000)
    y, d = _stretch(x, 0.8, 64, 48)
    ym, dm = _stretch(x, 0.8, 64, 48, "no_normalisation")
    assert d.tobytes() != dm.tobytes() and y.tobytes() != ym.tobytes()
    # the template follows the frame as it was TAKEN
    x = speech[8000:16000]
    y, d = _stretch(x, 1.25)
    ym, dm = _stretch(x, 1.25, mutant="template_from_pos")
    assert np.any(d != 0) and d.tobytes() != dm.tobytes() and y.tobytes() != ym.tobytes()
    # reads outside the utterance are 0.0: frame 0 starts H - 1 samples in front of it
    x = rng.randn(500) + 2.0
    y, d = _stretch(x, 1.25, 32, 20)
    ym, dm = _stretch(x, 1.25, 32, 20, "clipped_read")
    assert y.tobytes() != ym.tobytes()
    assert set(wref.MUTANTS) == {"pairwise_sum", "fused_sum", "ties_lowest_index", "no_normalisation", "template_from_pos", "clipped_read"}


def test_ratio_one_returns_the_recording(speech):
    rng = np.random.RandomState(4)
    for name, x in (("speech", speech), ("noise", rng.randn(20000))):
        y, d = _stretch(x, 1.0)
        assert len(y) == len(x) and not np.any(d), name
        worst = np.max(np.abs(y - x))
        print("wsola reference, ratio 1 on %s: %d frames, worst |y - x| = %.3g of max|x|" % (name, len(d), worst / np.max(np.abs(x))))
        assert worst <= 4 * np.spacing(np.max(np.abs(x))), name


def test_output_length_is_exact_and_silence_does_not_move(speech):
    for ratio, n_out in ((1.25, 41344), (0.8, 26460), (1.5, 49613), (0.5, 16538)):
        y, d = _stretch(speech[:33075], ratio, 176, 0)  # (tolerance 0: the geometry alone)
        assert len(y) == n_out == int(np.floor(ratio * 33075 + 0.5)) and len(d) == -(-n_out // 176) + 1 and not np.any(d)
    y, d = wref.wsola(np.zeros(3000), 2400, wref.positions(2400, 80, 0.8), 80, 50)
    assert not np.any(d) and not np.any(y)
    x = np.full(3000, np.nan)
    y, d = wref.wsola(x, 2400, wref.positions(2400, 80, 0.8), 80, 50)
    assert not np.any(d)


def _f0(x):
    from oracle.pitch_dio import dio_np

    r = dio_np(x, FS)
    return np.asarray(r["f0"]), np.asarray(r["vuv"]) > 0.5


def _pitch_figure(src, out, time_ratio):
    """(median f0_out / f0_in over the source frames voiced in both, their share of the source's voiced frames); source
    frame k is compared with output frame round(k time_ratio)."""
    (f_in, v_in), (f_out, v_out) = src, out
    k = np.arange(len(f_in))
    j = np.minimum(np.floor(k * time_ratio + 0.5).astype(np.int64), len(f_out) - 1)
    both = v_in & v_out[j] & (f_in > 0) & (f_out[j] > 0)
    return float(np.median(f_out[j][both] / f_in[both])), int(both.sum()), int(v_in.sum())


def test_pitch_figures(speech):
    """The shifts by 5/4, 4/5 and 3/2 (stretch, then scipy.signal.resample_poly by the inverse ratio, trimmed or padded to the
    input's length) and the pure stretches by 5/4 and 4/5, whose nominal f0 ratio is 1: each median within 1 % of nominal,
    on at least 85 % of the source's voiced frames.  This reference gives (H = 176, D = 110):
        shift 5/4 1.2496 (104 / 112)   shift 4/5 0.8012 (110 / 112)   shift 3/2 1.4990 (105 / 112)
        stretch 5/4 0.9996 (107 / 112)   stretch 4/5 1.0015 (109 / 112)
    that is 0.03 %, 0.15 %, 0.07 %, 0.04 % and 0.15 % off nominal."""
    from scipy.signal import resample_poly

    src = _f0(speech)
    for kind, p, q in (("shift", 5, 4), ("shift", 4, 5), ("shift", 3, 2), ("stretch", 5, 4), ("stretch", 4, 5)):
        y, _ = _stretch(speech, p / q)
        assert len(y) == (2 * len(speech) * p + q) // (2 * q)
        if kind == "shift":
            z = resample_poly(y, q, p)[:len(speech)]
            z = np.concatenate([z, np.zeros(len(speech) - len(z))])
            nominal, time_ratio = p / q, 1.0
        else:
            z, nominal, time_ratio = y, 1.0, p / q
        median, both, voiced = _pitch_figure(src, _f0(z), time_ratio)
        print("wsola reference, %s %d/%d: median f0 ratio %.4f (nominal %.4f, off by %.2f %%), voiced in both %d / %d"
              % (kind, p, q, median, nominal, 100 * abs(median / nominal - 1), both, voiced))
        assert both >= 0.85 * voiced, (kind, p, q, both, voiced)
        assert abs(median / nominal - 1) <= 0.01, (kind, p, q, median)
