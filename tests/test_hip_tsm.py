"""GPU: world/tsm.py end to end on the first 1.5 s of tests/golden/test-mwm.wav (22.05 kHz: H = 176, D = 110).
stretch_device gives the bits of tests/_wsola_reference.py, shift_pitch_device those of the reference followed by
scipy.signal.resample_poly and the same trim; the World.*_waveform forms give the bits of the device forms;
log_f0_ratio is NumPy's on the encodings' own f0; a shift by ratio 1 returns the recording within 4 ulp of max|x|."""
import os
from fractions import Fraction

import numpy as np
import pytest

import _wsola_cases as wc
import _wsola_reference as wref

pytestmark = pytest.mark.gpu

FS, HOP, TOL = 22050, 176, 110


@pytest.fixture(scope="module")
def rt():
    from world import _hip
    return _hip.Runtime.get()


@pytest.fixture(scope="module")
def speech():
    from scipy.io import wavfile

    fs, xi = wavfile.read(os.path.join(os.path.dirname(__file__), "golden", "test-mwm.wav"))
    assert fs == FS
    x = (xi / (2 ** 15 - 1))[:int(1.5 * FS)]
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module")
def stretched(speech):
    """The reference's (y, delta) per ratio, computed once."""
    out = {}
    for frac in (Fraction(5, 4), Fraction(4, 5)):
        n_out = (2 * len(speech) * frac.numerator + frac.denominator) // (2 * frac.denominator)
        y, d = wref.wsola(speech, n_out, wref.positions(n_out, HOP, frac), HOP, TOL)
        y.setflags(write=False)
        out[frac] = (y, d)
    return out


def _shifted(y, frac, n):
    from scipy.signal import resample_poly

    z = resample_poly(y, frac.denominator, frac.numerator)[:n]
    return np.concatenate([z, np.zeros(n - len(z))])


def test_stretch_and_shift_give_the_reference_bits(rt, speech, stretched):
    from world import tsm

    assert tsm.default_hop_tol(FS) == (HOP, TOL)
    x_d = rt.to_device(np.array(speech))
    for frac, (want, want_d) in stretched.items():
        y_d, y_off = tsm.stretch_device(rt, x_d, [0, len(speech)], FS, float(frac))
        assert y_off.tolist() == [0, len(want)] and wc.same_bits(y_d.cpu().numpy(), want), frac
        pos = tsm.positions(len(want), HOP, float(frac))
        _, _, delta_d = tsm.wsola_device(rt, x_d, [0, len(speech)], [len(want)], [pos], HOP, TOL)
        assert delta_d.cpu().numpy().tobytes() == want_d.tobytes() and np.any(want_d != 0), frac
        z_d, used = tsm.shift_pitch_device(rt, x_d, [0, len(speech)], FS, float(frac))
        assert used == frac and z_d.shape == x_d.shape
        assert wc.same_bits(z_d.cpu().numpy(), _shifted(want, frac, len(speech))), frac
    assert rt.take_flags() == [0] * 16


def test_a_batch_with_a_ratio_per_utterance(rt, speech, stretched):
    """Two utterances at two ratios in one call, in x's layout: each is what it is alone."""
    from world import tsm

    a, b = speech[:20000], speech[9000:33000]
    x_d = rt.to_device(np.concatenate([a, b]))
    x_off = [0, len(a), len(a) + len(b)]
    z_d, used = tsm.shift_pitch_device(rt, x_d, x_off, FS, [1.25, 0.8])
    assert used == [Fraction(5, 4), Fraction(4, 5)] and z_d.shape == x_d.shape
    z = z_d.cpu().numpy()
    for u, (seg, r) in enumerate(((a, 1.25), (b, 0.8))):
        alone, _ = tsm.shift_pitch_device(rt, rt.to_device(np.array(seg)), [0, len(seg)], FS, r)
        assert alone.cpu().numpy().tobytes() == z[x_off[u]:x_off[u + 1]].tobytes(), u
    y_d, y_off = tsm.stretch_device(rt, x_d, x_off, FS, [Fraction(3, 2), 0.5], hop=80, tol=40)
    assert np.diff(y_off).tolist() == [30000, 12000]
    want, _ = wref.wsola(b, 12000, wref.positions(12000, 80, 0.5), 80, 40)
    assert wc.same_bits(y_d.cpu().numpy()[30000:], want)
    with pytest.raises(ValueError):
        tsm.stretch_device(rt, x_d, x_off, FS, [1.25])
    with pytest.raises(ValueError):
        tsm.stretch_device(rt, x_d, x_off, FS, 1.25, hop=2000)
    with pytest.raises(ValueError):
        tsm.wsola_device(rt, x_d, x_off, [100, 100], [np.zeros(4, dtype=np.int64)] * 2, 80, 40)  # (ceil(100 / 80) + 1 = 3 frames)
    assert rt.take_flags() == [0] * 16


def test_numpy_forms_give_the_device_forms(rt, speech, stretched):
    from world import main, tsm

    w = main.World()
    x = speech[:12000]
    x_d = rt.to_device(np.array(x))
    y_d, _ = tsm.stretch_device(rt, x_d, [0, len(x)], FS, 1.25)
    y = w.stretch_waveform(FS, x, 1.25)
    assert isinstance(y, np.ndarray) and y.tobytes() == y_d.cpu().numpy().tobytes() and len(y) == 15000
    z_d, _ = tsm.shift_pitch_device(rt, x_d, [0, len(x)], FS, 0.8)
    z = w.shift_pitch_waveform(FS, x, 0.8)
    assert z.shape == x.shape and z.tobytes() == z_d.cpu().numpy().tobytes()
    for f in (w.stretch_waveform, w.shift_pitch_waveform):
        with pytest.raises(NotImplementedError):
            f(FS, x, 1.25, devices=[0])
        with pytest.raises(ValueError):
            f(FS, np.zeros((2, 100)), 1.25)


def test_shift_by_ratio_one_returns_the_recording(rt, speech):
    from world import tsm

    z_d, used = tsm.shift_pitch_device(rt, rt.to_device(np.array(speech)), [0, len(speech)], FS, 1)
    z = z_d.cpu().numpy()
    worst = float(np.max(np.abs(z - speech)))
    print("tsm: shift by 1: worst |y - x| = %.3g of max|x|" % (worst / np.max(np.abs(speech))))
    assert used == 1 and worst <= 4 * np.spacing(np.max(np.abs(speech)))


def test_log_f0_ratio_is_numpys(rt, speech):
    from world import tsm
    from world.batch import WorldBatch

    wb = WorldBatch(0)
    encs = []
    for x in (speech[15000:26000], speech[22000:]):  # (the recording is voiced from 0.78 s on)
        batch, x_d, tp_d = wb.upload([np.array(x)], FS)
        encs.append(wb.encode_device(batch, x_d, tp_d, FS, f0_method="dio", want_coarse=True))

    def mean_log(e):
        f0, vuv = e.f0.cpu().numpy(), e.vuv.cpu().numpy()
        keep = (vuv != 0) & (f0 > 0)
        assert keep.sum() > 20
        return np.mean(np.log(f0[keep]))

    want = float(np.exp(mean_log(encs[1]) - mean_log(encs[0])))
    got = tsm.log_f0_ratio(encs[0], encs[1])
    # two means of some hundred logarithms of magnitude 5 and one exp: a few units of 2^-52 relative
    assert abs(got - want) <= 1e-13 * want
    ce = [e.compact(lsf_order=24) for e in encs]
    assert tsm.log_f0_ratio(ce[0], ce[1]) == got
    assert abs(tsm.log_f0_ratio(ce[0].to_host(), ce[1].to_host()) - want) <= 1e-13 * want
    assert tsm.log_f0_ratio(encs[0], encs[0]) == 1.0
    wb.rt.take_flags()
