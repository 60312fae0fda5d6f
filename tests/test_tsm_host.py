"""CPU: the host side of world/tsm.py — the position formulas, the fraction handed to the resampler, the argument checks,
the window's partition of unity — and the library's export of wh_wsola."""
from fractions import Fraction

import numpy as np
import pytest

import _wsola_reference as wref
from world import tsm


def test_library_exports_the_entry():
    from world import _hip

    lib = _hip.load_library()
    assert lib.wh_version() >= 122 and hasattr(lib, "wh_wsola") and "wh_wsola" in _hip.SIGNATURES


def test_window_is_a_partition_of_unity():
    for hop in (1, 2, 3, 80, 176, 1024):
        w = tsm.window(hop)
        assert w.dtype == np.float64 and w.shape == (2 * hop - 1,)
        assert w.tobytes() == wref.window(hop).tobytes()
        # the argument pi (j + 1) / H (up to 2 pi) carries two roundings of 2^-53 relative, so each cosine is within
        # 2 pi 2^-52 + 2^-53 and each window value within half of that + 2^-54: the pair sums to 1 within 8 x 2^-52
        assert np.max(np.abs(w[:hop - 1] + w[hop:] - 1.0), initial=0.0) <= 8 * 2 ** -52 and abs(w[hop - 1] - 1.0) <= 2 ** -52
        assert np.all(w > 0)


def test_frame_count_and_positions():
    assert [tsm.n_frames(n, 4) for n in (0, 1, 4, 5, 8, 9)] == [0, 2, 2, 3, 3, 4]
    for hop in (1, 2, 80, 176):
        for n_out in (0, 1, hop, hop + 1, 10 * hop + 3):
            # ratio 1: frame m starts at its own output position m H - H
            p = tsm.positions(n_out, hop, 1)
            assert p.dtype == np.int64 and np.array_equal(p, np.arange(tsm.n_frames(n_out, hop)) * hop - hop)
            for ratio in (0.5, 0.8, 1.25, 1.5, Fraction(5, 4)):
                p = tsm.positions(n_out, hop, ratio)
                m = np.arange(tsm.n_frames(n_out, hop))
                want = [int(np.floor((int(k) * hop - 1.0) / float(ratio) + 0.5)) - (hop - 1) for k in m]
                assert p.tolist() == want and p.tobytes() == wref.positions(n_out, hop, ratio).tobytes()
    for bad in (0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError):
            tsm.positions(100, 10, bad)


def test_positions_from_map():
    hop, n_out = 10, 95
    # one segment of slope 1 / ratio is the uniform stretch
    for ratio in (0.8, 1.25, 2.0):
        p = tsm.positions_from_map(n_out, hop, [0.0, 1000.0], [0.0, 1000.0 / ratio])
        assert np.array_equal(p, tsm.positions(n_out, hop, ratio))
    # two segments: twice as slow up to output sample 40, real time behind it
    p = tsm.positions_from_map(n_out, hop, [0, 40, 100], [0, 20, 80])
    centre = np.arange(tsm.n_frames(n_out, hop)) * hop - 1.0
    want = np.where(centre < 40, centre / 2, 20 + (centre - 40))
    assert np.array_equal(p, (np.floor(want + 0.5) - (hop - 1)).astype(np.int64))
    for out_t, in_t in (([0, 0], [0, 1]), ([0, 2, 1], [0, 1, 2]), ([0], [0]), ([0, 1], [0, 1, 2]), ([0, np.nan], [0, 1])):
        with pytest.raises(ValueError):
            tsm.positions_from_map(n_out, hop, out_t, in_t)


def test_default_hop_and_tolerance():
    assert tsm.default_hop_tol(16000) == (128, 80)
    assert tsm.default_hop_tol(22050) == (176, 110)
    assert tsm.default_hop_tol(48000) == (384, 240)
    assert tsm.default_hop_tol(44100) == (352, 220)
    with pytest.raises(ValueError):
        tsm.default_hop_tol(192000)


def test_as_fraction_and_lengths():
    assert tsm.as_fraction(1.25) == Fraction(5, 4) and tsm.as_fraction(0.8) == Fraction(4, 5)
    assert tsm.as_fraction(1) == Fraction(1) and tsm.as_fraction(Fraction(3, 2)) == Fraction(3, 2)
    assert tsm.as_fraction(2 ** 0.5) == Fraction(2 ** 0.5).limit_denominator(64)
    assert tsm.as_fraction(1.8931).denominator <= 64
    for bad in (0, -1.5, "1.2", None, True, 1e-4):
        with pytest.raises(ValueError):
            tsm.as_fraction(bad)
    assert tsm.stretched_length(33075, Fraction(5, 4)) == 41344 and tsm.stretched_length(33075, 1.25) == 41344
    assert tsm.stretched_length(2, Fraction(5, 4)) == 3 and tsm.stretched_length(10, Fraction(4, 5)) == 8
    assert tsm.stretched_length(0, 1.5) == 0


def test_argument_checks():
    pos = [tsm.positions(100, 10, 0.8), tsm.positions(0, 10, 0.8)]
    x_off, y_off, pos_off, flat = tsm.check_wsola_args([0, 80, 80], [100, 0], pos, 10, 4)
    assert y_off.tolist() == [0, 100, 100] and pos_off.tolist() == [0, 11, 11] and flat.dtype == np.int64 and len(flat) == 11
    good = dict(x_off=[0, 80, 80], y_lengths=[100, 0], positions=pos, hop=10, tol=4)
    bad = {
        "hop 0": dict(hop=0), "hop too large": dict(hop=1025), "hop a float": dict(hop=10.0), "hop a bool": dict(hop=True),
        "tol negative": dict(tol=-1), "tol too large": dict(tol=513),
        "offsets decrease": dict(x_off=[0, 80, 70]), "offsets negative": dict(x_off=[-1, 80, 80]),
        "no offsets": dict(x_off=[], y_lengths=[], positions=[]), "offsets a table": dict(x_off=[[0, 80, 80]]),
        "lengths of another batch": dict(y_lengths=[100]), "negative length": dict(y_lengths=[100, -1]),
        "a bool length": dict(y_lengths=[100, False]), "a fractional length": dict(y_lengths=[100.5, 0]),
        "list of another length": dict(positions=[pos[0][:-1], pos[1]]),
        "float positions": dict(positions=[pos[0].astype(np.float64), pos[1]]),
        "lists of another batch": dict(positions=pos[:1]),
    }
    for name, kw in bad.items():
        with pytest.raises(ValueError):
            tsm.check_wsola_args(**dict(good, **kw))
            pytest.fail(name)
    # the limits themselves are legal
    tsm.check_wsola_args([0, 5], [3], [np.zeros(2, dtype=np.int64)], 1024, 512)
    tsm.check_wsola_args([0, 5], [3], [np.array([2 ** 62, -2 ** 62, 0, 1])], 1, 0)


def test_log_f0_ratio_on_host_encodings():
    class Enc:
        def __init__(self, f0, vuv):
            self.f0, self.vuv = np.asarray(f0, dtype=np.float64), np.asarray(vuv, dtype=np.float64)

    a = Enc([100.0, 0.0, 120.0, 110.0], [1, 0, 1, 1])
    b = Enc([0.0, 200.0, 240.0, 0.0, 220.0, 50.0], [0, 1, 1, 0, 1, 0])
    want = np.exp(np.mean(np.log([200.0, 240.0, 220.0])) - np.mean(np.log([100.0, 120.0, 110.0])))
    assert abs(tsm.log_f0_ratio(a, b) - want) <= 4 * np.spacing(want) and abs(tsm.log_f0_ratio(a, b) - 2.0) < 1e-12
    with pytest.raises(ValueError):
        tsm.log_f0_ratio(a, Enc([0.0, 100.0], [0, 0]))
    with pytest.raises(ValueError):
        tsm.log_f0_ratio(a, object())


def test_recording_checks():
    import types

    import torch

    from world import _hip

    rt = types.SimpleNamespace(torch=torch)
    x = torch.zeros(80, dtype=torch.float64)
    _hip.check_recording(rt, x, [0, 30, 80], "w")
    for name, bad in (("short", x[:79]), ("float32", x.float()), ("strided", torch.zeros(160, dtype=torch.float64)[::2]),
                      ("2-D", x.reshape(1, 80))):
        with pytest.raises(ValueError, match="w: x must be a contiguous float64 tensor of at least 80 samples"):
            _hip.check_recording(rt, bad, [0, 30, 80], "w")
            pytest.fail(name)
    h = _hip.host_recording([1, 2, 3], "w")
    assert h.dtype == np.float64 and h.flags.c_contiguous and h.tolist() == [1.0, 2.0, 3.0]
    with pytest.raises(ValueError, match=r"w: x must be 1-D, got shape \(2, 3\)"):
        _hip.host_recording(np.zeros((2, 3)), "w")
