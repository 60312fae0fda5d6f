"""GPU: analysis under a given contour for a whole batch — World.encode_batch_w_gvn_f0 against World.encode_w_gvn_f0 of every
utterance alone, bit for bit, and WorldBatch.encode_given_f0 against encode_device (which must enqueue what it always
did)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FS, FFT = 16000, 1024
KEYS = ("temporal_positions", "vuv", "f0", "fs", "spectrogram", "aperiodicity", "coarse_ap", "is_requiem")


def _utterances():
    from conftest import synth_cached

    return [synth_cached(70, FS, 0.3), synth_cached(71, FS, 0.5)]


def _grid_sources(xs, hz=(120.0, 210.0)):
    """Constant-voiced contours on the 5 ms analysis grid: both above 3 fs / fft_size = 46.9 Hz (encode_w_gvn_f0's assert)."""
    from world._tables import frame_count, frame_times

    out = []
    for x, f in zip(xs, hz):
        n = frame_count(len(x), FS, 5)
        out.append({"temporal_positions": frame_times(n, 5), "f0": np.full(n, f), "vuv": np.ones(n)})
    return out


def _copy(source):
    return {k: np.array(v) for k, v in source.items()}


def _same(a, b):
    assert sorted(a) == sorted(b) == sorted(KEYS)
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k


def test_batch_equals_every_utterance_alone():
    from world.main import World

    W = World()
    xs = _utterances()
    sources = _grid_sources(xs)
    kept = [_copy(s) for s in sources]
    dats = W.encode_batch_w_gvn_f0(FS, xs, sources, fft_size=FFT)
    assert len(dats) == 2
    for s, k in zip(sources, kept):  # the sources are not modified
        assert all(np.array_equal(s[key], k[key]) for key in k)
    for x, s, d in zip(xs, sources, dats):
        _same(d, W.encode_w_gvn_f0(FS, x, _copy(s), fft_size=FFT))
    with pytest.raises(NotImplementedError):
        W.encode_batch_w_gvn_f0(FS, xs, sources, fft_size=FFT, devices=[0])


def test_sources_on_a_10ms_grid_are_interpolated():
    from world._tables import frame_times
    from world.main import World

    import _regrid_cases as rc

    W = World()
    xs = _utterances()
    grid = _grid_sources(xs)
    sources = []
    for g, f in zip(grid, (120.0, 210.0)):
        n10 = (len(g["f0"]) + 1) // 2 + 1  # one knot beyond the last frame
        sources.append({"temporal_positions": frame_times(n10, 10), "f0": f + np.arange(n10), "vuv": np.ones(n10)})
    dats = W.encode_batch_w_gvn_f0(FS, xs, sources, fft_size=FFT)
    for x, g, s, d in zip(xs, grid, sources, dats):
        tp = g["temporal_positions"]
        j0, j1 = rc.read_knots(s["temporal_positions"], tp)
        voiced = (s["f0"][j0] > 0) & (s["f0"][j1] > 0)
        host = {"temporal_positions": tp.copy(), "vuv": voiced.astype(np.float64),
                "f0": np.where(voiced, np.interp(tp, s["temporal_positions"], s["f0"]), 0.0)}
        assert np.array_equal(d["f0"], host["f0"]) and np.array_equal(d["vuv"], host["vuv"]) and voiced.all()
        ref = W.encode_w_gvn_f0(FS, x, host, fft_size=FFT)
        assert np.array_equal(d["spectrogram"], ref["spectrogram"])
        _same(d, ref)


def test_encode_device_is_unchanged_and_shares_the_tail():
    import torch

    from world.batch import WorldBatch

    wb = WorldBatch(0)
    xs = _utterances()
    batch, x_d, tp_d = wb.upload(xs, FS)
    enc = wb.encode_device(batch, x_d, tp_d, FS, f0_method="dio", want_coarse=True)
    f0_in, vuv_in = enc.f0.clone(), enc.vuv.clone()
    again = wb.encode_given_f0(batch, x_d, tp_d, FS, enc.f0, enc.vuv, want_coarse=True)
    assert torch.equal(enc.f0, f0_in) and torch.equal(enc.vuv, vuv_in)  # the caller's tensors are left alone
    for key in ("temporal_positions", "f0", "vuv", "spectrogram", "aperiodicity", "coarse_ap", "ap_gate"):
        assert torch.equal(getattr(again, key), getattr(enc, key)), key
    assert again.fft_size == enc.fft_size and again.frame_period == enc.frame_period == 5
    assert (again._timebase is not None) == (enc._timebase is not None)
    with pytest.raises(ValueError):
        wb.encode_given_f0(batch, x_d, tp_d, FS, enc.f0[:-1], enc.vuv)
