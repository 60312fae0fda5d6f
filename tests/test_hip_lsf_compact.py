"""GPU: compact encodings whose spectrum is kept as line spectral frequencies (BatchEncoding.compact(lsf_order=p),
world/compact.py, world/lsf.py) — at 16 kHz next to the mel-cepstrum, and at 48 kHz, where the mel-cepstrum does not
exist: compact -> to_host -> to_device -> expand -> decode_device."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _batch(fs):
    from conftest import synth_cached

    return [synth_cached(70, fs, 0.3), synth_cached(71, fs, 0.5)]


@pytest.mark.parametrize("fs", [16000, 48000])
def test_lsf_compact_round_trip_decodes(fs, tmp_path):
    """No flag, finite audio, the sample count of the dense decode, the expanded spectrogram equal to ilsf_device of the
    stored rows bit for bit, the aperiodicity the one every other compact path rebuilds (D4C's own rows).  At 48 kHz the
    mel-cepstral compact() refuses, as before."""
    import torch

    from world.batch import WorldBatch
    from world.compact import CompactEncoding
    from world.lsf import ilsf_device

    xs = _batch(fs)
    wb = WorldBatch(0)
    rt = wb.rt
    enc = wb.encode(xs, fs, f0_method="dio", want_coarse=True)
    ce = enc.compact(lsf_order=40)
    assert ce.kind == "lsf" and ce.lsf_order == 40 and ce.mcep is None and ce.spectrogram is None and ce.n0 is None
    assert tuple(ce.lsf.shape) == (enc.batch.total_frames, 41)
    rows = ce.lsf.cpu().numpy()
    assert np.all(np.isfinite(rows)) and np.all(np.diff(rows[:, 1:], axis=1) > 0)
    assert rows[:, 1].min() > 0 and rows[:, -1].max() < np.pi
    host = ce.to_host()
    assert host.rt is None and isinstance(host.lsf, np.ndarray) and host.lsf.tobytes() == rows.tobytes()
    path = str(tmp_path / "lsf.npz")
    host.save_npz(path)
    loaded = CompactEncoding.load_npz(path)
    assert loaded.kind == "lsf" and loaded.lsf_order == 40 and loaded.lsf.tobytes() == rows.tobytes()
    back = loaded.to_device(rt)
    assert torch.equal(back.lsf, ce.lsf)
    full = back.expand(wb)
    with rt.lock, rt.on_stream():
        assert torch.equal(full.spectrogram, ilsf_device(rt, back.lsf, enc.fft_size))
    assert tuple(full.spectrogram.shape) == tuple(enc.spectrogram.shape)
    # the aperiodicity: what the other compact paths rebuild, which is D4C's own
    if fs == 16000:
        other = enc.compact(n0=40).expand(wb)
    else:
        with pytest.raises(ValueError, match="16000"):
            enc.compact(n0=40)
        other = enc.compact(n0=None).expand(wb)
    assert torch.equal(full.aperiodicity, other.aperiodicity) and torch.equal(full.aperiodicity, enc.aperiodicity)
    assert torch.equal(full.f0, enc.f0) and torch.equal(full.vuv, enc.vuv)
    rng = np.random.RandomState(0)
    noise = [rng.randn(2 * len(x)) for x in xs]
    y, y_off = wb.decode_device(full, noise=noise)
    y_dense, off_dense = wb.decode_device(enc, noise=noise)
    assert np.array_equal(np.asarray(y_off), np.asarray(off_dense)) and tuple(y.shape) == tuple(y_dense.shape)
    y = y.cpu().numpy()
    assert np.all(np.isfinite(y)) and np.max(np.abs(y)) > 0
    # (for the record: how far the audio of the order-40 envelope is from the dense one)
    err = np.sqrt(np.mean((y - y_dense.cpu().numpy()) ** 2) / np.mean(y_dense.cpu().numpy() ** 2))
    print("fs %d: relative rms of the LSF decode against the dense one %.3f" % (fs, err))
    assert rt.take_flags() == [0] * 16


def test_plain_dicts_carry_the_kind():
    from world.batch import WorldBatch
    from world.compact import CompactEncoding

    xs = _batch(48000)
    wb = WorldBatch(0)
    ce = wb.encode(xs, 48000, f0_method="dio", want_coarse=True).compact(lsf_order=24)
    dats = ce.to_dicts()
    assert len(dats) == 2 and all("lsf" in d and "mcep" not in d and "spectrogram" not in d for d in dats)
    again = CompactEncoding.from_dicts(dats)
    assert again.kind == "lsf" and again.lsf_order == 24 and again.lsf.tobytes() == ce.lsf.cpu().numpy().tobytes()
    assert wb.rt.take_flags() == [0] * 16
