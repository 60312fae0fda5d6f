"""GPU: compact encodings (world/compact.py) — f0 / vuv, mel-cepstrum and D4C's band aperiodicity, expanded again on the
device by imcep_device and wh_aperiodicity_from_bands.  The rebuilt aperiodicity is D4C's own, bit for bit (both kernels
evaluate world/d4c.py:45-59 through csrc/wh_apbands.h); against the reference it meets the 1e-7 that
tests/test_hip_getters.py applies to the same quantity; the spectrum side reproduces the reference's own 5.23 dB
(test/spectralFeatures.py:34); and encode_compact_batch -> decode_compact_batch gives the samples of the dense flow whose
spectrogram went through encode_mcep / decode_mcep, with no dense tensor crossing PCIe."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _rebuilt(wb, enc):
    from world.d4c import aperiodicity_from_bands_device

    with wb.rt.on_stream():
        return aperiodicity_from_bands_device(wb.rt, enc.coarse_ap, enc.ap_gate, enc.fs, enc.fft_size)


def _classes(enc):
    """(gate-failed, unvoiced, through the bands): frames the F0 stage calls voiced but D4C's gate rejected, frames with
    vuv == 0, frames whose row came from the bands."""
    vuv = enc.vuv.cpu().numpy()
    gate = enc.ap_gate.cpu().numpy()
    assert set(np.unique(gate)) <= {0.0, 1.0}
    assert not ((vuv == 0) & (gate == 1)).any()  # d4c.py:32,70: an unvoiced frame never passes
    return int(((vuv != 0) & (gate == 0)).sum()), int((vuv == 0).sum()), int((gate == 1).sum())


@pytest.mark.parametrize("tag,counts", [("syn16k", (0, 81, 160)), ("syn48k", (0, 14, 87))])
def test_rebuilt_aperiodicity_is_d4cs_own_bitwise(golden, tag, counts):
    """The fixtures' synthetic utterances; at 48 kHz nap = 5, so every segment of the interpolation is walked.  ``counts``:
    (gate-failed, unvoiced, through the bands) frames, read off the reference's own results in the fixtures (dio_vuv and
    bin 0 of d4c_aperiodicity): these clean utterances have no voiced frame that D4C's gate rejects — the ragged batch of
    the next test brings those."""
    import torch

    from world.batch import WorldBatch

    g = golden(tag)
    fs = int(g["fs"])
    wb = WorldBatch(0)
    batch, x_d, tp_d = wb.upload([g["x"]], fs)
    enc = wb.encode_device(batch, x_d, tp_d, fs, f0_method="dio", want_coarse=True)
    got = _classes(enc)
    print("frame classes", tag, got)
    assert got == counts
    assert tuple(enc.coarse_ap.shape) == (batch.total_frames, 1 if fs == 16000 else 5)
    assert torch.equal(_rebuilt(wb, enc), enc.aperiodicity)
    # and the default path is the one it was: same bits without want_coarse, nothing kept
    plain = wb.encode_device(batch, x_d, tp_d, fs, f0_method="dio")
    assert plain.coarse_ap is None and plain.ap_gate is None
    assert torch.equal(plain.aperiodicity, enc.aperiodicity) and torch.equal(plain.spectrogram, enc.spectrogram)
    assert wb.rt.take_flags() == [0] * 16


def test_rebuilt_aperiodicity_of_a_ragged_batch_with_a_silent_utterance():
    import torch

    from world._synthetic import synth_utterance
    from world.batch import WorldBatch

    fs = 16000
    # the third utterance: harmonics below 3.5 kHz plus a band of noise between 4.3 and 7.6 kHz whose gain rises — DIO
    # calls it voiced throughout, D4C's gate (the power below 4 kHz against the power below 7.9 kHz, d4c.py:76-87) rejects
    # the later frames (the signal of tests/test_hip_d4c.py::test_love_train_gate_around_its_threshold)
    rng = np.random.RandomState(12)
    n = int(1.13 * fs)
    t = np.arange(n) / fs
    low = sum(np.sin(2 * np.pi * 140.0 * h * t + 0.3 * h) / h for h in range(1, 25))
    spec = np.fft.rfft(rng.randn(n))
    fr = np.fft.rfftfreq(n, 1 / fs)
    spec[(fr < 4300) | (fr > 7600)] = 0.0
    high = np.fft.irfft(spec, n)
    high *= np.sqrt(np.mean(low ** 2) / np.mean(high ** 2))
    xs = [synth_utterance(21, fs, 0.7), np.zeros(int(0.31 * fs)), 0.2 * (low + np.linspace(0.15, 0.75, n) * high)]
    wb = WorldBatch(0)
    enc = wb.encode(xs, fs, f0_method="dio", want_coarse=True)
    failed, unvoiced, banded = got = _classes(enc)
    print("frame classes ragged", got)
    assert failed >= 1 and unvoiced >= 1 and banded >= 1
    # as measured on an MI355X: 132 voiced frames rejected by the gate (the later part of the noisy utterance), 118
    # unvoiced ones (the silent utterance's 63 among them), 181 through the bands — 431 frames, an odd number, so the
    # batch also ends on the kernel's single-bin tail
    assert got == (132, 118, 181)
    fo = enc.batch.frame_off
    gate = enc.ap_gate.cpu().numpy()
    assert not gate[int(fo[1]):int(fo[2])].any()  # the silent utterance: every row is the constant one
    rebuilt = _rebuilt(wb, enc)
    assert torch.equal(rebuilt, enc.aperiodicity)
    # an output that does not start on a 16-byte boundary takes the scalar-store variant of the kernel: same bits
    from world import _hip
    rt = wb.rt
    nf, k = (int(v) for v in enc.aperiodicity.shape)
    buf = rt.zeros((nf * k + 1,))
    out = buf[1:]
    assert out.data_ptr() % 16 == 8
    with rt.on_stream():
        _hip.check(rt.lib.wh_aperiodicity_from_bands(rt.ctx, rt.stream(), nf, 1, k, float(fs), 3000, rt.ptr(enc.coarse_ap),
                                                     rt.ptr(enc.ap_gate), rt.ptr(out)))
    assert torch.equal(out.view(nf, k), enc.aperiodicity) and float(buf[0]) == 0.0
    assert rt.take_flags() == [0] * 16


@pytest.mark.parametrize("tag", ["16k", "48k"])
def test_expansion_of_the_references_bands_matches_its_dense_aperiodicity(golden, tag):
    """tests/golden/golden_compact.npz (make_compact.py: the unmodified reference).  1e-7 absolute: the tolerance
    tests/test_hip_getters.py applies to this quantity."""
    from world.d4c import aperiodicity_from_coarse

    g = golden("compact")
    fs, fft_size = int(g["fs_" + tag]), int(g["fft_size_" + tag])
    gate = 1.0 - g["failed_" + tag].astype(np.float64)
    got = aperiodicity_from_coarse(g["coarse_" + tag], gate, fs, fft_size)
    assert got.shape == (fft_size // 2 + 1, len(gate))
    err = np.max(np.abs(got[:, g["ap_frames_" + tag]] - g["ap_" + tag]))
    print("max abs error against the reference", tag, err)
    assert err <= 1e-7
    assert np.all(got[:, gate == 0] == 1 - 0.000000000001)
    assert got.max() <= 1.0


def _lsd(ori_spec, syn_spec):
    """test/spectralFeatures.py:12-19, restated."""
    a = ori_spec / np.sqrt(np.mean(ori_spec ** 2, axis=1)).reshape(-1, 1)
    b = syn_spec / np.sqrt(np.mean(syn_spec ** 2, axis=1)).reshape(-1, 1)
    return np.mean(np.mean((20 * np.log10(a) - 20 * np.log10(b)) ** 2, axis=1) ** 0.5)


def test_spectrum_side_is_mcep_then_imcep_and_meets_the_references_distortion(golden):
    import torch
    from scipy.io import wavfile

    from world.batch import WorldBatch
    from world.features import imcep_device, mcep_device

    fs, xi = wavfile.read(os.path.join(GOLDEN, "test-mwm.wav"))
    x = xi / (2 ** 15 - 1)
    wb = WorldBatch(0)
    enc = wb.encode([x], fs, f0_method="harvest", want_coarse=True)
    # the reference's example is a 22.05 kHz recording that its script hands to encode_mcep with the default fs = 16000
    # (test/spectralFeatures.py:21,31-33): compact() refuses to do that silently and does it when told to
    assert fs == 22050 and enc.fft_size == 1024
    with pytest.raises(ValueError, match="16000"):
        enc.compact(n0=40)
    ce = enc.compact(n0=40, mcep_fs=16000)
    assert tuple(ce.mcep.shape) == (enc.batch.total_frames, 40)
    assert ce.nbytes() == enc.batch.total_frames * (40 + 2 + 4) * 8  # two aperiodicity bands at 22.05 kHz
    back = ce.expand(wb)
    with wb.rt.on_stream():
        want = imcep_device(wb.rt, mcep_device(wb.rt, enc.spectrogram, 40), enc.fft_size)  # (fs = 16000: the default)
    assert torch.equal(back.spectrogram, want)
    assert torch.equal(back.aperiodicity, enc.aperiodicity)
    assert back.f0 is ce.f0 and back.vuv is ce.vuv
    got = _lsd(back.spectrogram.cpu().numpy(), enc.spectrogram.cpu().numpy())
    print("log-spectral distortion", got, "reference", float(golden("manifold")["lsd_mcep"]))
    assert abs(got - float(golden("manifold")["lsd_mcep"])) <= 2e-3
    # through the host and a file: the same tensors come back
    host = ce.to_host()
    dev = host.to_device(wb.rt)
    for k in ("temporal_positions", "f0", "vuv", "mcep", "band_ap", "ap_gate"):
        assert torch.equal(getattr(dev, k), getattr(ce, k)), k
    # band aperiodicity alone: every rate
    g = golden("syn48k")
    enc48 = wb.encode([g["x"]], 48000, f0_method="dio", want_coarse=True)
    with pytest.raises(ValueError, match="16000"):
        enc48.compact(n0=40)
    back48 = enc48.compact(n0=None).expand(wb)
    assert back48.spectrogram is enc48.spectrogram and torch.equal(back48.aperiodicity, enc48.aperiodicity)
    with pytest.raises(ValueError, match="want_coarse"):
        wb.encode([g["x"]], 48000, f0_method="dio").compact(n0=None)


@pytest.mark.parametrize("is_requiem", [False, True])
def test_compact_round_trip_decodes_to_the_samples_of_the_dense_flow(is_requiem, monkeypatch):
    from world import _hip, main
    from world._synthetic import synth_utterance
    from world.batch import _Pending

    fs = 16000
    xs = [synth_utterance(31, fs, 0.8), synth_utterance(32, fs, 0.45), synth_utterance(33, fs, 1.1)]
    W = main.World()
    # the comparison batch: the dense flow with the spectrogram through encode_mcep / decode_mcep
    ref = W.encode_batch(fs, xs, is_requiem=is_requiem)
    fft_size = ref[0]._enc.fft_size
    for d in ref:
        spec = np.asarray(d["spectrogram"])
        d["spectrogram"] = W.decode_mcep(W.encode_mcep(spec.T, 40), fft_size).T
    W.decode_batch(ref, seed=7)

    moved = []
    real = _hip.Runtime.to_host

    def counting(self, t, transpose=False):
        moved.append(int(t.numel()) * t.element_size())
        return real(self, t, transpose)

    monkeypatch.setattr(_hip.Runtime, "to_host", counting)
    dats = W.encode_compact_batch(fs, xs, n0=40, is_requiem=is_requiem)
    frames = sum(len(d["f0"]) for d in dats)
    bands = 3 if is_requiem else 2  # Requiem: nap + 2 rows; D4C: one band and the gate
    assert moved == [frames * (3 + 40 + bands) * 8]  # ONE block, the compact tensors and nothing else
    assert set(dats[0]) == {"f0", "vuv", "temporal_positions", "mcep", "coarse_ap", "ap_gate", "fs", "fft_size", "is_requiem"}
    assert all(type(d) is dict and not any(isinstance(v, _Pending) for v in d.values()) for d in dats)
    assert dats[0]["mcep"].shape == (len(dats[0]["f0"]), 40) and dats[0]["coarse_ap"].shape == (bands if is_requiem else 1, len(dats[0]["f0"]))
    del moved[:]
    W.decode_compact_batch(dats, seed=7)
    assert moved == [sum(len(d["out"]) for d in dats) * 8]  # the audio
    for d, r in zip(dats, ref):
        assert np.array_equal(d["f0"], r["f0"]) and np.array_equal(d["vuv"], r["vuv"])
        assert d["out"].shape == r["out"].shape and np.array_equal(d["out"], r["out"])
        assert np.isfinite(d["out"]).all() and np.abs(d["out"]).max() > 1e-3
