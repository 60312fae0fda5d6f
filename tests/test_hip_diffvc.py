"""GPU: vocoder-free conversion end to end on the first 1.5 s of tests/golden/test-mwm.wav (22.05 kHz: the frame period is
110.25 samples, so the default row map is at work).  Encode with DIO, compact(lsf_order=40), a target whose angles are the
source's times 0.95 (every formant a twentieth lower), the recording filtered by target over source
(world.specfilter.differential_device), the result analysed again under the source's f0: on voiced frames its LSF
envelope must be closer to the target's than half of the source-to-target distortion.  (The NumPy reference with the
oracle's CheapTrick gives 3.81 dB against 16.47 dB on the CPU, a ratio of 0.23.)  Then the fused form against the
materialised envelopes, convert_waveform under an identity model, and the NumPy facade against the device form."""
import os

import numpy as np
import pytest

import _specfilter_reference as sref

pytestmark = pytest.mark.gpu

P, FACTOR, SECONDS = 40, 0.95, 1.5


@pytest.fixture(scope="module")
def chain():
    from scipy.io import wavfile

    from world import specfilter
    from world.batch import WorldBatch

    fs, xi = wavfile.read(os.path.join(os.path.dirname(__file__), "golden", "test-mwm.wav"))
    x = (xi / (2 ** 15 - 1))[:int(SECONDS * fs)]
    wb = WorldBatch(0)
    rt = wb.rt
    batch, x_d, tp_d = wb.upload([x], fs)
    enc = wb.encode_device(batch, x_d, tp_d, fs, f0_method="dio", want_coarse=True)
    ce = enc.compact(lsf_order=P)
    arrays = dict(ce._tensors())
    rows = ce.lsf.clone()
    rows[:, 1:] *= FACTOR
    arrays["lsf"] = rows
    target = ce._like(rt, arrays, None)
    y_d = specfilter.differential_device(wb, batch, x_d, ce, target)
    assert rt.take_flags() == [0] * 16
    return {"fs": int(fs), "x": x, "wb": wb, "rt": rt, "batch": batch, "x_d": x_d, "tp_d": tp_d, "enc": enc, "ce": ce,
            "target": target, "y_d": y_d}


def test_the_filtered_recording_moves_to_the_target(chain):
    from world import lsf

    rt, wb, enc, ce, target = chain["rt"], chain["wb"], chain["enc"], chain["ce"], chain["target"]
    y = chain["y_d"].cpu().numpy()
    assert y.shape == chain["x"].shape and np.all(np.isfinite(y))
    again = wb.encode_given_f0(chain["batch"], chain["y_d"], chain["tp_d"], chain["fs"], enc.f0, enc.vuv)
    got = lsf.lsf_device(rt, again.spectrogram, P)
    voiced = (enc.vuv.cpu().numpy() > 0.5)
    assert voiced.sum() > 50
    to_target = lsf.distortion_device(rt, got, target.lsf, enc.fft_size).cpu().numpy()[voiced].mean()
    source_to_target = lsf.distortion_device(rt, ce.lsf, target.lsf, enc.fft_size).cpu().numpy()[voiced].mean()
    print("diffvc: %.2f dB to the target against %.2f dB from the source (ratio %.2f)"
          % (to_target, source_to_target, to_target / source_to_target))
    assert to_target < 0.5 * source_to_target
    assert rt.take_flags() == [0] * 16


def test_fused_rows_equal_materialised_envelopes(chain):
    from world import lsf, specfilter

    rt, ce, target, batch = chain["rt"], chain["ce"], chain["target"], chain["batch"]
    num, den = lsf.ilsf_device(rt, target.lsf, ce.fft_size), lsf.ilsf_device(rt, ce.lsf, ce.fft_size)
    want = specfilter.filter_device(rt, chain["x_d"], batch.x_off, chain["fs"], 5, ce.fft_size, num, den,
                                    frame_off=batch.frame_off).cpu().numpy()
    got = chain["y_d"].cpu().numpy()
    print("diffvc: fused against materialised: relative RMS %.3g, worst sample / max|y| %.3g" % sref.errors(got, want))
    assert sref.compare(got, want) == []
    # and both against the NumPy statement of the contract
    wmap = sref.window_map(len(got), ce.total_frames, 110, chain["fs"], 5)
    assert np.any(wmap != np.minimum(np.arange(len(wmap)), ce.total_frames - 1))
    ref = sref.filter_spectrum(chain["x"], num.cpu().numpy(), den.cpu().numpy(), wmap, 110, ce.fft_size)
    assert sref.compare(want, ref) == []


def test_convert_waveform_under_an_identity_model(chain):
    """A one-component model fitted on (ce, ce) converts every row to itself up to its regularisation, so the filter is
    all but the unit gain.  The bound: per window ||r_w - seg_w|| <= max_k |G[k] - 1| ||seg_w||; a sample lies in at most
    ceil(N / H) responses and sum_w ||seg_w||^2 <= ||x||^2 (win[j]^2 + win[j + H]^2 <= 1), so by Cauchy-Schwarz
    ||y - x|| <= sqrt(ceil(N / H)) max |G - 1| ||x||, with G from the reference on the converted rows the model gave."""
    import torch

    from world import gmm, specfilter

    rt, wb, ce, batch = chain["rt"], chain["wb"], chain["ce"], chain["batch"]
    model, _ = gmm.fit_compact(ce, ce, ce.align(ce), 1, n_iter=2, reg_covar=1e-10)
    y_d, conv = gmm.convert_waveform(wb, batch, chain["x_d"], ce, model)
    assert conv.kind == "lsf" and torch.equal(conv.lsf[:, 0], ce.lsf[:, 0])
    assert torch.equal(y_d, specfilter.differential_device(wb, batch, chain["x_d"], ce, conv))
    cos_rows = lambda t: np.concatenate([t[:, :1], np.cos(t[:, 1:])], axis=1)  # noqa: E731
    h = sref.gain_lsf(cos_rows(conv.lsf.cpu().numpy()), ce.fft_size // 2 + 1, cos_rows(ce.lsf.cpu().numpy()))
    g_max = float(np.max(np.abs(sref.min_phase(h, ce.fft_size) - 1.0)))
    x, y = chain["x"], y_d.cpu().numpy()
    rel = float(np.sqrt(np.sum((y - x) ** 2) / np.sum(x ** 2)))
    bound = np.sqrt(np.ceil(ce.fft_size / 110)) * g_max + sref.RMS_BOUND
    print("diffvc: identity model: ||y - x|| / ||x|| %.3g, bound %.3g (max |G - 1| %.3g)" % (rel, bound, g_max))
    assert g_max < 0.05 and rel <= bound
    assert rel <= 8 * 7.1e-7  # (measured on an MI355X: 7.1e-7, what reg_covar = 1e-10 leaves of the identity)
    assert rt.take_flags() == [0] * 16


def test_numpy_facade_agrees_with_the_device_form(chain):
    from world import main, specfilter

    rt, enc, batch = chain["rt"], chain["enc"], chain["batch"]
    dat = enc.to_dicts()[0]
    other = dict(dat)
    other["spectrogram"] = np.ascontiguousarray(np.roll(np.asarray(dat["spectrogram"]), 3, axis=0))  # every bin three up
    w = main.World()
    got = w.filter_waveform(chain["fs"], chain["x"], other, dat)
    num = rt.to_device(other["spectrogram"]).transpose(0, 1).contiguous()
    want = specfilter.filter_device(rt, chain["x_d"], batch.x_off, chain["fs"], 5, enc.fft_size, num, enc.spectrogram,
                                    frame_off=batch.frame_off).cpu().numpy()
    assert got.shape == want.shape and sref.compare(got, want) == []
    alone = w.filter_waveform(chain["fs"], chain["x"], dat)
    assert alone.shape == want.shape and np.all(np.isfinite(alone))
    with pytest.raises(ValueError):
        specfilter.differential_device(chain["wb"], batch, chain["x_d"], chain["ce"], enc)
    with pytest.raises(ValueError):
        specfilter.differential_device(chain["wb"], batch, chain["x_d"], chain["ce"], enc.compact(lsf_order=24))


def test_every_form_of_source_and_target(chain):
    """differential_device on two BatchEncodings and on two mel-cepstral CompactEncodings is filter_device on their
    spectrograms, bit for bit."""
    import torch

    from world import lsf, specfilter
    from world._synthetic import synth_utterance
    from world.batch import BatchEncoding

    rt, wb, enc, batch = chain["rt"], chain["wb"], chain["enc"], chain["batch"]
    spec2 = lsf.ilsf_device(rt, chain["target"].lsf, enc.fft_size)
    enc2 = BatchEncoding(rt, enc.batch, enc.fs, enc.temporal_positions, enc.f0, enc.vuv, spec2, enc.aperiodicity, enc.fft_size,
                         False, 5)
    got = specfilter.differential_device(wb, batch, chain["x_d"], enc, enc2)
    want = specfilter.filter_device(rt, chain["x_d"], batch.x_off, chain["fs"], 5, enc.fft_size, spec2, enc.spectrogram,
                                    frame_off=batch.frame_off)
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    # mel-cepstra exist at 16 kHz only: a synthetic utterance
    fs = 16000
    b16, x16, tp16 = wb.upload([synth_utterance(80, fs, 0.5), synth_utterance(81, fs, 0.3)], fs)
    e16 = wb.encode_device(b16, x16, tp16, fs, f0_method="dio", want_coarse=True)
    ce = e16.compact(n0=24)
    arrays = dict(ce._tensors())
    mc = ce.mcep.clone()
    mc[:, 1:] *= 0.9
    arrays["mcep"] = mc
    tgt = ce._like(rt, arrays, None)
    got = specfilter.differential_device(wb, b16, x16, ce, tgt)
    want = specfilter.filter_device(rt, x16, b16.x_off, fs, 5, ce.fft_size, tgt.expand(wb).spectrogram, ce.expand(wb).spectrogram,
                                    frame_off=b16.frame_off)
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    assert float((got - x16).abs().max()) > 1e-3 * float(x16.abs().max())  # (a gain that does something)
    assert rt.take_flags() == [0] * 16


def test_world_convert_waveform_is_the_device_route(chain):
    """World.convert_waveform on the encode() dict against world.gmm.convert_waveform on the resident encoding, under a
    model that moves the source towards the target (one component fitted on the pair)."""
    from world import gmm, main

    rt, wb, ce, batch = chain["rt"], chain["wb"], chain["ce"], chain["batch"]
    model, _ = gmm.fit_compact(ce, chain["target"], ce.align(chain["target"]), 1, n_iter=2)
    y_d, conv = gmm.convert_waveform(wb, batch, chain["x_d"], ce, model)
    want = y_d.cpu().numpy()
    assert float(np.max(np.abs(want - chain["x"]))) > 1e-3 * float(np.max(np.abs(chain["x"])))
    got = main.World().convert_waveform(chain["fs"], chain["x"], chain["enc"].to_dicts()[0], model)
    print("diffvc: World.convert_waveform against the device route: relative RMS %.3g, worst sample / max|y| %.3g"
          % sref.errors(got, want))
    assert got.shape == want.shape and sref.compare(got, want) == []
    assert rt.take_flags() == [0] * 16
