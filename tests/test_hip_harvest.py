"""GPU parity: wh_harvest vs the golden fixtures (reference output) and the oracle's intermediates."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tag", ["syn16k", "syn48k"])
def test_harvest_stages_vs_oracle(golden, tag):
    from oracle import pitch_harvest
    from world import _hip, _tables
    from world.harvest import harvest_device

    g = golden(tag)
    fs = int(g["fs"])
    x = g["x"]
    o = pitch_harvest.harvest_np(x, fs, return_aux=True)
    aux = o["aux"]
    rt = _hip.Runtime.get()
    nf = _tables.frame_count(len(x), fs, 5)
    tp = _tables.frame_times(nf, 5)
    batch = rt.make_batch([0, len(x)], [0, nf])
    f0, vuv, dbg = harvest_device(rt, batch, rt.to_device(x), rt.to_device(tp), fs, debug=True)
    y = dbg["y"].cpu().numpy()[: len(aux["y"])]
    assert np.max(np.abs(y - aux["y"])) < 1e-12          # decimation (SciPy filtfilt semantics)
    nb = aux["raw"].shape[0]
    raw = dbg["raw"].cpu().numpy()[: nb * aux["raw"].shape[1]].reshape(nb, -1)
    live_mismatch = np.sum((raw != 0) != (aux["raw"] != 0))
    assert live_mismatch == 0
    assert np.max(np.abs(raw - aux["raw"])) < 1e-6       # Hz; FFT-conv vs direct FIR
    f1 = dbg["f0_1ms"].cpu().numpy()[: len(aux["f0_1ms"])]
    assert np.array_equal(f1 != 0, aux["f0_1ms"] != 0)
    assert np.max(np.abs(f1 - aux["f0_1ms"])) < 1e-6
    assert np.array_equal(vuv.cpu().numpy(), g["harvest_vuv"])
    assert np.max(np.abs(f0.cpu().numpy() - g["harvest_f0"])) < 1e-6
    assert rt.take_flags() == [0] * 16


def test_harvest_mwm_config1(golden):
    """BASELINE config 1 input: test-mwm.wav (22.05 kHz → decimation ratio 3) against the reference's f0."""
    from scipy.io import wavfile

    from world.harvest import harvest

    g = golden("mwm")
    fs, xi = wavfile.read(os.path.join(os.path.dirname(__file__), "golden", "test-mwm.wav"))
    x = xi / (2 ** 15 - 1)
    h = harvest(x, fs)
    assert np.array_equal(h["temporal_positions"], g["tp"])
    assert np.array_equal(h["vuv"], g["vuv"])
    ref = g["f0"]  # after cheaptrick/d4c bookkeeping: 0 where unvoiced
    voiced = g["vuv"] != 0
    assert np.max(np.abs(h["f0"][voiced] - ref[voiced]) / ref[voiced]) < 1e-8


@pytest.mark.parametrize("floor,ceil,period", [(40, 600, 5), (90, 400, 10), (71, 800, 2), (20, 400, 5)])
def test_harvest_other_search_ranges(floor, ceil, period):
    """Non-default f0 range / frame period: the longest refinement window, the band set (and with a 40 Hz floor the
    direct-FIR fallback of the band filters: taps longer than an overlap-save tile allows) all change with them; at a
    20 Hz floor the refinement's transform tables no longer fit LDS (global twiddles, rotation windows)."""
    from oracle import pitch_harvest
    from world._synthetic import synth_utterance
    from world.harvest import harvest

    fs = 16000
    x = synth_utterance(41, fs, 1.6)
    o = pitch_harvest.harvest_np(x, fs, f0_floor=floor, f0_ceil=ceil, frame_period=period)
    d = harvest(x, fs, f0_floor=floor, f0_ceil=ceil, frame_period=period)
    assert np.array_equal(d["temporal_positions"], o["temporal_positions"])
    assert np.array_equal(d["vuv"], o["vuv"])
    assert np.max(np.abs(d["f0"] - o["f0"])) < 1e-6


def test_harvest_ragged_batch_of_short_utterances():
    """24 utterances of 50 to 300 ms in one call: the contour back end's share of the workspace is carved exactly from the
    per-utterance frame counts, and short utterances are where its five regions leave the least room after rounding —
    every utterance of the batch against the oracle run on it alone."""
    from oracle import pitch_harvest
    from world._synthetic import synth_utterance
    from world.batch import WorldBatch
    from world.harvest import harvest_device

    fs = 16000
    src = synth_utterance(41, fs, 1.6)[6000:]  # (voiced from sample 3684 to 16483)
    lengths = [800, 1200, 1600, 2400, 4800]
    ref = {n: pitch_harvest.harvest_np(src[:n], fs) for n in lengths}
    assert len(ref[800]["f0"]) == 11 and np.all(ref[800]["vuv"] == 1)
    xs = [src[:lengths[u % 5]] for u in range(24)]
    wb = WorldBatch()
    batch, x_d, tp_d = wb.upload(xs, fs)
    with wb.rt.on_stream():
        f0_d, vuv_d = harvest_device(wb.rt, batch, x_d, tp_d, fs)
    f0, vuv = f0_d.cpu().numpy(), vuv_d.cpu().numpy()
    assert wb.rt.take_flags() == [0] * 16
    for u, x in enumerate(xs):
        o = ref[len(x)]
        s = slice(int(batch.frame_off[u]), int(batch.frame_off[u + 1]))
        assert np.array_equal(vuv[s], o["vuv"]), u
        assert np.max(np.abs(f0[s] - o["f0"])) < 1e-6, u
