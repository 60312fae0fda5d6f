"""GPU: polyphase resampling on the device (wh_resample_poly, world.resample, WorldBatch.resample_device /
upload_resampled / encode_resampled, the WAV helpers' resample_to / out_fs).  The bar is scipy.signal.resample_poly bit
for bit (np.array_equal), the step the reference's callers run before the analysis (example/prosody.py:16-19): with
it, everything behind the resampler — Harvest's voicing decisions included — is what it is after resampling on the
host."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

scipy_signal = pytest.importorskip("scipy.signal")

RATES = (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000)


def _random(n, seed):
    return np.random.RandomState(seed).randn(n) * 0.3


def test_drop_in_equals_scipy_for_every_rate_pair_and_short_lengths():
    from world.resample import design, resample_poly

    bad = []
    for fs_in in RATES:
        for fs_out in RATES:
            if fs_in == fs_out:
                continue
            P = design(fs_out, fs_in, 1)["P"]
            for n in (0, 1, 2, 37, max(1, P - 1), 3 * P + 5):
                x = _random(n, n + fs_in % 101 + fs_out % 7)
                got, ref = resample_poly(x, fs_out, fs_in), scipy_signal.resample_poly(x, fs_out, fs_in)
                if got.shape != ref.shape or not np.array_equal(got, ref):
                    bad.append((fs_in, fs_out, n))
    assert bad == []


def test_drop_in_equals_scipy_on_ten_seconds():
    from world._synthetic import synth_utterance
    from world.resample import resample_poly

    bad = []
    for k, fs_in in enumerate(RATES):
        x = synth_utterance(700 + k, fs_in, 10.0) if k % 2 else _random(10 * fs_in, k)
        for fs_out in (16000, 8000, 48000) if fs_in not in (16000, 8000, 48000) else (22050, 96000):
            got, ref = resample_poly(x, fs_out, fs_in), scipy_signal.resample_poly(x, fs_out, fs_in)
            if not np.array_equal(got, ref):
                bad.append((fs_in, fs_out))
    assert bad == []


def test_non_finite_inputs_match_scipy():
    from world.resample import resample_poly

    x = _random(4000, 9)
    x[[0, 5, 1000, 1001, 2500, 3999]] = [np.nan, np.inf, -np.inf, np.inf, np.nan, -np.inf]
    for up, down in ((160, 441), (1, 3), (3, 1), (320, 441), (1280, 147)):
        got, ref = resample_poly(x, up, down), scipy_signal.resample_poly(x, up, down)
        assert np.array_equal(got, ref, equal_nan=True), (up, down)


def test_drop_in_two_dimensional_window_and_integer_input():
    from world.resample import resample_poly

    x = _random(3 * 777, 4).reshape(3, 777)
    assert np.array_equal(resample_poly(x, 2, 3, axis=1), scipy_signal.resample_poly(x, 2, 3, axis=1))
    assert np.array_equal(resample_poly(x.T, 2, 3, axis=0), scipy_signal.resample_poly(x.T, 2, 3, axis=0))
    fir = scipy_signal.firwin(47, 0.2)
    assert np.array_equal(resample_poly(x[0], 5, 2, window=fir), scipy_signal.resample_poly(x[0], 5, 2, window=fir))
    assert np.array_equal(resample_poly(x[1], 3, 7, window=('hamming',)),
                          scipy_signal.resample_poly(x[1], 3, 7, window=('hamming',)))
    pcm = (x[2] * 20000).astype(np.int16)
    assert np.array_equal(resample_poly(pcm, 160, 441), scipy_signal.resample_poly(pcm, 160, 441))


def _mixed():
    from world._synthetic import synth_utterance

    rates = (44100, 48000, 22050, 24000, 8000, 96000)
    xs, fss = [], []
    for u in range(12):
        fs = rates[u % 6]
        n = [fs, 37, fs // 3, 1, 2 * fs, 0][u // 2 % 6] if u % 5 else int(1.3 * fs)
        xs.append(synth_utterance(800 + u, fs, max(n, 1) / fs)[:n] if n > 100 else _random(n, u))
        fss.append(fs)
    return xs, fss


def test_mixed_batch_rows_equal_solo_and_scipy_and_repeat():
    from world.batch import WorldBatch
    from world.resample import resample_poly

    xs, fss = _mixed()
    wb = WorldBatch()
    rt = wb.rt
    off = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    x_d = rt.to_device(np.concatenate(xs))
    y1, yo = wb.resample_device(x_d, off, fss, 16000)
    y2, yo2 = wb.resample_device(x_d, off, fss, 16000)
    y1, y2 = y1.cpu().numpy(), y2.cpu().numpy()
    assert np.array_equal(yo, yo2) and np.array_equal(y1, y2)
    for u, (x, fs) in enumerate(zip(xs, fss)):
        ref = scipy_signal.resample_poly(x, 16000, fs)
        row = y1[yo[u]:yo[u + 1]]
        assert np.array_equal(row, ref), u
        assert np.array_equal(row, resample_poly(x, 16000, fs)), u
    assert rt.take_flags() == [0] * 16


def test_guard_bands_stay_untouched_and_poisoned_output_is_overwritten():
    from world import _hip
    from world.resample import resample_device

    rt = _hip.Runtime.get()
    torch = rt.torch
    xs, fss = _mixed()
    off = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    x_d = rt.to_device(np.concatenate(xs))
    ups = [16000 // np.gcd(16000, f) for f in fss]
    downs = [f // np.gcd(16000, f) for f in fss]
    _, yo = resample_device(rt, x_d, off, ups, downs)
    G = 4096
    big = torch.full((int(yo[-1]) + 2 * G,), float("nan"), dtype=torch.float64, device=rt.device)
    resample_device(rt, x_d, off, ups, downs, out=big[G:G + int(yo[-1])])
    b = big.cpu().numpy()
    assert np.all(np.isnan(b[:G])) and np.all(np.isnan(b[-G:]))
    assert np.all(np.isfinite(b[G:-G]))
    want = np.concatenate([scipy_signal.resample_poly(x, 16000, f) for x, f in zip(xs, fss)])
    assert np.array_equal(b[G:-G], want)


def _pcm_set():
    from world._synthetic import synth_utterance

    return [((synth_utterance(900 + i, fs, 1.2 + 0.3 * i) * 20000).astype(np.int16), fs)
            for i, fs in enumerate((44100, 48000, 22050))]


@pytest.mark.parametrize("method", ["harvest", "dio"])
def test_pcm_upload_resampled_encodes_like_host_resampling(method):
    from world.batch import WorldBatch

    items = _pcm_set()
    wb = WorldBatch()
    batch, x_d, tp_d = wb.upload_resampled([p for p, _ in items], [fs for _, fs in items], 16000)
    got = wb.encode_device(batch, x_d, tp_d, 16000, f0_method=method).to_dicts()
    host = [scipy_signal.resample_poly(p / 32767.0, 16000, fs) for p, fs in items]
    assert np.array_equal(x_d.cpu().numpy(), np.concatenate(host))
    ref = WorldBatch().encode(host, 16000, f0_method=method).to_dicts()
    for u in range(len(items)):
        for key in ("f0", "vuv", "spectrogram", "aperiodicity"):
            assert np.array_equal(got[u][key], ref[u][key]), (method, u, key)


def test_asynchronous_harvest_encode_resampled_settles_by_repeating():
    """A 48 kHz clip between 0.4 s of digital silence: resampled, the silence stays exactly zero, and Harvest's crossing
    lists — sized without the host array's flat samples — overflow.  settle_encode repeats the encode with the counted
    capacities, and the result is the encode of the host-resampled audio."""
    from world._synthetic import synth_utterance
    from world.batch import WorldBatch

    fs = 48000
    pad = np.zeros(int(0.4 * fs))
    xs = [np.concatenate([pad, synth_utterance(131, fs, 2.0), pad]), synth_utterance(132, fs, 1.0)]
    wb = WorldBatch()
    repeats = []
    plain = wb.encode_device

    def spy(*a, **kw):
        repeats.append(kw.get("event_caps"))
        return plain(*a, **kw)

    enc = wb.encode_resampled(xs, fs, 16000, f0_method="harvest", check=False)
    wb.encode_device = spy
    try:
        enc = wb.settle_encode(enc)
    finally:
        del wb.encode_device
    assert len(repeats) == 1 and repeats[0] is not None  # the overflow was raised, and the encode repeated
    host = [scipy_signal.resample_poly(x, 16000, fs) for x in xs]
    ref = WorldBatch().encode(host, 16000, f0_method="harvest").to_dicts()
    for u, d in enumerate(enc.to_dicts()):
        for key in ("f0", "vuv", "spectrogram", "aperiodicity"):
            assert np.array_equal(d[key], ref[u][key]), (u, key)


def test_swipe_encode_resampled_runs_on_swipes_grid():
    from world.batch import WorldBatch

    items = _pcm_set()
    wb = WorldBatch()
    got = wb.encode_resampled([p for p, _ in items], [fs for _, fs in items], 16000, f0_method="swipe").to_dicts()
    host = [scipy_signal.resample_poly(p / 32767.0, 16000, fs) for p, fs in items]
    ref = WorldBatch().encode(host, 16000, f0_method="swipe").to_dicts()
    for u in range(len(items)):
        for key in ("temporal_positions", "f0", "vuv", "spectrogram", "aperiodicity"):
            assert np.array_equal(got[u][key], ref[u][key]), (u, key)


def test_wav_round_trip_at_mixed_rates(tmp_path):
    from scipy.io import wavfile

    from world.batch import WorldBatch
    from world.wavio import encode_wavs, read_wavs, write_wavs

    items = _pcm_set()
    paths = []
    for i, (p, fs) in enumerate(items):
        paths.append(tmp_path / ("in%d.wav" % i))
        wavfile.write(str(paths[-1]), fs, p)
    with pytest.raises(ValueError):
        read_wavs(paths)
    wb = WorldBatch()
    fs, enc = encode_wavs(paths, world_batch=wb, resample_to=16000, f0_method="dio")
    assert fs == 16000
    y, y_off = wb.decode_device(enc)
    up, up_off = wb.resample_device(y, y_off, 16000, 48000)
    yh, uh = y.cpu().numpy(), up.cpu().numpy()
    for u in range(len(items)):
        ref = scipy_signal.resample_poly(yh[y_off[u]:y_off[u + 1]], 48000, 16000)
        assert np.array_equal(uh[up_off[u]:up_off[u + 1]], ref), u
    outs = [tmp_path / ("out%d.wav" % i) for i in range(len(items))]
    write_wavs(outs, 16000, wb, y, y_off, out_fs=48000)
    for u, p in enumerate(outs):
        r, v = wavfile.read(str(p))
        assert r == 48000 and len(v) == 3 * int(y_off[u + 1] - y_off[u])


def test_offsets_beyond_two_to_the_31():
    from world import _hip
    from world.resample import resample_device

    rt = _hip.Runtime.get()
    torch = rt.torch
    big = (1 << 31) + 12345
    tail = _random(44100, 31)
    x_d = torch.zeros(big + len(tail), dtype=torch.float64, device=rt.device)
    x_d[big:] = torch.from_numpy(tail).to(rt.device)
    off = np.array([0, big, big + len(tail)], dtype=np.int64)
    y_d, yo = resample_device(rt, x_d, off, [1, 160], [3, 441])
    last = y_d[int(yo[1]):int(yo[2])].cpu().numpy()
    first = y_d[:16].cpu().numpy()
    del x_d, y_d
    torch.cuda.empty_cache()
    assert np.array_equal(last, scipy_signal.resample_poly(tail, 160, 441))
    assert np.array_equal(first, np.zeros(16))
    assert rt.take_flags() == [0] * 16


def test_facade_threads_get_their_solo_results():
    from world.resample import resample_poly

    jobs = [(_random(30000 + 1000 * i, 50 + i), r) for i, r in enumerate(((160, 441), (1, 3), (3, 1), (147, 160)))]
    solo = [resample_poly(x, *r) for x, r in jobs]
    got, errs = [[] for _ in jobs], []

    def work(i):
        try:
            for _ in range(5):
                got[i].append(resample_poly(jobs[i][0], *jobs[i][1]))
        except BaseException as e:  # noqa: BLE001
            errs.append(repr(e))

    ts = [threading.Thread(target=work, args=(i,)) for i in range(len(jobs))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert errs == []
    for i in range(len(jobs)):
        assert all(np.array_equal(g, solo[i]) for g in got[i]), i
