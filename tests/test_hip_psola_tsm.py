"""GPU: world/psola.py end to end on synth_utterance(40, 16000, 1.0) and the first 1.5 s of tests/golden/test-mwm.wav
(22.05 kHz).  The tracks built on the device equal period_track / source_map; modify_device at pitch 5/4 and 4/5 moves the
median f0 of the re-encoded output by the asked ratio and leaves the CheapTrick envelope nearer to the input's than
world.tsm.shift_pitch_device does; a rising contour is followed; duration = 1.25 gives round(1.25 n) samples; the
World.*_waveform forms give the bits of the device forms.

The margins are set from the reference, not from the code under test: tests/_psola_reference.py on
the oracle's DIO tracks, re-analysed by the oracle's DIO on the CPU.  One margin per signal and kind of check, each the
reference's greatest deviation of that kind on that signal plus the spread of its deviations there:
    ratio    |median f0_out / f0_in - asked| at 5/4 and 4/5: 0.00018 and 0.00030 at 16 kHz -> 0.00030 + 0.00013 = 0.00044;
             0.00865 and 0.00892 at 22.05 kHz -> 0.00892 + 0.00027 = 0.0092.
    contour  |median f0_out / target - 1| over all frames, over the first third and over the last third of the frames voiced
             before and after: 0.0008, 0.0008 and 0.0003 at 16 kHz -> 0.0008 + 0.0005 = 0.0013; 0.0111, 0.0311 and 0.0101 at
             22.05 kHz -> 0.0311 + 0.0210 = 0.0521.  The thirds tell a followed contour from an ignored one: the same
             reference with the recording left as it is gives 1.0230 and 0.9333 (16 kHz) and 0.8560 and 0.8052 (22.05 kHz)
             in the thirds, with the target flattened to its median 1.1361 / 0.8918 and 1.0170 / 0.9434, with half the slope
             1.0723 / 0.9480 and 0.9335 / 0.9183 — each outside its margin in at least one third.
The medians are taken over the frames voiced before and after, which must be at least 85 % of the input's voiced frames,
the share tests/test_wsola_reference_host.py asks of the pitch figures there (the reference keeps 160 to 163 of 164 and
110 or 111 of 112)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MARGINS = {"synth": {"ratio": 0.00044, "contour": 0.0013}, "speech": {"ratio": 0.0092, "contour": 0.0521}}
RATIOS = (1.25, 0.8)


@pytest.fixture(scope="module")
def wb():
    from world.batch import WorldBatch
    return WorldBatch(0)


def _signal(name):
    if name == "synth":
        from world._synthetic import synth_utterance
        return 16000, np.ascontiguousarray(synth_utterance(40, 16000, 1.0), dtype=np.float64)
    from scipy.io import wavfile
    fs, xi = wavfile.read(os.path.join(os.path.dirname(__file__), "golden", "test-mwm.wav"))
    return fs, np.ascontiguousarray((xi / (2 ** 15 - 1))[:int(1.5 * fs)])


def _tracks(enc):
    f0, vuv, tp = (t.cpu().numpy() for t in (enc.f0, enc.vuv, enc.temporal_positions))
    return f0, (vuv > 0.5) & (f0 > 0), tp


def _contour(f0, voiced, tp):
    """A target rising linearly from 0.8 to 1.25 times the recording's median f0 over the utterance."""
    return np.where(voiced, float(np.median(f0[voiced])) * (0.8 + 0.45 * tp / tp[-1]), 0.0)


def _lsd(wb, enc_in, enc_out, both):
    a, b = enc_in.spectrogram[:len(both)].cpu().numpy()[both], enc_out.spectrogram[:len(both)].cpu().numpy()[both]
    return float(np.mean(np.sqrt(np.mean((10 * np.log10(b / a)) ** 2, axis=1))))


@pytest.fixture(scope="module", params=["synth", "speech"])
def run(request, wb):
    """Everything the tests below read of one signal, computed once."""
    from world import psola, tsm

    rt = wb.rt
    fs, x = _signal(request.param)
    enc = wb.encode([x], fs, f0_method="dio")
    f_in, v_in, tp = _tracks(enc)
    x_d, x_off = rt.to_device(x), [0, len(x)]
    out = {"name": request.param, "fs": fs, "x": x, "enc": enc, "f_in": f_in, "v_in": v_in, "x_d": x_d, "ratio": {}}
    for r in RATIOS:
        y_d, y_off = psola.modify_device(rt, x_d, x_off, fs, enc, pitch=r)
        z_d, _ = tsm.shift_pitch_device(rt, x_d, x_off, fs, r)
        assert y_off.tolist() == x_off
        fig = {"y": y_d.cpu().numpy()}
        for key, w_d in (("psola", y_d), ("wsola", z_d)):
            e = wb.encode([w_d.cpu().numpy()], fs, f0_method="dio")
            f_out, v_out, _ = _tracks(e)
            both = v_in & v_out
            fig[key] = (float(np.median(f_out[both] / f_in[both])), int(both.sum()), _lsd(wb, enc, e, both))
        out["ratio"][r] = fig
    target = _contour(f_in, v_in, tp)
    y_d, _ = psola.modify_device(rt, x_d, x_off, fs, enc, f0=rt.to_device(target))
    f_out, v_out, _ = _tracks(wb.encode([y_d.cpu().numpy()], fs, f0_method="dio"))
    both = v_in & v_out
    out["contour"] = (f_out[both] / target[both], int(both.sum()), target, y_d.cpu().numpy())
    assert rt.take_flags() == [0] * 16
    return out


def test_device_tracks_equal_the_host_functions(wb):
    from world import psola

    rt = wb.rt
    for name in ("synth", "speech"):
        fs, x = _signal(name)
        xs = [x[:len(x) // 2 + 7], x[len(x) // 3:], x[:0]]
        enc = wb.encode(xs[:2], fs, f0_method="dio")
        fo = np.asarray(enc.batch.frame_off)
        f0, vuv, tp = (t.cpu().numpy() for t in (enc.f0, enc.vuv, enc.temporal_positions))
        x_off = np.concatenate([[0], np.cumsum([len(v) for v in xs[:2]])])
        p = psola.default_params(fs)
        for pitch, duration in ((1.25, 1.0), ([0.8, 1.25], [1.25, 0.5]), (1.0, 2.0)):
            n_out, per_a, per_s, src, used = psola.tracks_device(rt, x_off, fs, enc, pitch=pitch, duration=duration)
            assert used == p
            pl, dl = ([v] * 2 if np.ndim(v) == 0 else v for v in (pitch, duration))
            want = {"a": [], "s": [], "src": []}
            for u in range(2):
                s = slice(fo[u], fo[u + 1])
                n = len(xs[u])
                assert n_out[u] == int(np.floor(dl[u] * n + 0.5))
                want["a"].append(psola.period_track(tp[s], f0[s], vuv[s], fs, n, p.grid, pmin=p.pmin))
                want["s"].append(psola.period_track(tp[s], f0[s] * pl[u], vuv[s], fs, n_out[u], p.grid, time_map=dl[u], pmin=p.pmin))
                want["src"].append(psola.source_map(n_out[u], p.grid, dl[u]))
            assert per_a.dtype == rt.torch.int32 and per_s.dtype == rt.torch.int32 and src.dtype == rt.torch.int64
            assert np.array_equal(per_a.cpu().numpy(), np.concatenate(want["a"])), (name, pitch, duration)
            assert np.array_equal(per_s.cpu().numpy(), np.concatenate(want["s"])), (name, pitch, duration)
            assert np.array_equal(src.cpu().numpy(), np.concatenate(want["src"])), (name, pitch, duration)
            assert np.count_nonzero(np.concatenate(want["a"])) > 100
        # a target per frame: a contour rising over each utterance, and a shorter output
        target = np.where((vuv > 0.5) & (f0 > 0), 90.0 + 120.0 * tp / tp.max(), 0.0)
        for duration in (1.0, [0.8, 1.25]):
            n_out, per_a, per_s, src, _ = psola.tracks_device(rt, x_off, fs, enc, f0=rt.to_device(target), duration=duration)
            dl = [duration] * 2 if np.ndim(duration) == 0 else duration
            want = [psola.period_track(tp[fo[u]:fo[u + 1]], target[fo[u]:fo[u + 1]], vuv[fo[u]:fo[u + 1]], fs, n_out[u], p.grid,
                                       time_map=dl[u], pmin=p.pmin) for u in range(2)]
            assert np.array_equal(per_s.cpu().numpy(), np.concatenate(want)), (name, "f0", duration)
            assert len(set(np.concatenate(want).tolist())) > 20
        with pytest.raises(ValueError):
            psola.tracks_device(rt, x_off, fs, enc, f0=rt.to_device(target[:-1]))
    with pytest.raises(ValueError):
        psola.tracks_device(rt, [0, 10], fs, enc)  # (one recording, an encoding of two)
    with pytest.raises(ValueError):
        psola.tracks_device(rt, x_off, fs, enc, pitch=[1.0])
    with pytest.raises(ValueError):
        psola.tracks_device(rt, x_off, fs, enc, duration=0.0)


def test_the_output_is_the_reference_s(run):
    """modify_device is wh_psola on the host functions' tracks: the bits of tests/_psola_reference.py."""
    import _psola_cases as pc
    import _psola_reference as pref
    from world import psola

    fs, x, enc = run["fs"], run["x"], run["enc"]
    f0, vuv, tp = (t.cpu().numpy() for t in (enc.f0, enc.vuv, enc.temporal_positions))
    p = psola.default_params(fs)
    per_a = psola.period_track(tp, f0, vuv, fs, len(x), p.grid, pmin=p.pmin)
    per_s = psola.period_track(tp, f0 * 1.25, vuv, fs, len(x), p.grid, pmin=p.pmin)
    want = pref.psola(x, len(x), per_a, per_s, psola.source_map(len(x), p.grid), pref.Params(*p))["y"]
    assert pc.same_bits(run["ratio"][1.25]["y"], want)


@pytest.mark.parametrize("ratio", RATIOS)
def test_pitch_moves_by_the_asked_ratio_and_the_envelope_stays(run, ratio):
    fig = run["ratio"][ratio]
    (median, both, lsd), (w_median, w_both, w_lsd) = fig["psola"], fig["wsola"]
    print("psola on %s, ratio %.2f: median f0 ratio %.4f over %d frames, envelope distance %.2f dB; shift_pitch_device: %.4f over %d, %.2f dB"
          % (run["name"], ratio, median, both, lsd, w_median, w_both, w_lsd))
    assert both >= 0.85 * int(run["v_in"].sum())
    assert abs(median - ratio) <= MARGINS[run["name"]]["ratio"]
    assert lsd < w_lsd


def test_a_rising_contour_is_followed(run):
    """Frame by frame: the ratio of the output's f0 to the target, over the whole utterance and over its first and last
    third, where a contour that was ignored, flattened, or applied with another slope shows (the figures are in the
    module's docstring)."""
    q, both, target, _ = run["contour"]
    third = len(q) // 3
    figures = {"all": float(np.median(q)), "first third": float(np.median(q[:third])), "last third": float(np.median(q[-third:]))}
    print("psola on %s, contour: median f0 / target %s over %d frames" % (run["name"], ", ".join("%s %.4f" % kv for kv in figures.items()), both))
    assert both >= 0.85 * int(run["v_in"].sum()) and third >= 30
    for where, median in figures.items():
        assert abs(median - 1.0) <= MARGINS[run["name"]]["contour"], (where, median)


def test_the_contour_output_is_the_reference_s(run):
    """modify_device(f0=target) is wh_psola on period_track(tp, target, ..): the bits of tests/_psola_reference.py."""
    import _psola_cases as pc
    import _psola_reference as pref
    from world import psola

    fs, x, enc = run["fs"], run["x"], run["enc"]
    f0, vuv, tp = (t.cpu().numpy() for t in (enc.f0, enc.vuv, enc.temporal_positions))
    _, _, target, y = run["contour"]
    p = psola.default_params(fs)
    per_a = psola.period_track(tp, f0, vuv, fs, len(x), p.grid, pmin=p.pmin)
    per_s = psola.period_track(tp, target, vuv, fs, len(x), p.grid, pmin=p.pmin)
    assert np.count_nonzero(per_s) > 100 and len(set(per_s[per_s > 0].tolist())) > 20  # (a contour, not one period)
    want = pref.psola(x, len(x), per_a, per_s, psola.source_map(len(x), p.grid), pref.Params(*p))["y"]
    assert pc.same_bits(y, want)


def test_duration_and_the_numpy_forms(run, wb):
    from world import main, psola

    rt, fs, x, enc, x_d = wb.rt, run["fs"], run["x"], run["enc"], run["x_d"]
    y_d, y_off = psola.modify_device(rt, x_d, [0, len(x)], fs, enc, duration=1.25)
    assert y_off.tolist() == [0, int(np.floor(1.25 * len(x) + 0.5))] and int(y_d.shape[0]) == y_off[-1]
    w, dat = main.World(), enc.to_dicts()[0]
    y = w.modify_waveform(fs, x, dat, pitch=1.25)
    assert isinstance(y, np.ndarray) and y.tobytes() == run["ratio"][1.25]["y"].tobytes()
    assert w.modify_waveform(fs, x, dat, f0=run["contour"][2]).tobytes() == run["contour"][3].tobytes()
    assert w.modify_waveform(fs, x, dat, duration=1.25).tobytes() == y_d.cpu().numpy().tobytes()
    # the contour as knots: set_pitch_waveform is impose_contour_device
    tp = np.asarray(dat["temporal_positions"])
    knots_t, knots_v = np.array([0.0, tp[-1]]), np.array([120.0, 180.0])
    z_d, _ = psola.impose_contour_device(rt, x_d, [0, len(x)], fs, enc, knots_t, knots_v)
    z = w.set_pitch_waveform(fs, x, dat, knots_t, knots_v)
    assert z.shape == x.shape and z.tobytes() == z_d.cpu().numpy().tobytes() and z.tobytes() != x.tobytes()
    for f, args in ((w.modify_waveform, (fs, x, dat)), (w.set_pitch_waveform, (fs, x, dat, knots_t, knots_v))):
        with pytest.raises(NotImplementedError):
            f(*args, devices=[0])
        with pytest.raises(ValueError):
            f(fs, np.zeros((2, 100)), *args[2:])
    assert rt.take_flags() == [0] * 16
