"""GPU: wh_interp_contour (csrc/wh_regrid.hip) against np.interp, bit for bit, and the surfaces on top of it:
BatchEncoding.set_pitch_contour and World.set_pitch_contour.  The voiced rule is compared with a NumPy restatement
(tests/_regrid_cases.py: read_knots)."""
import numpy as np
import pytest

import _regrid_cases as rc

pytestmark = pytest.mark.gpu

FS = 16000


def _rt():
    from world import _hip

    return _hip.Runtime.get()


def _frames_and_knots():
    """Utterances of 1, 7 and 401 frames (5 ms grid) with 1, 2 and 1000 knots on a jittered 10 ms grid.  Knots sit on some
    frame times on purpose; the frames of the last utterance start below its first knot, those of the second end above its
    last knot."""
    from world._tables import frame_times

    rng = np.random.RandomState(7)
    tp = [frame_times(1, 5), frame_times(7, 5), frame_times(401, 5)]
    knots = [(np.array([0.25]), np.array([180.0]))]
    knots.append((np.array([0.005, 0.02]), np.array([100.0, 130.0])))  # on frames 1 and 4; frames 5, 6 lie above
    t = 0.0123 + np.arange(1000) * 0.01 + rng.uniform(-0.003, 0.003, 1000)
    on = np.arange(5, 195, 19)
    t[on] = tp[2][2 * on + 3]  # exact hits
    t = np.sort(t)
    assert np.all(np.diff(t) > 0) and tp[2][0] < t[0] and len(np.intersect1d(t, tp[2])) == len(on)
    knots.append((t, 120.0 + 60.0 * rng.rand(1000)))
    return tp, knots


def _voiced_ref(tp, time, value):
    j0, j1 = rc.read_knots(time, tp)
    voiced = (value[j0] > 0) & (value[j1] > 0)
    return np.where(voiced, np.interp(tp, time, value), 0.0), voiced.astype(np.float64)


def test_plain_mode_equals_interp():
    tp, knots = _frames_and_knots()
    got, vuv = rc.contour(_rt(), tp, knots, voiced_rule=False)
    assert vuv is None
    ref = np.concatenate([np.interp(t, kt, kv) for t, (kt, kv) in zip(tp, knots)])
    assert np.array_equal(got, ref)
    assert got[0] == 180.0 and got[1] == 100.0 and got[2] == 100.0 and got[7] == 130.0  # one knot; below, on, above


def test_voiced_rule_equals_numpy_restatement():
    """Voiced and unvoiced stretches, a lone unvoiced knot between voiced ones, an unvoiced first and last knot: no frame
    next to an unvoiced knot gets a value strictly between 0 and the smaller voiced neighbour."""
    from world._tables import frame_times

    rng = np.random.RandomState(8)
    tp = [frame_times(150, 5), frame_times(90, 5)]
    t0 = np.arange(70) * 0.01 + 0.003
    v0 = 150.0 + 40.0 * rng.rand(70)
    v0[0] = v0[-1] = 0.0  # unvoiced first and last knot
    v0[20:31] = 0.0       # an unvoiced stretch
    v0[45] = 0.0          # a lone unvoiced knot
    t1 = np.arange(40) * 0.01  # on every other frame: exact hits on voiced and unvoiced knots
    v1 = np.where(np.arange(40) % 7 < 2, 0.0, 210.0 + rng.rand(40))
    knots = [(t0, v0), (t1, v1)]
    f0, vuv = rc.contour(_rt(), tp, knots, voiced_rule=True)
    ref = [_voiced_ref(t, kt, kv) for t, (kt, kv) in zip(tp, knots)]
    assert np.array_equal(f0, np.concatenate([r[0] for r in ref]))
    assert np.array_equal(vuv, np.concatenate([r[1] for r in ref]))
    assert 0.2 < vuv.mean() < 0.9 and np.array_equal(vuv, (f0 > 0).astype(np.float64))
    lowest = min(v0[v0 > 0].min(), v1[v1 > 0].min())
    assert not np.any((f0 > 0) & (f0 < lowest))
    plain, _ = rc.contour(_rt(), tp, knots, voiced_rule=False)
    assert np.any((plain > 0) & (plain < lowest))  # what the rule is for


def test_entry_refuses_bad_knot_lists():
    rt = _rt()
    from world._tables import frame_times

    tp = [frame_times(5, 5)]
    for kt, msg in (([0.0, 0.0], b"strictly increasing"), ([0.0, np.inf], b"finite"), ([0.1, 0.05], b"strictly increasing")):
        with pytest.raises(Exception):
            rc.contour(rt, tp, [(np.array(kt), np.zeros(2))], voiced_rule=False)
        assert msg in rt.lib.wh_last_error()
    with pytest.raises(Exception):
        rc.contour(rt, tp, [(np.zeros(0), np.zeros(0))], voiced_rule=False)
    assert b"at least one knot" in rt.lib.wh_last_error()


def test_set_pitch_contour_on_an_encoded_batch():
    import torch

    from conftest import synth_cached
    from world.batch import WorldBatch

    wb = WorldBatch(0)
    xs = [synth_cached(60, FS, 0.3), synth_cached(61, FS, 0.5)]
    enc = wb.encode(xs, FS, f0_method="dio")
    other = wb.encode(xs, FS, f0_method="dio")
    assert enc._timebase is not None or not wb.prefetch_timebase
    tp = enc.host_times()
    fo = enc.batch.frame_off
    times = [np.arange(31) * 0.01 + 0.002, np.arange(42) * 0.0125]
    values = [np.where((np.arange(31) > 4) & (np.arange(31) < 25), 140.0 + np.arange(31), 0.0),
              np.where(np.arange(42) % 11 < 8, 230.0 - np.arange(42), 0.0)]
    assert enc.set_pitch_contour(times, values) is enc
    assert enc._timebase is None
    ref = [_voiced_ref(tp[int(fo[u]):int(fo[u + 1])], times[u], values[u]) for u in range(2)]
    f0_h, vuv_h = np.concatenate([r[0] for r in ref]), np.concatenate([r[1] for r in ref])
    assert np.array_equal(enc.f0.cpu().numpy(), f0_h) and np.array_equal(enc.vuv.cpu().numpy(), vuv_h)
    assert 0 < vuv_h.sum() < len(vuv_h)
    # the same contours installed by hand
    other.f0, other.vuv = wb.rt.to_device(f0_h), wb.rt.to_device(vuv_h)
    y, y_off = wb.decode_device(enc, seed=11)
    y2, y_off2 = wb.decode_device(other, seed=11)
    assert np.array_equal(y_off, y_off2) and torch.equal(y, y2) and bool(torch.isfinite(y).all())
    # one pair for every utterance, and the plain mode
    enc.set_pitch_contour(np.array([0.0, 1.0]), np.array([100.0, 200.0]), voiced_rule=False)
    assert np.array_equal(enc.f0.cpu().numpy(), np.interp(tp, [0.0, 1.0], [100.0, 200.0]))
    assert bool((enc.vuv == 1).all())


def test_world_set_pitch_contour_on_a_dict_and_set_pitch_still_raises():
    from world._tables import frame_times
    from world.main import World

    W = World()
    tp = frame_times(61, 5)
    dat = {"temporal_positions": tp, "f0": np.zeros(61), "vuv": np.zeros(61), "fs": FS}
    time = np.array([0.0, 0.1, 0.11, 0.2, 0.4])
    value = np.array([110.0, 150.0, 0.0, 180.0, 90.0])
    assert W.set_pitch_contour(dat, time, value) is dat
    f0, vuv = _voiced_ref(tp, time, value)
    assert np.array_equal(dat["f0"], f0) and np.array_equal(dat["vuv"], vuv) and dat["temporal_positions"] is tp
    assert vuv[20] == 1 and vuv[21] == 0 and vuv[22] == 0 and vuv[40] == 1
    with pytest.raises(NotImplementedError):
        W.set_pitch(dat, time, value)
