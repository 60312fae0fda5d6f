"""GPU: wh_regrid_rows (csrc/wh_regrid.hip) called directly on made tensors, and BatchEncoding.regrid on encoded batches.
Every comparison is np.array_equal / torch.equal against np.interp, per utterance and per bin: value equality, no
tolerance anywhere."""
import numpy as np
import pytest

import _regrid_cases as rc

pytestmark = pytest.mark.gpu

FS = 16000


def _rt():
    from world import _hip

    return _hip.Runtime.get()


@pytest.fixture(scope="module")
def encoded():
    """Two short utterances (0.5 s and 1.2 s: the longer one spans a whole voiced / unvoiced period of the synthetic
    source) encoded once with want_coarse=True; read-only."""
    from conftest import synth_cached
    from world.batch import WorldBatch

    wb = WorldBatch(0)
    enc = wb.encode([synth_cached(50, FS, 0.5), synth_cached(51, FS, 1.2)], FS, f0_method="dio", want_coarse=True)
    return wb, enc


# ---- a. shapes and base pointers -------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_shift", (0, 1))
@pytest.mark.parametrize("out_shift", (0, 1))
@pytest.mark.parametrize("k_bins", rc.SHAPE_K)
def test_shapes_and_bases_equal_interp(k_bins, out_shift, in_shift):
    """K = 1 (per-frame scalars), 2, 5 (band rows), 513, 1025; utterances of 1, 2, 3 and 401 frames in one ragged batch;
    input and output bases on and off a 16-byte boundary (the pair walk and the scalar instantiation, 16-byte and 8-byte
    loads); destination times outside the source range, on source frames and in between."""
    src, dst, rows = rc.shape_case(k_bins)
    got = rc.regrid(_rt(), src, dst, rows, in_shift=in_shift, out_shift=out_shift)
    ref = rc.ref_batch(src, dst, rows)
    assert got.shape == ref.shape and (k_bins % 2 == 0 or got.size % 2 == 1)
    assert np.array_equal(got, ref), "%d elements differ" % np.sum(got != ref)


@pytest.mark.parametrize("k_bins", (1, 5))
def test_positive_rule_equals_numpy_restatement(k_bins):
    """Gates and contours: 0 unless every source value read is > 0, the interpolated value otherwise."""
    src, dst, rows = rc.shape_case(k_bins, seed=1)
    rows = np.where(np.random.RandomState(5).rand(*rows.shape) < 0.3, 0.0, np.abs(rows) + 0.5)
    got = rc.regrid(_rt(), src, dst, rows, positive=True)
    ref = rc.ref_batch(src, dst, rows, positive=True)
    assert 0.1 < np.mean(ref == 0) < 0.9
    assert np.array_equal(got, ref)
    gate = (rows[:, :1] > 0).astype(np.float64)
    got = rc.regrid(_rt(), src, dst, gate, positive=True)
    assert set(np.unique(got)) <= {0.0, 1.0} and np.array_equal(got, rc.ref_batch(src, dst, gate, positive=True))


# ---- b. grid conversions ---------------------------------------------------------------------------------------------
def test_grid_conversions_equal_interp():
    rng = np.random.RandomState(2)
    for name, src, dst in rc.conversion_cases():
        assert all(np.all(np.diff(t) > 0) for t in src)
        rows = rng.rand(sum(len(t) for t in src), 513) + 0.05
        got = rc.regrid(_rt(), src, dst, rows)
        assert np.array_equal(got, rc.ref_batch(src, dst, rows)), name
    counts = {name: [len(d) for d in dst] for name, _, dst in rc.conversion_cases()}
    assert counts["5->10"] == [201, 31] and counts["5->2.5"] == [801, 121] and counts["5->12.5"] == [161, 25]


# ---- c. identity -----------------------------------------------------------------------------------------------------
def test_regrid_to_the_own_period_is_the_identity(encoded):
    import torch

    wb, enc = encoded
    same = enc.regrid(5)
    assert same.batch is not enc.batch and np.array_equal(same.batch.frame_off, enc.batch.frame_off)
    assert np.array_equal(same.tp_host, enc.host_times()) and same.frame_period == 5
    for key in ("temporal_positions", "f0", "vuv", "spectrogram", "aperiodicity", "coarse_ap", "ap_gate"):
        assert torch.equal(getattr(same, key), getattr(enc, key)), key
    assert same.ps_spectrogram is None and same._timebase is None


# ---- d. no leakage, batch invariance -----------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ("AB", "BA"))
def test_no_row_of_another_utterance_is_read(order):
    from world._tables import frame_times
    from world.regrid import destination_times

    rng = np.random.RandomState(3)
    t = {"A": frame_times(7, 5), "B": frame_times(33, 5)}
    rows = {"A": np.full((7, 513), np.nan), "B": rng.rand(33, 513) + 0.05}
    dst = {u: destination_times(t[u], 2.5) for u in "AB"}
    got = rc.regrid(_rt(), [t[u] for u in order], [dst[u] for u in order], np.concatenate([rows[u] for u in order]))
    alone = rc.regrid(_rt(), [t["B"]], [dst["B"]], rows["B"])
    at = order.index("B") * len(dst["A"])
    part = got[at:at + len(dst["B"])]
    assert np.all(np.isfinite(part)) and np.array_equal(part, alone)
    assert np.all(np.isnan(np.delete(got, np.s_[at:at + len(dst["B"])], axis=0)))


# ---- e. the encoding as a whole --------------------------------------------------------------------------------------
def test_regrid_10ms_compacts_expands_and_decodes(encoded):
    import torch

    from world.synthesis import time_axis_params

    wb, enc = encoded
    out = enc.regrid(10)
    fo, fo2 = enc.batch.frame_off, out.batch.frame_off
    tp, tp2 = enc.host_times(), out.tp_host
    assert np.array_equal(out.temporal_positions.cpu().numpy(), tp2) and out.frame_period == 10
    gate, gate2 = enc.ap_gate.cpu().numpy(), out.ap_gate.cpu().numpy()
    spec, spec2 = enc.spectrogram.cpu().numpy(), out.spectrogram.cpu().numpy()
    assert 0 < gate.sum() < len(gate)
    for u in range(enc.n_utt):
        s, d = slice(int(fo[u]), int(fo[u + 1])), slice(int(fo2[u]), int(fo2[u + 1]))
        assert len(tp2[d]) == (len(tp[s]) + 1) // 2 and np.array_equal(tp2[d], np.arange(len(tp2[d])) * 10 / 1000)
        j0, j1 = rc.read_knots(tp[s], tp2[d])
        assert np.array_equal(gate2[d], ((gate[s][j0] > 0) & (gate[s][j1] > 0)).astype(np.float64))
        assert np.array_equal(spec2[d], rc.ref_rows(tp[s], tp2[d], spec[s]))
    ce = out.compact(n0=40)
    back = ce.expand(wb)
    assert tuple(back.spectrogram.shape) == tuple(out.spectrogram.shape)
    assert bool(torch.isfinite(back.spectrogram).all()) and bool(torch.isfinite(back.aperiodicity).all())
    y, y_off = wb.decode_device(out, seed=3)
    assert bool(torch.isfinite(y).all())
    ny = [time_axis_params(tp2[int(fo2[u]):int(fo2[u + 1])], FS)[0] for u in range(out.n_utt)]
    assert [int(v) for v in np.diff(y_off)] == ny
    dicts = out.to_dicts()
    assert dicts[1]["spectrogram"].shape == (513, int(fo2[2] - fo2[1]))
    assert tuple(out.mcep(n0=12).shape) == (int(fo2[-1]), 12)


def test_world_regrid_on_a_dict(encoded):
    from world.main import World

    wb, enc = encoded
    d = enc.to_dicts()[0]
    before = {k: np.array(d[k]) for k in ("temporal_positions", "spectrogram", "aperiodicity")}
    W = World()
    assert W.regrid(d, 2.5) is d
    tp2 = d["temporal_positions"]
    assert len(tp2) == 2 * len(before["temporal_positions"]) - 1
    for key in ("spectrogram", "aperiodicity"):
        assert np.array_equal(d[key].T, rc.ref_rows(before["temporal_positions"], tp2, before[key].T)), key
    assert len(d["f0"]) == len(d["vuv"]) == len(tp2)


# ---- f. what the entry refuses before it launches ---------------------------------------------------------------------
def test_regrid_rows_refuses_bad_arguments():
    rt = _rt()
    a, b = rc.make_batch(rt, [4, 3]), rc.make_batch(rt, [5])
    t = rt.to_device(np.arange(7) * 0.005)
    x, y = rt.zeros((7, 3)), rt.zeros((7, 3))
    call = lambda *args: rt.lib.wh_regrid_rows(rt.ctx, rt.stream(), *args)  # noqa: E731
    assert call(a.handle, b.handle, rt.ptr(t), rt.ptr(t), rt.ptr(x), rt.ptr(y), 3, 0) != 0
    assert b"same utterances" in rt.lib.wh_last_error()
    assert call(a.handle, a.handle, rt.ptr(t), rt.ptr(t), rt.ptr(x), rt.ptr(x), 3, 0) != 0
    assert b"overlap" in rt.lib.wh_last_error()
    assert call(a.handle, a.handle, rt.ptr(t), rt.ptr(t), rt.ptr(x), rt.ptr(y), 0, 0) != 0
    empty = rc.make_batch(rt, [0, 7])
    assert call(empty.handle, a.handle, rt.ptr(t), rt.ptr(t), rt.ptr(x), rt.ptr(y), 3, 0) != 0
    assert b"no source frame" in rt.lib.wh_last_error()
