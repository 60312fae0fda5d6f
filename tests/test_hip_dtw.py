"""GPU: wh_dtw (csrc/wh_dtw.hip) through world.align.align_device on made feature rows, and BatchEncoding.align / warp on
encoded utterances.  Everything the call returns — the accumulated costs, the path, its length, the cost, both frame
maps — is compared with tests/_dtw_reference.py bit for bit; there is no tolerance anywhere."""
import numpy as np
import pytest

import _dtw_cases as dc
import _dtw_reference as ref

pytestmark = pytest.mark.gpu

FS = 16000


def _rt():
    from world import _hip

    return _hip.Runtime.get()


# ---- a. shapes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dc.kernel_cases(), ids=lambda c: c.name)
def test_equals_the_reference_bit_for_bit(case):
    """N and M independently at 1, 2, 3, 63, 64, 65 and around the rows per lane, the columns per staged chunk and the rows
    per strip; d = 1, 2, 24, 39, 64; one row against many; integer features that tie everywhere, across lanes, strips and
    chunks; bands of radius 1, 2 and 17 on unequal lengths and on a one-row side; rows inside a wider tensor."""
    assert dc.compare(dc.run(_rt(), case), case) == []


def test_tile_constants_are_the_kernels():
    from world import align

    assert align.STRIP_ROWS == 64 * align.ROWS_PER_LANE and align.CHUNK_COLS < 64
    s = dc.edge_sizes()
    for t in (align.ROWS_PER_LANE, align.CHUNK_COLS, align.STRIP_ROWS):
        assert {t - 1, t, t + 1, 2 * t + 1} - {0} <= set(s)


# ---- b. the square root and the order of the sum on their own -----------------------------------------------------------
@pytest.mark.parametrize("d", (2, 39))
def test_single_cells_equal_numpy_sqrt_of_the_sequential_sum(d):
    """4096 pairs of one row each: cost = c(0,0) = np.sqrt of the column sum taken in order."""
    from world.align import align_device

    rt = _rt()
    rng = np.random.RandomState(d)
    a, b = rng.randn(4096, d) * np.exp(rng.randn(4096, 1) * 3), rng.randn(4096, d)
    off = np.arange(4097, dtype=np.int64)
    ba, bb = rt.make_batch(np.zeros(4097, dtype=np.int64), off), rt.make_batch(np.zeros(4097, dtype=np.int64), off)
    al = align_device(rt, ba, rt.to_device(a), bb, rt.to_device(b))
    s = np.zeros(4096)
    for k in range(d):
        e = a[:, k] - b[:, k]
        s = s + e * e
    want = np.sqrt(s)
    got = al.cost.cpu().numpy()
    assert got.tobytes() == want.tobytes(), "%d of 4096 differ" % np.sum(got != want)
    assert np.array_equal(al.path_len.cpu().numpy(), np.ones(4096, dtype=np.int64))
    assert np.array_equal(al.path_a.cpu().numpy(), off[:-1]) and np.array_equal(al.map_b2a.cpu().numpy(), off[:-1])
    assert np.array_equal(al.mean_cost().cpu().numpy(), want)


# ---- c. batch invariance ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged():
    return dc.run(_rt(), dc.RAGGED)


def test_ragged_batch_equals_the_reference(ragged):
    assert dc.compare(ragged, dc.RAGGED) == []


def test_a_pair_alone_equals_the_pair_in_the_batch(ragged):
    rt = _rt()
    batch = dc.download(ragged)
    for u in range(len(dc.RAGGED.shapes)):
        alone = dc.download(dc.run(rt, dc.RAGGED, only=u))[0]
        for key in dc.KEYS:
            assert dc.same_bits(alone[key], batch[u][key]), (u, key)


def test_two_runs_of_the_batch_are_equal(ragged):
    again = dc.download(dc.run(_rt(), dc.RAGGED))
    for one, two in zip(dc.download(ragged), again):
        for key in dc.KEYS:
            assert dc.same_bits(one[key], two[key]), key


def test_workspace_groups_do_not_change_a_bit(ragged):
    from world.align import pair_workspace_bytes, plan_groups

    need = [pair_workspace_bytes(n, m) for n, m in dc.RAGGED.shapes]
    limit = (sum(need) + 2) // 3 + max(need) // 4
    na, nb = zip(*dc.RAGGED.shapes)
    assert len(plan_groups(na, nb, limit)) == 3
    split = dc.run(_rt(), dc.RAGGED._replace(max_ws=limit))
    assert dc.compare(split, dc.RAGGED) == []
    for one, two in zip(dc.download(ragged), dc.download(split)):
        for key in dc.KEYS:
            assert dc.same_bits(one[key], two[key]), key


# ---- d. non-finite input ---------------------------------------------------------------------------------------------
def test_a_nan_row_leaves_a_well_formed_path():
    from world.align import align_device

    rt = _rt()
    rng = np.random.RandomState(9)
    a, b = rng.randn(140, 5), rng.randn(90, 5)
    a[37] = np.nan
    b[60, 2] = np.inf
    ba = rt.make_batch([0, 0], [0, 140])
    bb = rt.make_batch([0, 0], [0, 90])
    for radius in (None, 3):
        al = align_device(rt, ba, rt.to_device(a), bb, rt.to_device(b), radius=radius)
        pa, pb = al.pairs(0)
        assert ref.well_formed(pa, pb, 140, 90)
        m = al.map_b2a.cpu().numpy()
        assert m.min() >= 0 and m.max() < 140
    assert rt.take_flags() == [0] * 16


def test_arguments_the_library_refuses():
    """Behind the Python checks: the C entry fails with a message, before anything is launched."""
    from world import _hip

    rt = _rt()
    one, two, empty = rt.make_batch([0, 0], [0, 4]), rt.make_batch([0, 0, 0], [0, 2, 4]), rt.make_batch([0, 0, 0], [0, 4, 4])
    x = rt.zeros((4, 3))
    i64 = rt.torch.int64
    outs = [rt.zeros((16,), i64) for _ in range(5)] + [rt.zeros((4,))]
    off = np.array([0, 7, 14], dtype=np.int64)

    def call(a, b, d=3):
        return rt.lib.wh_dtw(rt.ctx, rt.stream(), a.handle, b.handle, rt.ptr(x), 3, rt.ptr(x), 3, d, 0,
                             off.ctypes.data_as(_hip._c_i64p), rt.ptr(outs[0]), rt.ptr(outs[1]), rt.ptr(outs[2]),
                             rt.ptr(outs[5]), rt.ptr(outs[3]), rt.ptr(outs[4]), None, None)

    for args, word in (((one, two), b"same number"), ((two, empty), b"no frames"), ((one, one, 65), b"d must be")):
        assert call(*args) != 0
        assert word in rt.lib.wh_last_error()
    assert call(one, one) == 0 and call(two, two) == 0
    rt.torch.cuda.synchronize()


# ---- e. end to end ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def parallel():
    """Two utterances of 1 s and 1.3 s standing in for two speakers' recordings of one sentence; read-only."""
    from conftest import synth_cached
    from world.batch import WorldBatch

    wb = WorldBatch(0)
    enc_a = wb.encode([synth_cached(60, FS, 1.0)], FS, f0_method="dio", want_coarse=True)
    enc_b = wb.encode([synth_cached(61, FS, 1.3)], FS, f0_method="dio", want_coarse=True)
    return wb, enc_a, enc_b, enc_a.align(enc_b)


def test_encoded_utterances_align_as_the_reference_says(parallel):
    wb, enc_a, enc_b, al = parallel
    n, m = enc_a.batch.total_frames, enc_b.batch.total_frames
    pa, pb = al.pairs(0)
    assert ref.well_formed(pa, pb, n, m) and max(n, m) <= len(pa) <= n + m - 1
    ma = np.ascontiguousarray(enc_a.mcep(40).cpu().numpy()[:, 1:])
    mb = np.ascontiguousarray(enc_b.mcep(40).cpu().numpy()[:, 1:])
    want = ref.dtw(ma, mb)
    assert np.array_equal(pa, want["path_a"]) and np.array_equal(pb, want["path_b"])
    assert al.cost.cpu().numpy().tobytes() == np.array([want["cost"]]).tobytes()
    assert al.mcd_db().cpu().numpy().tobytes() == np.array([want["mcd"]]).tobytes()
    assert np.array_equal(al.map_b2a.cpu().numpy(), want["map_b2a"])
    assert np.array_equal(al.map_a2b.cpu().numpy(), want["map_a2b"])
    joint, off = al.joint(enc_a.mcep(40)[:, 1:], enc_b.mcep(40)[:, 1:])
    assert tuple(joint.shape) == (len(pa), 78) and off.tolist() == [0, len(pa)]
    assert np.array_equal(joint.cpu().numpy(), np.concatenate([ma[pa], mb[pb]], axis=1))


def test_warp_gathers_by_the_frame_map_and_decodes(parallel):
    import torch

    wb, enc_a, enc_b, al = parallel
    w = al.warp(enc_a, enc_b)
    assert w.batch is enc_b.batch and torch.equal(w.temporal_positions, enc_b.temporal_positions)
    for name in ("f0", "vuv", "spectrogram", "aperiodicity", "coarse_ap", "ap_gate"):
        assert torch.equal(getattr(w, name), getattr(enc_a, name).index_select(0, al.map_b2a)), name
    assert w.ps_spectrogram is None and w._timebase is None
    y, y_off = wb.decode_device(w)
    _, want_off = wb.decode_device(enc_b)
    assert np.array_equal(np.asarray(y_off), np.asarray(want_off))
    assert bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0
    assert wb.rt.take_flags() == [0] * 16


def test_an_encoding_aligned_with_itself_is_the_diagonal(parallel):
    wb, enc_a, _, _ = parallel
    al = enc_a.align(enc_a, radius=5)
    n = enc_a.batch.total_frames
    pa, pb = al.pairs(0)
    assert np.array_equal(pa, np.arange(n)) and np.array_equal(pb, np.arange(n))
    assert float(al.cost.cpu()[0]) == 0.0 and float(al.mcd_db().cpu()[0]) == 0.0
    assert np.array_equal(al.map_a2b.cpu().numpy(), np.arange(n))
