"""CPU: the host side of the alignment (world/align.py): the ABI entry is declared and bound, the facade has its methods,
every argument error is raised before a device is needed, the workspace grouping splits as documented, and the tile
constants the GPU tests are built around are the kernel's."""
import os
import re
import types

import numpy as np
import pytest

import _dtw_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_binding_lists_wh_dtw():
    from world import _hip

    header = open(os.path.join(ROOT, "include", "world_hip.h")).read()
    decl = re.search(r"int wh_dtw\(([^;]*)\);", header)
    assert decl is not None
    assert len(decl.group(1).split(",")) == len(_hip.SIGNATURES["wh_dtw"][1]) == 19


def test_library_version_and_export():
    from world import _hip

    lib = _hip.load_library()
    assert lib.wh_version() >= 114
    assert hasattr(lib, "wh_dtw")


def test_tile_constants_match_the_kernel_source():
    from world import align

    src = open(os.path.join(ROOT, "python-world_amd", "csrc", "wh_dtw.hip")).read()
    value = lambda name: re.search(r"constexpr int %s = ([^;]+);" % name, src).group(1).strip()  # noqa: E731
    assert int(value("kDtwRowsPerLane")) == align.ROWS_PER_LANE
    assert value("kDtwStripRows") == "WH_WAVE * kDtwRowsPerLane" and align.STRIP_ROWS == 64 * align.ROWS_PER_LANE
    assert int(value("kDtwChunkCols")) == align.CHUNK_COLS
    assert "d < 1 || d > %d" % align.MAX_D in src


def test_facade_exposes_the_alignment_methods():
    from world.batch import BatchEncoding
    from world.main import World

    for name in ("align", "align_batch", "warp_to"):
        assert callable(getattr(World, name))
    assert callable(BatchEncoding.align)
    with pytest.raises(NotImplementedError):
        World().align_batch([], [], devices=[0, 1])


def _fake(rt, fs=16000, n_utt=2, frame_off=(0, 3, 7)):
    return types.SimpleNamespace(rt=rt, fs=fs, n_utt=n_utt, batch=types.SimpleNamespace(frame_off=np.array(frame_off)))


def test_encoding_checks_come_before_the_device():
    """The fakes have no tensors and no library behind them: reaching the device would raise something else."""
    from world.batch import BatchEncoding

    rt = object()
    a = _fake(rt)
    with pytest.raises(ValueError, match="sampling rates"):
        BatchEncoding.align(a, _fake(rt, fs=22050))
    with pytest.raises(ValueError, match="utterance"):
        BatchEncoding.align(a, _fake(rt, n_utt=3, frame_off=(0, 1, 2, 3)))
    with pytest.raises(ValueError, match="runtimes"):
        BatchEncoding.align(a, _fake(object()))
    with pytest.raises(ValueError, match="n0"):
        BatchEncoding.align(a, _fake(rt), n0=66)
    with pytest.raises(ValueError, match="n0"):
        BatchEncoding.align(a, _fake(rt), n0=1)
    with pytest.raises(ValueError, match="radius"):
        BatchEncoding.align(a, _fake(rt), radius=0)
    with pytest.raises(ValueError, match="no frames"):
        BatchEncoding.align(a, _fake(rt, frame_off=(0, 3, 3)))


def test_dict_checks_come_before_the_device():
    from world.main import World

    d = lambda fs, n: {'fs': fs, 'f0': np.zeros(n)}  # noqa: E731
    w = World()
    with pytest.raises(ValueError, match="against"):
        w.align_batch([d(16000, 3)], [])
    with pytest.raises(ValueError, match="sampling rates"):
        w.align(d(16000, 3), d(8000, 3))
    with pytest.raises(ValueError, match="n0"):
        w.align(d(16000, 3), d(16000, 3), n0=70)
    with pytest.raises(ValueError, match="radius"):
        w.align(d(16000, 3), d(16000, 3), radius=1.5)
    with pytest.raises(ValueError, match="no frames"):
        w.align(d(16000, 0), d(16000, 3))
    assert w.align_batch([], []) == []


def test_shape_and_radius_checks():
    from world import align

    assert align.check_radius(None) == 0 and align.check_radius(7) == 7 and align.check_radius(np.int64(2)) == 2
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            align.check_radius(bad)
    na, nb = align.check_pair_shapes([0, 2, 5], [0, 1, 9], 39)
    assert na.tolist() == [2, 3] and nb.tolist() == [1, 8]
    for d in (0, 65):
        with pytest.raises(ValueError, match="columns"):
            align.check_pair_shapes([0, 2], [0, 2], d)


def test_workspace_grouping_splits_as_documented():
    from world import align

    assert align.pair_workspace_bytes(2001, 2001) == 4 * 2001 * 126 + 8 * 2001
    assert align.pair_workspace_bytes(1, 1) == 12 and align.pair_workspace_bytes(3, 16) == 140 and align.pair_workspace_bytes(3, 17) == 160
    one = align.pair_workspace_bytes(100, 100)
    n = [100] * 7
    assert align.plan_groups(n, n, 10 * one) == [(0, 7)]
    assert align.plan_groups(n, n, 3 * one) == [(0, 3), (3, 6), (6, 7)]
    assert align.plan_groups(n, n, 3 * one - 1) == [(0, 2), (2, 4), (4, 6), (6, 7)]
    assert align.plan_groups(n, n, 1) == [(u, u + 1) for u in range(7)]  # a pair beyond the limit goes alone
    assert align.plan_groups([10, 1000, 10], [10, 1000, 10], align.pair_workspace_bytes(10, 10) * 2) == [(0, 1), (1, 2), (2, 3)]
    assert align.plan_groups([], [], 100) == []
    # the default holds 1024 pairs of 10 s x 10 s in one call
    assert align.plan_groups([2001] * 1024, [2001] * 1024) == [(0, 1024)]


def test_host_map_rule_and_warp_to_follow_the_reference():
    from world import align
    from world.main import World

    rng = np.random.RandomState(3)
    a, b = rng.randn(9, 2), rng.randn(14, 2)
    r = ref.dtw(a, b)
    a2b, b2a = align.maps_from_path(r["path_a"], r["path_b"], 9, 14)
    assert np.array_equal(a2b, r["map_a2b"]) and np.array_equal(b2a, r["map_b2a"])
    assert align.MCD_SCALE == ref.MCD_SCALE
    dat_a = {'fs': 16000, 'is_requiem': False, 'temporal_positions': np.arange(9) * 0.005, 'f0': rng.rand(9) + 100,
             'vuv': np.ones(9), 'spectrogram': rng.rand(5, 9), 'aperiodicity': rng.rand(5, 9)}
    dat_b = dict(dat_a, temporal_positions=np.arange(14) * 0.005, f0=np.zeros(14))
    out = World().warp_to(dat_a, dat_b, {'path_a': r["path_a"], 'path_b': r["path_b"]})
    assert np.array_equal(out['temporal_positions'], dat_b['temporal_positions'])
    assert np.array_equal(out['f0'], dat_a['f0'][r["map_b2a"]])
    assert np.array_equal(out['spectrogram'], dat_a['spectrogram'][:, r["map_b2a"]]) and out['spectrogram'].shape == (5, 14)
    with pytest.raises(ValueError, match="path"):
        World().warp_to(dat_a, dat_b, {'path_a': r["path_a"][:-1], 'path_b': r["path_b"][:-1]})
