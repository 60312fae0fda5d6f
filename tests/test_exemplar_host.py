"""The host side of world.exemplar (no GPU): the scales against NumPy, succ at utterance ends, every argument check
raising before a device is touched, the .npz round trip, the header's declarations against the binding's arity and
the constants the tests restate against csrc/wh_exemplar.hip."""
import os
import re

import numpy as np
import pytest

from world import _hip, exemplar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _db(r=12, d=3, kind="mcep", **kw):
    rng = np.random.RandomState(1)
    x, y = rng.randn(r, 2 * d), rng.randn(r, 2 * d)
    off = [0, 5, 5, 6, r]
    return exemplar.FrameDatabase(x, y, exemplar.chain_succ(off), exemplar.column_scales(x), exemplar.column_scales(y), off,
                                  kind=kind, **kw)


def test_library_and_binding():
    lib = _hip.load_library()
    assert lib.wh_version() >= 124
    for name in ("wh_knn", "wh_frame_select"):
        assert hasattr(lib, name) and name in _hip.SIGNATURES
    with open(os.path.join(ROOT, "include", "world_hip.h")) as f:
        header = f.read()
    for name in ("wh_knn", "wh_frame_select"):
        decl = re.search(r"\nint %s\((.*?)\);" % name, header, re.S).group(1)
        assert len(decl.split(",")) == len(_hip.SIGNATURES[name][1]), name


def test_constants_are_the_kernels():
    with open(os.path.join(ROOT, "python-world_amd", "csrc", "wh_exemplar.hip")) as f:
        src = f.read()
    for name, value in (("kKnnTileQ", exemplar.TILE_Q), ("kKnnTileR", exemplar.TILE_R), ("kKnnStrip", exemplar.STRIP),
                        ("kFsChunk", exemplar.CHUNK), ("kKnnMaxD", exemplar.MAX_D), ("kKnnMaxK", exemplar.MAX_K),
                        ("kFsMaxK", exemplar.MAX_K), ("kFsMaxDy", exemplar.MAX_DY)):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1)) == value, name
    import _exemplar_cases as xc
    assert (xc.TILE_Q, xc.TILE_R, xc.STRIP, xc.CHUNK) == (exemplar.TILE_Q, exemplar.TILE_R, exemplar.STRIP, exemplar.CHUNK)


def test_scales():
    rng = np.random.RandomState(0)
    rows = rng.randn(50, 6) * np.array([1e-3, 1.0, 50.0, 1.0, 1.0, 1.0])
    rows[:, 3] = 2.5               # zero std
    rows[7, 4] = np.inf            # std not finite
    rows[9, 5] = np.nan
    s = exemplar.column_scales(rows)
    assert s[:3].tobytes() == (1.0 / np.std(rows[:, :3], axis=0)).tobytes()
    assert s[3:].tolist() == [1.0, 1.0, 1.0]
    assert exemplar.column_scales(np.zeros((0, 2))).tolist() == [1.0, 1.0]


def test_succ_at_utterance_ends():
    assert exemplar.chain_succ([0, 3, 4, 4, 6]).tolist() == [1, 2, 2, 3, 5, 5]  # (a one-frame utterance follows itself)
    assert exemplar.chain_succ([0, 1]).tolist() == [0] and exemplar.chain_succ([0, 1]).dtype == np.int32


def test_npz_round_trip(tmp_path):
    for db in (_db(), _db(d=4, kind="lsf", lsf_order=4, lsf_min_gap=0.0123)):
        path = str(tmp_path / ("db_%s.npz" % db.kind))
        db.save_npz(path)
        back = exemplar.FrameDatabase.load_npz(path)
        for name in ("x", "y", "succ", "scale_x", "scale_y", "utt_off"):
            assert getattr(back, name).tobytes() == getattr(db, name).tobytes() and getattr(back, name).dtype == getattr(db, name).dtype
        assert (back.kind, back.lsf_order, back.lsf_min_gap, back.windows) == (db.kind, db.lsf_order, db.lsf_min_gap, db.windows)
    t = db.host_tables()
    assert t["x"].tobytes() == (db.x * db.scale_x).tobytes() and t["var_y"].tobytes() == np.var(db.y, axis=0).tobytes()


def test_database_checks():
    rng = np.random.RandomState(2)
    x = rng.randn(6, 4)
    ok = dict(x=x, y=x, succ=[1, 2, 3, 4, 5, 5], scale_x=np.ones(4), scale_y=np.ones(4), utt_off=[0, 6])
    exemplar.FrameDatabase(**ok)
    for change in (dict(y=x[:5]), dict(succ=[1, 2, 3, 4, 5, 6]), dict(succ=[1, 2, 3]), dict(scale_x=np.ones(3)), dict(utt_off=[0, 5]),
                   dict(utt_off=[0, 4, 3, 6]), dict(x=x[:, :3], y=x[:, :3]), dict(kind="spectrogram"), dict(kind="lsf"),
                   dict(lsf_order=2), dict(kind="lsf", lsf_order=4, lsf_min_gap=0.1), dict(x=np.zeros((0, 4)), y=np.zeros((0, 4))),
                   dict(x=np.zeros((6, 162)), y=np.zeros((6, 162)))):
        with pytest.raises(ValueError):
            exemplar.FrameDatabase(**dict(ok, **change))


def test_argument_checks_touch_no_device():
    db = _db()
    for kw in (dict(k=0), dict(k=33), dict(k=2.5), dict(weight=-1.0), dict(weight=float("nan")), dict(weight=float("inf")),
               dict(mode="frame"), dict(d=4), dict(exclude=[0]), dict(exclude=[0, 9]), dict(exclude=[0, True])):
        a = dict(dict(n_utt=2, d=3, k=4, weight=1.0, mode="frames", exclude=None), **kw)
        with pytest.raises(ValueError):
            exemplar.check_convert_args(a["n_utt"], a["d"], db, a["k"], a["weight"], a["mode"], a["exclude"])
    lo, hi = exemplar.check_convert_args(3, 3, db, 4, 0.0, "mlpg", [None, 3, 1])
    assert lo.tolist() == [0, 6, 5] and hi.tolist() == [0, 12, 5] and lo.dtype == np.int32
    one = exemplar.FrameDatabase(db.x[:5], db.y[:5], [1, 2, 3, 4, 4], db.scale_x, db.scale_y, [0, 5])
    with pytest.raises(ValueError, match="leaves no row"):
        exemplar.check_convert_args(1, 3, one, 4, 1.0, "frames", [0])
    for args in ((3, 4, 5, 3, 2, 0), (3, 0, 5, 0, 2, 0), (3, 161, 5, 161, 2, 0), (3, 4, 2 ** 31, 4, 2, 0), (3, 4, 5, 4, 2, -1),
                 (3, 4, 5, 4, 2, 65536), (3, 4, 5, 4, True, 0)):
        with pytest.raises(ValueError):
            exemplar.check_knn_args(*args)
    for args in ((5, (5, 3), (5, 3), (9, 65), 9, 1.0), (5, (4, 3), (4, 3), (9, 4), 9, 1.0), (5, (5, 3), (5, 2), (9, 4), 9, 1.0),
                 (5, (5, 33), (5, 33), (9, 4), 9, 1.0), (5, (5, 3), (5, 3), (9, 4), 8, 1.0), (5, (5, 3), (5, 3), (9, 4), 9, -0.5)):
        with pytest.raises(ValueError):
            exemplar.check_select_args(*args)

    class Host:  # an encoding that is not resident: refused before anything else is looked at
        rt, mcep, lsf, kind, lsf_order = None, None, None, "mcep", None
    with pytest.raises(ValueError, match="resident"):
        exemplar.build_compact(Host(), Host(), None)
    with pytest.raises(ValueError, match="host"):
        exemplar.convert_compact(Host(), db)
    from world.main import World
    with pytest.raises(NotImplementedError):
        World().build_exemplars([], [], devices=[0])
    with pytest.raises(NotImplementedError):
        World().convert_voice_exemplar({}, db, devices=[0])
    with pytest.raises(ValueError):
        World().build_exemplars([], [])
