"""CPU: the host side of compact encodings (world/compact.py) — the committed fixture is self-consistent with
world/d4c.py:45-59 restated in NumPy, save_npz / load_npz round-trip a ragged batch exactly, and every argument check
raises before a device is touched.  No GPU, no library call."""
import ast
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dense_from_bands_np(coarse, failed, fs, fft_size):
    """world/d4c.py:44-59 for stored band values: (K, frames)."""
    from scipy.interpolate import interp1d

    interval = 2000 if fs < 16000 else 3000
    nap = coarse.shape[0]
    frequency_axis = np.arange(fft_size / 2 + 1) * fs / fft_size
    coarse_axis = np.r_[np.arange(nap + 1) * interval, fs / 2]
    ap = np.zeros([fft_size // 2 + 1, coarse.shape[1]])
    for i in range(coarse.shape[1]):
        if failed[i]:
            ap[:, i] = 1 - 0.000000000001
            continue
        ap[:, i] = 10 ** ((interp1d(coarse_axis, np.r_[np.r_[-60, coarse[:, i]], -0.000000000001])(frequency_axis)) / 20)
    return ap


@pytest.mark.parametrize("tag,nap", [("16k", 1), ("48k", 5)])
def test_fixture_is_self_consistent(golden, tag, nap):
    g = golden("compact")
    fs, fft_size = int(g["fs_" + tag]), int(g["fft_size_" + tag])
    coarse, failed, cols = g["coarse_" + tag], g["failed_" + tag], g["ap_frames_" + tag]
    assert coarse.shape == (nap, len(failed)) and g["ap_" + tag].shape == (fft_size // 2 + 1, len(cols))
    assert failed.any() and (~failed).any() and failed[cols].any() and (~failed[cols]).any()
    assert np.array_equal(g["ap_" + tag][0] > 0.5, failed[cols])
    assert not coarse[:, failed].any() and (coarse <= 0).all()  # a rejected frame keeps ap_debug's zeros (d4c.py:42,49-51)
    want = _dense_from_bands_np(coarse, failed, fs, fft_size)
    assert np.max(np.abs(want[:, cols] - g["ap_" + tag])) <= 1e-12
    # 1 s at a 5 ms hop
    assert len(failed) == 201


def _ragged_host(is_requiem=False, n0=40):
    from world.compact import CompactEncoding

    rng = np.random.RandomState(3)
    nfs = [57, 0, 131, 2]
    fo = np.concatenate([[0], np.cumsum(nfs)])
    f = int(fo[-1])
    tp = np.concatenate([np.arange(n) * 0.005 for n in nfs])
    vuv = (rng.rand(f) > 0.3).astype(np.float64)
    band = -np.abs(rng.randn(f, 3 if is_requiem else 1)) * 5
    band[5, :] = -0.0
    return CompactEncoding(None, 16000, 1024, 5, is_requiem, n0, 0, 8000, fo, tp, rng.rand(f) * 200 * vuv, vuv,
                           rng.randn(f, n0), band, None if is_requiem else vuv * (rng.rand(f) > 0.2), tp_host=tp)


@pytest.mark.parametrize("is_requiem", [False, True])
def test_save_and_load_round_trip_a_ragged_batch_exactly(tmp_path, is_requiem):
    from world.compact import CompactEncoding

    ce = _ragged_host(is_requiem)
    path = str(tmp_path / "batch.npz")
    ce.save_npz(path)
    back = CompactEncoding.load_npz(path)
    assert back.rt is None
    assert (back.fs, back.fft_size, back.frame_period, back.is_requiem, back.n0, back.lowhz, back.highhz) == \
           (16000, 1024, 5, is_requiem, 40, 0, 8000)
    assert np.array_equal(back.frame_off, ce.frame_off) and back.n_utt == 4 and back.total_frames == 190
    for k in ("temporal_positions", "f0", "vuv", "mcep", "band_ap"):
        a, b = getattr(ce, k), getattr(back, k)
        assert a.dtype == b.dtype == np.float64 and a.tobytes() == b.tobytes(), k  # (bytes: a -0.0 stays one)
    assert (back.ap_gate is None) if is_requiem else back.ap_gate.tobytes() == ce.ap_gate.tobytes()
    assert back.nbytes() == ce.nbytes() == 190 * (3 + 40 + (3 if is_requiem else 2)) * 8
    # and through the plain dicts of World.encode_compact_batch
    dats = ce.to_dicts()
    assert [len(d["f0"]) for d in dats] == [57, 0, 131, 2]
    again = CompactEncoding.from_dicts(dats)
    assert np.array_equal(again.frame_off, ce.frame_off)
    assert again.mcep.tobytes() == ce.mcep.tobytes() and again.band_ap.tobytes() == ce.band_ap.tobytes()


def test_bytes_per_frame():
    """ISSUE figures: dense (2 K + 3) * 8 B per frame, compact (n0 + nap + 4) * 8: 8 232 against 360 at 16 kHz, n0 = 40."""
    ce = _ragged_host()
    k = ce.fft_size // 2 + 1
    assert (2 * k + 3) * 8 == 8232
    assert ce.nbytes() == ce.total_frames * 360


class _NoDevice:
    """Stands in for a resident BatchEncoding: any use of the runtime is an error."""

    def __init__(self, fs, fft_size=1024, is_requiem=False):
        self.fs, self.fft_size, self.is_requiem = fs, fft_size, is_requiem

    def __getattr__(self, name):
        raise AssertionError("compact() touched '%s' before its checks" % name)


def test_argument_checks_raise_before_any_device_call():
    from world import main
    from world.batch import BatchEncoding
    from world.compact import CompactEncoding

    for fs in (8000, 22050, 48000):
        with pytest.raises(ValueError, match="16000"):
            BatchEncoding.compact(_NoDevice(fs, 2048), n0=40)
    for n0 in (1, 0, -3, 514, 2.5):
        with pytest.raises(ValueError, match="n0"):
            BatchEncoding.compact(_NoDevice(16000), n0=n0)
    W = main.World()
    x = np.zeros(1600)
    with pytest.raises(ValueError, match="16000"):
        W.encode_compact_batch(48000, [x])
    with pytest.raises(ValueError, match="n0"):
        W.encode_compact_batch(16000, [x], n0=1)
    with pytest.raises(ValueError, match="n0"):
        W.encode_compact_batch(16000, [x], n0=258, fft_size=512)
    with pytest.raises(NotImplementedError, match="devices"):
        W.encode_compact_batch(16000, [x], devices=[0])
    # mismatched lengths
    dats = _ragged_host().to_dicts()
    good = [dats[0], dats[2]]
    for key, val in (("vuv", good[0]["vuv"][:-1]), ("mcep", good[0]["mcep"][1:]), ("coarse_ap", good[0]["coarse_ap"][:, 1:]),
                     ("ap_gate", good[0]["ap_gate"][:5]), ("temporal_positions", np.zeros(3)), ("ap_gate", None)):
        bad = [dict(good[0], **{key: val}), good[1]]
        with pytest.raises(ValueError, match=key):
            W.decode_compact_batch(bad)
    # dicts of mixed fs / fft_size / is_requiem / coefficient count
    for key, val in (("fs", 48000), ("fft_size", 2048), ("is_requiem", True)):
        with pytest.raises(ValueError, match="share"):
            W.decode_compact_batch([good[0], dict(good[1], **{key: val})])
    with pytest.raises(ValueError, match="mcep"):
        W.decode_compact_batch([good[0], dict(good[1], mcep=good[1]["mcep"][:, :12])])
    with pytest.raises(ValueError, match="2 frames"):
        W.decode_compact_batch([dats[1]])
    with pytest.raises(ValueError):
        CompactEncoding(None, 16000, 1024, 5, False, 40, 0, 8000, [0, 4], np.zeros(4), np.zeros(4), np.zeros(3),
                        np.zeros((4, 40)), np.zeros((4, 1)), np.zeros(4))


def test_new_names_are_on_world_and_the_module_stands_alone():
    from world import d4c, main
    from world.batch import BatchEncoding

    assert callable(main.World.encode_compact_batch) and callable(main.World.decode_compact_batch)
    assert callable(BatchEncoding.compact) and callable(d4c.aperiodicity_from_coarse)
    src = open(os.path.join(ROOT, "python-world_amd", "world", "compact.py")).read()
    names = set()
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.Import):
            names.update(a.name.split(".")[0] for a in node.names)
        elif isinstance(node, ast.ImportFrom) and node.level == 0:
            names.add((node.module or "").split(".")[0])
    assert "oracle" not in names and "oracle" not in src


def test_the_abi_declares_the_expansion():
    from world import _hip

    assert "wh_aperiodicity_from_bands" in _hip.SIGNATURES and "wh_aperiodicity_gate" in _hip.SIGNATURES
    header = open(os.path.join(ROOT, "include", "world_hip.h")).read()
    assert "int wh_aperiodicity_from_bands(" in header and "d4c.py:45-59" in header
