"""CPU: the host side of world/lsf.py and of the LSF kind of compact encodings: the three ABI entries are declared, bound
and exported, the flag has its slot and its text, the kernel constants are the module's, the host tables are the
reference's bit for bit, every argument error is raised before a device is needed, the facade has the methods, and an
.npz of either kind — and one written before the kind existed — loads bit for bit."""
import os
import re

import numpy as np
import pytest

import _lsf_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = (("wh_lpc_levinson", 11), ("wh_lsf_from_lpc", 11), ("wh_lsf_envelope", 10))


def test_header_declares_and_binding_lists_the_three_entries():
    from world import _hip

    header = open(os.path.join(ROOT, "include", "world_hip.h")).read()
    for name, n_args in ENTRIES:
        decl = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == len(_hip.SIGNATURES[name][1]) == n_args
    assert re.search(r"#define WH_FLAG_LSF 7\b", header) and _hip.FLAG_LSF == 7
    assert len({int(v) for v in re.findall(r"#define WH_FLAG_\w+ (\d+)", header)}) == 8  # every slot its own
    assert "LSF" in _hip.FLAG_MESSAGES[_hip.FLAG_LSF]
    with pytest.raises(_hip.WorldHipError, match="LSF"):
        _hip.Runtime.raise_for_flags([0] * 7 + [1] + [0] * 8, "test")


def test_library_version_and_exports():
    from world import _hip

    lib = _hip.load_library()
    assert lib.wh_version() >= 118
    for name, _ in ENTRIES:
        assert hasattr(lib, name)
    assert lib.wh_lpc_levinson(None, None, None, 0, 25, 24, None, 25, None, None, 24) != 0
    assert b"null" in lib.wh_last_error()
    assert lib.wh_lsf_from_lpc(None, None, None, 0, 25, 24, None, 4097, None, 24, None) != 0
    assert lib.wh_lsf_envelope(None, None, None, 0, 25, 24, None, 513, None, 513) != 0


def test_constants_match_the_kernel_source_and_the_reference():
    from world import lsf

    src = open(os.path.join(ROOT, "python-world_amd", "csrc", "wh_lsf.hip")).read()
    value = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))  # noqa: E731
    assert value("kLsfMaxOrder") == lsf.MAX_ORDER == ref.MAX_ORDER == 64
    assert value("kLsfGridMax") == lsf.GRID_MAX == ref.G_MAX == 4096 and value("kLsfGridMin") == ref.G_MIN == 256
    assert value("kLsfMaxBisect") == ref.MAX_BISECT
    # the unit takes build.py's default flags: no contraction, no entry of its own
    build = open(os.path.join(ROOT, "python-world_amd", "build.py")).read()
    assert "wh_lsf" not in build and "-ffp-contract=off" in build
    assert not re.search(r"\b(cos|sin|acos|exp|log|sincos\w*)\s*\(", re.sub(r"//.*", "", src))  # no transcendental


def test_host_tables_are_the_reference_tables():
    from world import lsf

    assert lsf.grid_table().tobytes() == ref.grid_table().tobytes()
    g = lsf.grid_table()
    assert len(g) == 4097 and g[0] == 1.0 and g[-1] == -1.0 and np.all(np.diff(g) < 0) and not g.flags.writeable
    for k_bins in (129, 513, 1025):
        c = lsf.bin_table(k_bins)
        assert c.tobytes() == ref.bin_table(k_bins).tobytes() and c[0] == 1.0 and c[-1] == -1.0 and np.all(np.diff(c) < 0)
        # the bins of every K with 4096 % (K - 1) == 0 are points of the grid: one cosine for one angle
        assert np.array_equal(c, g[::4096 // (k_bins - 1)])
    for k_bins, p in ((129, 24), (513, 64), (1025, 40)):
        t = lsf.autocorr_table(k_bins, p)
        assert t.w.tobytes() == ref.autocorr_table(k_bins, p).tobytes() and t.w.shape == (k_bins, p + 1) and t.tag != 0
        # it is the inverse real transform: lags of a random row against numpy's irfft
        s = np.random.RandomState(k_bins).rand(k_bins)
        assert np.allclose(s @ t.w, np.fft.irfft(s)[:p + 1], rtol=0, atol=1e-15 * k_bins)
    assert lsf.autocorr_table(513, 24).tag != lsf.autocorr_table(513, 40).tag


def test_argument_checks_need_no_device():
    from world import lsf
    from world.main import World

    for bad in (3, 25, 0, 66, -2, 2.5, True, 1):
        with pytest.raises(ValueError, match="even integer"):
            lsf.check_order(bad)
    assert [lsf.check_order(p) for p in (2, 24, 64)] == [2, 24, 64]
    with pytest.raises(ValueError, match="too few"):
        lsf.check_order(40, "x", 33)
    assert lsf.check_order(32, "x", 33) == 32
    for bad in (0, 3, 1023, 65536):
        with pytest.raises(ValueError, match="fft_size"):
            lsf.check_fft_size(bad)
    assert lsf.check_fft_size(1024) == 513
    w = World()
    spec = np.ones((5, 33))
    with pytest.raises(ValueError, match="even integer"):
        w.encode_lsf(spec, order=25)
    with pytest.raises(ValueError, match="even integer"):
        w.encode_lsf(spec, order=66)
    with pytest.raises(ValueError, match="too few"):
        w.encode_lsf(spec, order=40)
    with pytest.raises(ValueError, match="too few"):
        w.encode_lpc(spec, order=40)
    with pytest.raises(ValueError, match="columns"):
        w.encode_lsf(np.ones(33), order=24)
    with pytest.raises(ValueError, match="even integer"):
        w.decode_lsf(np.ones((5, 26)), 1024)  # the gain and 25 angles: an odd order
    with pytest.raises(ValueError, match="fft_size"):
        w.decode_lsf(np.ones((5, 25)), 1023)


def test_facade_exposes_the_methods():
    from world import lsf
    from world.batch import BatchEncoding
    from world.main import World
    import inspect

    for name in ("encode_lsf", "decode_lsf", "encode_lpc"):
        assert callable(getattr(World, name))
    for name in ("lsf_device", "ilsf_device", "lpc_device", "autocorr_device", "levinson_device", "lsf_from_lpc_device",
                 "envelope_device"):
        assert callable(getattr(lsf, name))
    sig = inspect.signature(BatchEncoding.compact)
    assert sig.parameters["lsf_order"].default is None and sig.parameters["n0"].default == 40
    assert inspect.signature(World.encode_lsf).parameters["order"].default == 24


class _NoDevice:
    """Stands in for a BatchEncoding: compact() must raise before it touches anything but fs / fft_size."""

    def __init__(self, fs, fft_size=1024):
        self.fs, self.fft_size = fs, fft_size

    def __getattr__(self, name):
        raise AssertionError("compact() touched '%s' before its checks" % name)


def test_compact_refuses_wrong_orders_before_the_device_and_keeps_the_old_refusal():
    from world.batch import BatchEncoding

    for bad in (25, 66, 0, 2.5):
        with pytest.raises(ValueError, match="even integer"):
            BatchEncoding.compact(_NoDevice(48000, 2048), lsf_order=bad)
    with pytest.raises(ValueError, match="too few"):
        BatchEncoding.compact(_NoDevice(16000, 32), lsf_order=24)
    with pytest.raises(ValueError, match="16000"):  # the mel-cepstrum at another rate: as before
        BatchEncoding.compact(_NoDevice(48000, 2048), n0=40)


def _host_encoding(kind, fs=48000, fft_size=2048, frames=(5, 0, 7), seed=0):
    from world.compact import CompactEncoding, d4c_band_layout

    rng = np.random.RandomState(seed)
    nf = sum(frames)
    off = np.concatenate([[0], np.cumsum(frames)])
    _, nap = d4c_band_layout(fs)
    tp = np.arange(nf) * 0.005
    common = (tp, rng.rand(nf) * 200, (rng.rand(nf) > 0.3).astype(np.float64))
    band, gate = rng.rand(nf, nap), (rng.rand(nf) > 0.5).astype(np.float64)
    if kind == "lsf":
        rows = np.concatenate([rng.randn(nf, 1), np.sort(rng.uniform(0.01, 3.13, (nf, 24)), axis=1)], axis=1)
        return CompactEncoding(None, fs, fft_size, 5, False, None, 0, 8000, off, *common, None, band, gate, tp_host=tp, lsf=rows)
    if kind == "mcep":
        return CompactEncoding(None, fs, fft_size, 5, False, 40, 0, 8000, off, *common, rng.randn(nf, 40), band, gate, tp_host=tp)
    return CompactEncoding(None, fs, fft_size, 5, False, None, 0, 8000, off, *common, None, band, gate,
                           rng.rand(nf, fft_size // 2 + 1), tp_host=tp)


@pytest.mark.parametrize("kind,fs,fft_size", [("lsf", 48000, 2048), ("lsf", 16000, 1024), ("mcep", 16000, 1024),
                                               ("spectrogram", 48000, 2048)])
def test_npz_round_trip_of_every_kind(tmp_path, kind, fs, fft_size):
    from world.compact import CompactEncoding

    h = _host_encoding(kind, fs, fft_size)
    assert h.kind == kind and (h.lsf_order == 24) == (kind == "lsf")
    path = str(tmp_path / "ce.npz")
    h.save_npz(path)
    g = CompactEncoding.load_npz(path)
    assert g.kind == kind and g.lsf_order == h.lsf_order and g.n0 == h.n0 and g.fs == fs and g.fft_size == fft_size
    assert np.array_equal(g.frame_off, h.frame_off)
    for (ka, a), (kb, b) in zip(h._tensors(), g._tensors()):
        assert ka == kb and a.dtype == b.dtype == np.float64 and a.tobytes() == b.tobytes()
    with np.load(path) as z:
        assert ("lsf_order" in z.files) == (kind == "lsf") and ("lsf" in z.files) == (kind == "lsf")
    # and through the plain dicts
    dats = h.to_dicts()
    d = CompactEncoding.from_dicts(dats)
    assert d.kind == kind and d.lsf_order == h.lsf_order
    for (ka, a), (kb, b) in zip(h._tensors(), d._tensors()):
        assert ka == kb and a.tobytes() == b.tobytes()


def test_a_file_written_before_the_kind_existed_loads_as_it_did(tmp_path):
    """The keys the earlier save_npz wrote, and nothing else."""
    from world.compact import CompactEncoding

    h = _host_encoding("mcep", 16000, 1024)
    path = str(tmp_path / "old.npz")
    np.savez(path, temporal_positions=h.temporal_positions, f0=h.f0, vuv=h.vuv, mcep=h.mcep, band_ap=h.band_ap,
             ap_gate=h.ap_gate, frame_off=h.frame_off, fs=np.asarray(16000), fft_size=np.asarray(1024),
             frame_period=np.asarray(5.0), is_requiem=np.asarray(False), n0=np.asarray(40), lowhz=np.asarray(0.0),
             highhz=np.asarray(8000.0), mcep_fs=np.asarray(16000))
    g = CompactEncoding.load_npz(path)
    assert g.kind == "mcep" and g.lsf is None and g.lsf_order is None and g.n0 == 40 and g.mcep.tobytes() == h.mcep.tobytes()


def test_shape_checks_of_the_lsf_kind():
    from world.compact import CompactEncoding

    h = _host_encoding("lsf")
    args = dict(tp_host=h.tp_host)
    base = (None, h.fs, h.fft_size, 5, False, None, 0, 8000, h.frame_off, h.temporal_positions, h.f0, h.vuv)
    with pytest.raises(ValueError, match="exactly one"):
        CompactEncoding(*base, np.zeros((12, 40)), h.band_ap, h.ap_gate, lsf=h.lsf, **args)
    with pytest.raises(ValueError, match="'lsf' must be"):
        CompactEncoding(*base, None, h.band_ap, h.ap_gate, lsf=h.lsf[:-1], **args)
    with pytest.raises(ValueError, match="even integer"):
        CompactEncoding(*base, None, h.band_ap, h.ap_gate, lsf=h.lsf[:, :-1], **args)
    dats = h.to_dicts()
    with pytest.raises(ValueError, match="'lsf' must have shape"):
        CompactEncoding.from_dicts([dats[0], dict(dats[2], lsf=dats[2]["lsf"][:, :13])])
    assert h.nbytes() == 8 * 12 * (3 + 25 + 5 + 1)


def test_row_checks_keep_both_messages():
    import types

    import torch

    from world import _hip

    rt = types.SimpleNamespace(torch=torch)
    t = torch.zeros((4, 6), dtype=torch.float64)
    _hip.check_rows(rt, "rows", t, "w")
    _hip.check_rows(rt, "rows", t[:, :5], "w", 5)  # (a column slice keeps the unit column stride)
    assert _hip.ld(t[:, :5]) == 6 and _hip.ld(t[:1, :5]) == 5
    with pytest.raises(ValueError, match=r"w: rows must be \[frames\]\[>= 7\], got \(4, 6\)"):
        _hip.check_rows(rt, "rows", t, "w", 7)
    with pytest.raises(ValueError, match=r"w: rows must be \[frames\]\[>= 3\], got \(4,\)"):
        _hip.check_rows(rt, "rows", t[:, 0], "w", 3)
    for bad in (t.float(), t[:, ::2]):
        with pytest.raises(ValueError, match=r"w: rows must be a float64 tensor with unit column stride, got torch\.float"):
            _hip.check_rows(rt, "rows", bad, "w", 3)
        with pytest.raises(ValueError, match=r"w: rows must be a float64 tensor \[frames\]\[columns\] with unit column stride, got"):
            _hip.check_rows(rt, "rows", bad, "w")
    with pytest.raises(ValueError, match=r"\[frames\]\[columns\]"):
        _hip.check_rows(rt, "rows", t[0], "w")
