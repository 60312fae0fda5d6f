"""CPU: the host side of world/melcep.py — the ABI entry is declared, bound and exported and refuses a null context, the
customary alphas, the mel-cepstral distortion of a known difference, every argument error of the Python layer raised before
a device is needed, the facade has the methods — and wh_spectral_filter's binding is as it was."""
import os
import re
import types

import numpy as np
import pytest

import _melcep_reference as mref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_binding_lists_the_entry():
    from world import _hip

    header = open(os.path.join(ROOT, "include", "world_hip.h")).read()
    decl = re.search(r"int wh_melcep_filter\(([^;]*)\);", header)
    assert decl is not None
    assert len(decl.group(1).split(",")) == len(_hip.SIGNATURES["wh_melcep_filter"][1]) == 18
    names = [a.split()[-1].lstrip("*") for a in decl.group(1).split(",")]
    assert names == ["ctx", "stream", "n_utt", "h_x_off", "h_frame_off", "h_map_off", "h_map", "h_hop", "num", "ldn", "den", "ldd",
                     "order", "h_cos_beta", "h_sin_beta", "fft_size", "x", "y"]
    assert len(_hip.SIGNATURES["wh_spectral_filter"][1]) == 18


def test_library_version_and_export():
    from world import _hip

    lib = _hip.load_library()
    assert lib.wh_version() >= 127 and hasattr(lib, "wh_melcep_filter")
    assert lib.wh_melcep_filter(None, None, 0, None, None, None, None, None, None, 25, None, 0, 24, None, None, 1024, None, None) != 0
    assert lib.wh_last_error().decode().startswith("wh_melcep_filter")


def test_default_alpha():
    from world import melcep

    assert melcep.DEFAULT_ALPHA == {8000: 0.31, 10000: 0.35, 12000: 0.37, 16000: 0.42, 22050: 0.45, 24000: 0.466, 32000: 0.504,
                                    44100: 0.544, 48000: 0.554}
    assert melcep.default_alpha(16000) == 0.42 and melcep.default_alpha(48000.0) == 0.554
    for fs in (11025, 96000, 16000.5, True, 0):
        with pytest.raises(ValueError):
            melcep.default_alpha(fs)


def test_mcd_of_a_known_difference_on_tensors():
    import torch

    from world import melcep

    a = torch.zeros((3, 25), dtype=torch.float64)
    b = torch.zeros((3, 25), dtype=torch.float64)
    b[0, 0], b[1, 1], b[2, 1:] = 5.0, 1.0, 0.1
    got = melcep.mcd_db_device(a, b).numpy()
    assert np.allclose(got, mref.mcd_db(a.numpy(), b.numpy()), rtol=8 * np.finfo(np.float64).eps, atol=0)
    assert got[0] == 0.0 and abs(got[1] - 10 / np.log(10) * np.sqrt(2)) < 1e-14
    with pytest.raises(ValueError):
        melcep.mcd_db_device(a, b[:, :24])
    with pytest.raises(ValueError):
        melcep.mcd_db_device(a[:, :1], b[:, :1])


def test_argument_errors_before_any_device():
    import torch

    from world import melcep

    rt = types.SimpleNamespace(torch=torch)  # (every check below is made before the runtime is touched)
    x = torch.ones(200, dtype=torch.float64)
    num = torch.zeros((4, 25), dtype=torch.float64)

    def filt(**kw):
        a = dict(rt=rt, x_d=x, x_off=[0, 200], fs=16000, frame_period=5, fft_size=1024, num=num)
        a.update(kw)
        return melcep.filter_device(**a)

    bad = {
        "order 0": dict(num=num[:, :1]),
        "order 65": dict(num=torch.zeros((4, 66), dtype=torch.float64)),
        "den of another order": dict(den=torch.zeros((4, 24), dtype=torch.float64)),
        "float32 rows": dict(num=num.float()),
        "strided columns": dict(num=torch.zeros((4, 50), dtype=torch.float64)[:, ::2]),
        "no customary alpha": dict(fs=11025),
        "alpha 1": dict(alpha=1.0),
        "alpha below -1": dict(alpha=-1.5),
        "fft_size": dict(fft_size=1000),
        "fft_size too large": dict(fft_size=8192),
        "window longer than the transform": dict(hop=600),
        "hop 0": dict(hop=0),
        "map entry outside the rows": dict(window_map=[[0, 1, 2, 7]]),
        "map of another length": dict(window_map=[[0, 1, 2]]),
        "frame offsets past the rows": dict(frame_off=[0, 5]),
        "short recording": dict(x_off=[0, 300]),
    }
    for name, kw in bad.items():
        with pytest.raises(ValueError):
            filt(**kw)
            pytest.fail(name)
    for fn, args in ((melcep.melcep_device, (rt, torch.ones((4, 513), dtype=torch.float64), 0, 0.42)),
                     (melcep.melcep_device, (rt, torch.ones((4, 513), dtype=torch.float64), 65, 0.42)),
                     (melcep.melcep_device, (rt, torch.ones((4, 513), dtype=torch.float64), 24, None)),
                     (melcep.melcep_device, (rt, torch.ones((4, 513), dtype=torch.float32), 24, 0.42)),
                     (melcep.melcep_device, (rt, torch.ones((4, 9), dtype=torch.float64), 24, 0.42)),
                     (melcep.spectrum_device, (rt, num, 1023, 0.42)),
                     (melcep.spectrum_device, (rt, num, 1024, 1.0)),
                     (melcep.spectrum_device, (rt, num[:, :1], 1024, 0.42)),
                     (melcep.spectrum_device, (rt, torch.zeros((4, 66), dtype=torch.float64), 1024, 0.42))):
        with pytest.raises(ValueError):
            fn(*args)
    for fn, args in ((melcep.encode_melcep, (np.ones((4, 513)), 0)), (melcep.encode_melcep, (np.ones(513), 24)),
                     (melcep.encode_melcep, (np.ones((4, 513)), 24, None, 11025)), (melcep.decode_melcep, (np.ones((4, 66)), 1024)),
                     (melcep.melcep_distortion, (np.ones((4, 25)), np.ones((4, 24)))),
                     (melcep.filter_waveform_melcep, (16000, np.ones((2, 100)), np.zeros((4, 25)))),
                     (melcep.filter_waveform_melcep, (16000, np.ones(100), np.zeros((4, 25)), np.zeros((4, 24)))),
                     (melcep.filter_waveform_melcep, (11025, np.ones(100), np.zeros((4, 25))))):
        with pytest.raises(ValueError):
            fn(*args)


def test_tables_are_cached_read_only_and_tagged():
    from world import melcep

    t = melcep.encode_table(257, 24, 0.42)
    assert t is melcep.encode_table(257, 24, 0.42) and t.tag != 0 and not t.w.flags.writeable
    assert melcep.decode_table(24, 0.42, 257).tag != t.tag
    c, s = melcep.warp_tables(513, 0.42)
    assert not c.flags.writeable and not s.flags.writeable and np.max(np.abs(c * c + s * s - 1)) < 4e-16


def test_the_facade_has_the_methods():
    from world import main

    for name in ("encode_melcep", "decode_melcep", "melcep_distortion", "filter_waveform_melcep"):
        assert callable(getattr(main.World, name))
