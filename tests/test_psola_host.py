"""CPU: the host side of world/psola.py — the default parameters, the period track and the source map against
hand-computed tables, the capacities, the argument checks — and the library's declaration, binding and export of wh_psola."""
import os

import numpy as np
import pytest

import _psola_reference as pref
from world import psola


def test_library_declares_binds_and_exports_the_entry():
    from world import _hip

    lib = _hip.load_library()
    assert lib.wh_version() >= 125 and hasattr(lib, "wh_psola") and "wh_psola" in _hip.SIGNATURES
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "world_hip.h")).read()
    assert "int wh_psola(wh_ctx* ctx" in header and "ABI 125" in header
    assert len(_hip.SIGNATURES["wh_psola"][1]) == 27
    from world.main import World
    assert callable(World.modify_waveform) and callable(World.set_pitch_waveform)


def test_default_params():
    assert tuple(psola.default_params(16000)) == (16, 80, 80, 20, 10, 1)
    assert tuple(psola.default_params(22050)) == (22, 110, 110, 27, 13, 1)
    assert tuple(psola.default_params(48000)) == (48, 240, 240, 60, 30, 1)
    assert tuple(psola.default_params(192000, norm=0)) == (192, 960, 512, 240, 120, 0)  # the tolerance is capped
    assert tuple(psola.default_params(1600)) == (1, 8, 8, 2, 1, 1)
    for fs in (1500, 500000):  # pmin below 2; an unvoiced hop beyond 2048
        with pytest.raises(ValueError):
            psola.default_params(fs)
    assert (psola.PMAX, psola.MAX_GRID, psola.MAX_HOP, psola.MAX_TOL) == (pref.PMAX, pref.MAX_GRID, pref.MAX_HOP, pref.MAX_TOL)
    assert psola.Params._fields == pref.Params._fields


def test_period_track_against_a_hand_computed_table():
    # (a rate and frame times that are exact in binary: the ties are ties)
    fs, grid = 640, 10
    times = np.array([0.0, 2.0, 4.0, 6.0]) / 64.0  # frames at samples 0, 20, 40, 60
    f0 = np.array([64.0, 0.0, 80.0, 3.0])
    vuv = np.array([1.0, 1.0, 1.0, 1.0])
    # grid points at samples 0, 10, .. 70: the nearest frame, the earlier at 10, 30 and 50 — frames 0 0 1 1 2 2 3 3;
    # fs / f0 = 10, -, 8, 213.3
    got = psola.period_track(times, f0, vuv, fs, 75, grid, pmin=2)
    assert got.dtype == np.int32 and got.tolist() == [10, 10, 0, 0, 8, 8, 213, 213]
    # pmin = 9 makes the 8 unvoiced; vuv = 0 makes a frame unvoiced whatever its f0
    assert psola.period_track(times, f0, vuv, fs, 75, grid, pmin=9).tolist() == [10, 10, 0, 0, 0, 0, 213, 213]
    assert psola.period_track(times, f0, np.array([0.0, 1, 1, 1]), fs, 75, grid, pmin=2).tolist() == [0, 0, 0, 0, 8, 8, 213, 213]
    # rounding: fs / f0 + 0.5 floored — 640 / 51.2 = 12.5 -> 13, 640 / 52 = 12.3 -> 12; beyond PMAX -> 0
    assert psola.period_track([0.0], [51.2], [1], fs, 5, grid, pmin=2).tolist() == [13]
    assert psola.period_track([0.0], [52.0], [1], fs, 5, grid, pmin=2).tolist() == [12]
    assert psola.period_track([0.0], [0.3], [1], fs, 5, grid, pmin=2).tolist() == [0]
    # the default pmin is floor(fs / 800): 20 at 16 kHz — 850 Hz is no period, 790 Hz is
    assert psola.period_track([0.0], [850.0], [1], 16000, 5, 16).tolist() == [0]
    assert psola.period_track([0.0], [790.0], [1], 16000, 5, 16).tolist() == [20]
    # the output's grid under a stretch by 2: output sample k G is input sample k G / 2 — frames 0 0 0 0 1 1 1 1 2 ..
    got = psola.period_track(times, [64.0, 32.0, 80.0, 128.0], vuv, fs, 150, grid, time_map=2.0, pmin=2)
    assert got.tolist() == [10, 10, 10, 20, 20, 20, 20, 8, 8, 8, 8, 5, 5, 5, 5, 5]
    # and under a map: real time up to output sample 40, then the input stands still at sample 40 (frame 2)
    got = psola.period_track(times, [64.0, 32.0, 80.0, 128.0], vuv, fs, 90, grid, time_map=([0, 40, 100], [0, 40, 40]), pmin=2)
    assert got.tolist() == [10, 10, 20, 20, 8, 8, 8, 8, 8, 8]
    assert psola.period_track([], [], [], fs, 25, grid).tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        psola.period_track(times, f0[:3], vuv, fs, 75, grid)


def test_source_map_against_a_hand_computed_table():
    assert psola.source_map(45, 10).tolist() == [0, 10, 20, 30, 40] and psola.source_map(45, 10).dtype == np.int64
    assert psola.source_map(45, 10, 2.0).tolist() == [0, 5, 10, 15, 20]
    assert psola.source_map(30, 10, 0.8).tolist() == [0, 13, 25, 38]  # 12.5 rounds upwards, 37.5 too
    assert psola.source_map(0, 10, 1.25).tolist() == [0]
    assert psola.source_map(95, 10, ([0, 40, 100], [0, 20, 80])).tolist() == [0, 5, 10, 15, 20, 30, 40, 50, 60, 70]
    for ratio in (0.5, 0.8, 1.25, 2.0):  # one segment of slope 1 / ratio is the uniform stretch
        assert np.array_equal(psola.source_map(95, 10, ([0.0, 1000.0], [0.0, 1000.0 / ratio])), psola.source_map(95, 10, ratio))
    for bad in (0, -1.0, np.inf, np.nan, ([0, 0], [0, 1]), ([0], [0]), ([0, 1], [0, 1, 2])):
        with pytest.raises(ValueError):
            psola.source_map(100, 10, bad)


def test_capacities_are_the_reference_s():
    rng = np.random.RandomState(6)
    for _ in range(200):
        p = psola.Params(int(rng.randint(1, 4097)), int(rng.randint(1, 2049)), int(rng.randint(0, 513)), int(rng.randint(2, 2049)),
                         int(rng.randint(1, 2049)), 1)
        n = int(rng.randint(0, 100000))
        assert psola.mark_capacity(n, p) == pref.mark_capacity(n, pref.Params(*p))
        assert psola.smark_capacity(n, p) == pref.smark_capacity(n, pref.Params(*p))
    p = psola.default_params(16000)
    assert psola.mark_capacity(160000, p) == 10668 and psola.smark_capacity(160000, p) == 16001 and psola.mark_capacity(0, p) == 1


def test_argument_checks():
    p = psola.Params(16, 80, 50, 2, 1, 1)
    x_off, y_off, pa_off, ps_off, mark_off, smark_off = psola.check_psola_args([0, 200, 200, 233], [250, 0, 16], p)
    assert y_off.tolist() == [0, 250, 250, 266] and pa_off.tolist() == [0, 13, 14, 17] and ps_off.tolist() == [0, 16, 17, 19]
    assert mark_off.tolist() == [0, 101, 102, 120] and smark_off.tolist() == [0, 251, 252, 269]
    assert all(a.dtype == np.int64 for a in (x_off, y_off, pa_off, ps_off, mark_off, smark_off))
    for bad in (p._replace(grid=0), p._replace(grid=4097), p._replace(hop=0), p._replace(hop=2049), p._replace(tol=-1), p._replace(tol=513),
                p._replace(pmin=1), p._replace(pmin=2049), p._replace(smin=0), p._replace(smin=2049), p._replace(norm=2),
                p._replace(grid=16.0), p._replace(norm=True)):
        with pytest.raises(ValueError):
            psola.check_psola_args([0, 10], [10], bad)
    for x_off, lens in (([5, 0], [3]), ([-1, 4], [3]), ([0, 4], [3, 3]), ([0, 4], [-1]), ([0, 4], [2.5])):
        with pytest.raises(ValueError):
            psola.check_psola_args(x_off, lens, p)
