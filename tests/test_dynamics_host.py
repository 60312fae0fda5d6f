"""CPU: the host side of world/dynamics.py: the two ABI entries are declared, bound and exported, the facade has its
methods, every argument error is raised before a device is needed, and the workspace grouping splits as documented."""
import os
import re
import types

import numpy as np
import pytest

import _mlpg_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_binding_lists_both_entries():
    from world import _hip

    header = open(os.path.join(ROOT, "include", "world_hip.h")).read()
    for name, n_args in (("wh_delta_features", 11), ("wh_mlpg", 14)):
        decl = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == len(_hip.SIGNATURES[name][1]) == n_args
    assert re.search(r"#define WH_FLAG_MLPG_PIVOT 6\b", header) and _hip.FLAG_MLPG_PIVOT == 6
    assert "MLPG" in _hip.FLAG_MESSAGES[_hip.FLAG_MLPG_PIVOT]


def test_library_version_and_exports():
    from world import _hip

    lib = _hip.load_library()
    assert lib.wh_version() >= 115
    assert hasattr(lib, "wh_delta_features") and hasattr(lib, "wh_mlpg")


def test_constants_match_the_kernel_source_and_the_reference():
    from world import dynamics

    src = open(os.path.join(ROOT, "python-world_amd", "csrc", "wh_mlpg.hip")).read()
    value = lambda name: int(re.search(r"constexpr int %s = ([^;]+);" % name, src).group(1))  # noqa: E731
    assert value("kMlpgMaxWin") == dynamics.MAX_WINDOWS and value("kMlpgMaxTaps") == 2 * dynamics.MAX_HALF + 1
    assert dynamics.HTS_WINDOWS == ref.HTS_WINDOWS == ((0.0, 1.0, 0.0), (-0.5, 0.0, 0.5), (1.0, -2.0, 1.0))


def test_facade_exposes_the_methods():
    from world.compact import CompactEncoding
    from world.main import World

    assert callable(CompactEncoding.dynamic_features) and callable(CompactEncoding.with_trajectories)
    with pytest.raises(NotImplementedError):
        World().delta_features(np.zeros((3, 2)), devices=[0, 1])
    with pytest.raises(NotImplementedError):
        World().mlpg(np.zeros((3, 6)), np.ones(6), devices=[0, 1])


def test_window_checks():
    from world import dynamics

    win, half = dynamics.check_windows(dynamics.HTS_WINDOWS)
    assert half == 1 and win.shape == (3, 3) and win.dtype == np.float64 and win.flags.c_contiguous
    assert dynamics.check_windows([[1.0]])[1] == 0 and dynamics.check_windows([[0, 0, 1, 0, 0], [1, 2, 3, 4, 5]])[1] == 2
    for bad, word in (([[0.0, 0.5, 0.0], [-0.5, 0.0, 0.5]], "static"),            # window 0 not static
                      ([[0.0, 1.0, 1e-300]], "static"),
                      ([[1.0, 0.0, 0.0]], "static"),
                      ([[0.0, 1.0, 0.0], [1.0, 0.0, -2.0, 0.0, 1.0]], "same half-width"),  # mixed half-widths
                      ([[0, 0, 0, 1, 0, 0, 0]], "half-width"),                     # L > 2
                      ([[0.0, 1.0]], "taps"),
                      ([], "windows"),
                      ([[0, 1, 0]] * 5, "windows"),
                      ([[0.0, 1.0, 0.0], [np.nan, 0.0, 1.0]], "finite")):
        with pytest.raises(ValueError, match=word):
            dynamics.check_windows(bad)


def test_shape_checks():
    from world import dynamics

    assert dynamics.check_mlpg_shapes((7, 120), (7, 120), 7, 3) == (40, True)
    assert dynamics.check_mlpg_shapes((7, 120), (120,), 7, 3) == (40, False)
    for mean, var, word in (((7, 121), (7, 121), "windows"),      # a row width that is no multiple of n_win
                            ((6, 120), (6, 120), "frames"),       # not the batch's frames
                            ((7, 120), (7, 119), "var"), ((7, 120), (6, 120), "var"), ((7, 120), (40,), "var"),
                            ((7, 120), (1, 120), "var"), ((7, 2), (7, 2), "windows")):
        with pytest.raises(ValueError, match=word):
            dynamics.check_mlpg_shapes(mean, var, 7, 3)


def test_checks_come_before_the_device():
    """The fakes have no library behind them: reaching the device would raise something else."""
    from world import dynamics
    from world.main import World

    batch = types.SimpleNamespace(total_frames=5, n_utt=1, frame_off=np.array([0, 5]))
    t = lambda *shape: types.SimpleNamespace(shape=shape, dim=lambda: len(shape))  # noqa: E731
    rt = object()
    with pytest.raises(ValueError, match="static"):
        dynamics.delta_features_device(rt, batch, t(5, 3), [[0.5]])
    with pytest.raises(ValueError, match="frames"):
        dynamics.delta_features_device(rt, batch, t(4, 3))
    with pytest.raises(ValueError, match="half-width"):
        dynamics.mlpg_device(rt, batch, t(5, 9), t(9), [[0, 1, 0], [1, 0, 0, 0, 1]])
    with pytest.raises(ValueError, match="windows"):
        dynamics.mlpg_device(rt, batch, t(5, 10), t(10))
    with pytest.raises(ValueError, match="var"):
        dynamics.mlpg_device(rt, batch, t(5, 9), t(5, 3))
    w = World()
    with pytest.raises(ValueError, match="static"):
        w.delta_features(np.zeros((4, 2)), windows=[[2.0]])
    with pytest.raises(ValueError, match="T"):
        w.delta_features(np.zeros(4))
    with pytest.raises(ValueError, match="width"):
        w.delta_features([np.zeros((4, 2)), np.zeros((4, 3))])
    with pytest.raises(ValueError, match="var"):
        w.mlpg(np.zeros((4, 6)), np.ones(5))
    with pytest.raises(ValueError, match="var"):
        w.mlpg([np.zeros((4, 6))], [np.ones((3, 6))])
    with pytest.raises(ValueError, match="windows"):
        w.mlpg(np.zeros((4, 7)), np.ones(7))
    assert w.mlpg([], []) == [] and w.delta_features([]) == []
    ce = types.SimpleNamespace(rt=None, mcep=None)
    with pytest.raises(ValueError, match="host"):
        dynamics.compact_dynamic_features(ce)
    with pytest.raises(ValueError, match="static"):
        dynamics.compact_with_trajectories(ce, windows=[[0.0, 0.0, 1.0]])


def test_workspace_grouping_splits_as_documented():
    from world import dynamics

    assert dynamics.workspace_bytes(2001, 40, 1) == 8 * 2001 * 40 * 2
    assert dynamics.workspace_bytes(2001, 40, 0) == 0 and dynamics.workspace_bytes(10, 1, 2) == 320
    one = dynamics.workspace_bytes(100, 40, 1)
    n = [100] * 7
    assert dynamics.plan_groups(n, 40, 1, 10 * one) == [(0, 7)]
    assert dynamics.plan_groups(n, 40, 1, 3 * one) == [(0, 3), (3, 6), (6, 7)]
    assert dynamics.plan_groups(n, 40, 1, 3 * one - 1) == [(0, 2), (2, 4), (4, 6), (6, 7)]
    assert dynamics.plan_groups(n, 40, 1, 1) == [(u, u + 1) for u in range(7)]  # an utterance beyond the limit goes alone
    assert dynamics.plan_groups(n, 40, 0, 1) == [(0, 7)]                        # diagonal systems need no workspace
    assert dynamics.plan_groups([10, 1000, 10], 3, 2, dynamics.workspace_bytes(10, 3, 2) * 2) == [(0, 1), (1, 2), (2, 3)]
    assert dynamics.plan_groups([], 40, 1, 100) == []
    # the default holds 1024 utterances of 10 s and 40 columns in one call (1.3 GB)
    assert dynamics.plan_groups([2001] * 1024, 40, 1) == [(0, 1024)]
    assert dynamics.workspace_bytes(2001 * 1024, 40, 1) < dynamics.DEFAULT_MAX_WORKSPACE_BYTES
