"""CPU: the host side of world/gmm.py: the four ABI entries are declared, bound and exported, the kernel constants are
the module's, every argument error is raised before a device is needed, a model survives an .npz round trip bit for
bit, and the workspace grouping splits as documented."""
import os
import re

import numpy as np
import pytest

import _gmm_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = (("wh_gmm_estep", 16), ("wh_gmm_stats", 13), ("wh_gmm_convert", 16), ("wh_gmm_workspace_bytes", 3))


def test_header_declares_and_binding_lists_the_four_entries():
    from world import _hip

    header = open(os.path.join(ROOT, "include", "world_hip.h")).read()
    for name, n_args in ENTRIES:
        decl = re.search(r"(?:int|int64_t) %s\(([^;]*)\);" % name, header)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == len(_hip.SIGNATURES[name][1]) == n_args


def test_library_version_and_exports():
    from world import _hip

    lib = _hip.load_library()
    assert lib.wh_version() >= 116
    for name, _ in ENTRIES:
        assert hasattr(lib, name)


def test_constants_match_the_kernel_source():
    from world import _hip, gmm

    src = open(os.path.join(ROOT, "python-world_amd", "csrc", "wh_gmm.hip")).read()
    value = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))  # noqa: E731
    assert value("kGmmMaxD") == gmm.MAX_D == 160 and value("kGmmMaxM") == gmm.MAX_M == 64
    assert value("kGmmRowTile") == gmm.ROW_TILE and value("kGmmSplitRows") == gmm.SPLIT_ROWS
    assert gmm.DEFAULT_MAX_WORKSPACE_BYTES == 4 << 30
    lib = _hip.load_library()  # the library's own statement of the workspace (host only: no device is touched)
    for n, d, m in ((0, 1, 1), (1, 1, 1), (4096, 39, 5), (4097, 156, 32), (2049024, 156, 32), (12291, 160, 64)):
        assert lib.wh_gmm_workspace_bytes(n, d, m) == gmm.workspace_bytes(n, d, m)
    assert gmm.workspace_bytes(2049024, 156, 32) == 8 * 501 * 32 * 157 * 157
    for n, d, m in ((-1, 4, 2), (10, 0, 2), (10, 161, 2), (10, 4, 0), (10, 4, 65)):
        assert lib.wh_gmm_workspace_bytes(n, d, m) == -1
        with pytest.raises(ValueError):
            gmm.workspace_bytes(n, d, m)


def test_entries_refuse_wrong_arguments_before_a_launch():
    """A null context is refused first of all, so the checks behind it are reached through world.gmm's own (below)."""
    from world import _hip

    lib = _hip.load_library()
    assert lib.wh_gmm_estep(None, None, None, 0, 1, 1, 1, None, None, None, None, 1, None, 1, None, None) != 0
    assert b"null" in lib.wh_last_error()
    assert lib.wh_gmm_stats(None, None, None, 0, 1, 1, 1, None, 1, None, None, None, None) != 0
    assert lib.wh_gmm_convert(None, None, None, 0, 1, 1, 1, 1, None, None, None, None, None, 1, None, 1) != 0


def _model(m=3, d=6, dx=3, seed=0):
    w, mu, cov = ref.random_mixture(m, d, np.random.RandomState(seed), 1e3)
    return w, mu, cov, dx


def test_model_checks():
    from world import gmm

    w, mu, cov, dx = _model()
    g = gmm.JointGMM(w, mu, cov, dx)
    assert (g.n_components, g.dim, g.dx, g.dy) == (3, 6, 3, 3)
    for bad_dx in (0, 6, 7, -1, 2.5, True):
        with pytest.raises(ValueError, match="dx"):
            gmm.JointGMM(w, mu, cov, bad_dx)
    with pytest.raises(ValueError, match="components"):
        gmm.JointGMM(np.full(65, 1 / 65), np.zeros((65, 2)), np.repeat(np.eye(2)[None], 65, 0), 1)
    with pytest.raises(ValueError, match="columns"):
        gmm.JointGMM(np.ones(1), np.zeros((1, 161)), np.eye(161)[None], 80)
    with pytest.raises(ValueError, match="weights"):
        gmm.JointGMM(w[:2], mu, cov, dx)
    with pytest.raises(ValueError, match="covariances"):
        gmm.JointGMM(w, mu, cov[:, :5], dx)
    with pytest.raises(ValueError, match="positive"):
        gmm.JointGMM(np.array([0.5, 0.5, 0.0]), mu, cov, dx)
    # not symmetric positive definite: the component is named
    skew = cov.copy()
    skew[1, 0, 1] += 1e-9
    with pytest.raises(ValueError, match="component 1 is not symmetric"):
        gmm.JointGMM(w, mu, skew, dx)
    indef = cov.copy()
    indef[2] = -indef[2]
    with pytest.raises(ValueError, match="component 2 is not positive definite"):
        gmm.JointGMM(w, mu, indef, dx)
    semi = cov.copy()
    semi[0] = np.ones((6, 6))
    with pytest.raises(ValueError, match="component 0"):
        gmm.JointGMM(w, mu, semi, dx)
    nan = cov.copy()
    nan[0, 2, 2] = np.nan
    with pytest.raises(ValueError, match="component 0"):
        gmm.JointGMM(w, mu, nan, dx)


def test_host_tables_are_the_reference_tables():
    from world import gmm

    w, mu, cov, dx = _model(seed=1)
    t = gmm.JointGMM(w, mu, cov, dx).host_tables()
    whiten, logc = ref.prepare(w, mu, cov, ref.LD)
    c = ref.conditional(w, mu, cov, dx, ref.LD)
    kappa = max(np.linalg.cond(s) for s in cov)
    tol = 4 * 36 * ref.U * kappa
    for got, want in ((t["whiten"], whiten), (t["logc"], logc), (t["a"], c["a"]), (t["cvar"], c["cvar"]),
                      (t["whiten_x"], c["whiten_x"]), (t["logc_x"], c["logc_x"])):
        scale = float(np.max(np.abs(want)))
        assert float(np.max(np.abs(got - want))) <= tol * kappa * scale
    assert np.all(np.tril(t["whiten"], -1) == 0.0) and np.all(np.tril(t["whiten_x"], -1) == 0.0)
    assert np.array_equal(t["mu_x"], mu[:, :dx]) and np.array_equal(t["mu_y"], mu[:, dx:]) and t["a"].shape == (3, 3, 3)
    assert all(v.flags.c_contiguous and v.dtype == np.float64 for v in t.values())
    wx, mx, cx = gmm.JointGMM(w, mu, cov, dx).marginal_x()
    assert np.array_equal(wx, w) and np.array_equal(mx, mu[:, :dx]) and np.array_equal(cx, cov[:, :dx, :dx])


def test_m_step_is_the_reference_m_step():
    from world import gmm

    rng = np.random.RandomState(2)
    w, mu, cov, _ = _model(seed=2)
    x, _ = ref.sample(w, mu, cov, 100, rng)
    gamma = rng.dirichlet(np.ones(3), size=100)
    s0, s1, s2, _, _, _ = ref.stats(x, gamma, mu)
    s2 = (s2 + np.transpose(s2, (0, 2, 1))) / 2  # (as wh_gmm_stats hands it over: both triangles the same bits)
    got = gmm.m_step(mu, s0, s1, s2, 1e-6)
    want = ref.m_step(mu, s0, s1, s2, 1e-6, ref.LD)
    for g, e, b in zip(got, want[:3], want[3:]):
        assert ref.compare(g, e, b + ref.U * np.abs(e))[0] <= 1
    assert np.array_equal(got[2], np.transpose(got[2], (0, 2, 1)))  # symmetric bit for bit


def test_npz_round_trip_is_bit_for_bit(tmp_path):
    from world import gmm

    w, mu, cov, dx = _model(seed=3)
    g = gmm.JointGMM(w, mu, cov, dx)
    path = str(tmp_path / "model.npz")
    g.save_npz(path)
    h = gmm.JointGMM.load_npz(path)
    assert h.dx == g.dx
    for a, b in ((g.weights, h.weights), (g.means, h.means), (g.covariances, h.covariances)):
        assert a.dtype == b.dtype == np.float64 and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_workspace_grouping():
    from world import gmm

    per = gmm.workspace_bytes(gmm.SPLIT_ROWS, 39, 5)
    assert per == 8 * 5 * 40 * 40
    assert gmm.plan_row_groups(0, 39, 5) == []
    assert gmm.plan_row_groups(10, 39, 5) == [(0, 10)]
    assert gmm.plan_row_groups(3 * 4096 + 3, 39, 5) == [(0, 3 * 4096 + 3)]
    assert gmm.plan_row_groups(3 * 4096 + 3, 39, 5, max_workspace_bytes=per) == [(0, 4096), (4096, 8192), (8192, 12288),
                                                                                 (12288, 12291)]
    assert gmm.plan_row_groups(3 * 4096 + 3, 39, 5, max_workspace_bytes=2 * per + 1) == [(0, 8192), (8192, 12291)]
    assert gmm.plan_row_groups(5000, 39, 5, max_workspace_bytes=1) == [(0, 4096), (4096, 5000)]  # one run at the least
    # the headline shape fits the default limit in one group, and every group stays under the limit
    assert gmm.plan_row_groups(2049024, 156, 32) == [(0, 2049024)]
    for r0, r1 in gmm.plan_row_groups(2049024, 156, 32, max_workspace_bytes=1 << 30):
        assert gmm.workspace_bytes(r1 - r0, 156, 32) <= 1 << 30 and r0 % gmm.SPLIT_ROWS == 0


def test_conversion_argument_checks():
    from world import dynamics, gmm

    w, mu, cov, _ = _model(m=2, d=8, seed=4)
    g = gmm.JointGMM(w, mu, cov, 4)
    win2 = dynamics.HTS_WINDOWS[:2]
    assert gmm.check_convert_args((7, 4), 7, g, "mlpg", win2)[2] == 2
    assert gmm.check_convert_args((7, 4), 7, g, "frame", [[1.0]])[2] == 4
    with pytest.raises(ValueError, match="mode"):
        gmm.check_convert_args((7, 4), 7, g, "best", win2)
    with pytest.raises(ValueError, match="frames"):  # row count against the batch
        gmm.check_convert_args((6, 4), 7, g, "mlpg", win2)
    with pytest.raises(ValueError, match="windows"):  # windows not matching the row width
        gmm.check_convert_args((7, 4), 7, g, "mlpg", dynamics.HTS_WINDOWS)
    with pytest.raises(ValueError, match="windows"):
        gmm.check_convert_args((7, 6), 7, g, "mlpg", win2)
    with pytest.raises(ValueError, match="static"):
        gmm.check_convert_args((7, 4), 7, g, "mlpg", [[0.0, 0.5, 0.0], [-0.5, 0.0, 0.5]])
    with pytest.raises(ValueError, match="columns"):
        gmm.check_limits(161, 2)
    with pytest.raises(ValueError, match="components"):
        gmm.check_limits(4, 65)


def test_facade_exposes_the_methods_and_refuses_devices():
    from world import gmm
    from world.main import World

    for name in ("fit_device", "posteriors_device", "convert_device", "convert_compact", "fit_compact"):
        assert callable(getattr(gmm, name))
    w, mu, cov, dx = _model()
    with pytest.raises(NotImplementedError):
        World().fit_conversion([{}], [{}], devices=[0, 1])
    with pytest.raises(NotImplementedError):
        World().convert_voice({}, gmm.JointGMM(w, mu, cov, dx), devices=[0])
    with pytest.raises(ValueError):
        World().fit_conversion([{}], [], n_components=2)
    with pytest.raises(ValueError, match="components"):
        World().fit_conversion([{}], [{}], n_components=65)
    with pytest.raises(ValueError, match="columns"):
        World().fit_conversion([{}], [{}], n_components=2, n0=42)  # 2 speakers x 2 windows x 41 = 164 columns


def test_product_imports_neither_scipy_nor_sklearn():
    src = open(os.path.join(ROOT, "python-world_amd", "world", "gmm.py")).read()
    assert not re.search(r"^\s*(from|import)\s+(scipy|sklearn)\b", src, flags=re.M)
