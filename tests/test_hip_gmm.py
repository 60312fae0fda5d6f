"""GPU: wh_gmm_estep, wh_gmm_stats and wh_gmm_convert through the C ABI on device tensors (csrc/wh_gmm.hip) against
tests/_gmm_reference.py: bit for bit where every partial sum is exact, within the bounds derived there from the
long-double operands otherwise.  exp and log in the E-step's reduction are the device library's (documented <= 1 ulp:
the constant F of the reference), not wh::fexp / wh::flog.

Worst error / bound ratios seen on an MI355X (printed by every run; a ratio above 1 is a finding about the kernel), over
(n_rows, d, M) = (129, 39, 5), (300, 156, 3), (40, 160, 64) with covariance condition numbers up to 1e6:
    ll 0.015          gamma 0.0011       rowll 1.4e-8 (the posteriors of these mixtures are nearly one-hot, s = 1 and
    s0 0.084          s1 0.14            s2 0.24       log s = 0 exactly; tests/test_hip_gmm_fit.py has the soft ones)
    convert, best component 0.12         convert, MMSE 0.039
    statistics over two splits + 3 rows: s0 0.0013, s1 0.0007, s2 0.0046; one group against three: every ratio the same
"""
import numpy as np
import pytest

import _gmm_cases as gc
import _gmm_reference as ref

pytestmark = pytest.mark.gpu

LD = ref.LD


@pytest.fixture(scope="module")
def rt():
    from world import _hip
    return _hip.Runtime.get()


# ---- exact ---------------------------------------------------------------------------------------------------------------
def test_integer_inputs_give_the_integer_results_bit_for_bit(rt):
    bad = []
    for shape in gc.exact_shapes():
        got, want = gc.run_exact(rt, shape), gc.exact_data(shape)
        for key in gc.EXACT_KEYS:
            if not gc.same_bits(got[key], want[key]):
                bad.append("%s %s: %d of %d differ" % (shape, key, int(np.sum(got[key] != want[key])), want[key].size))
    assert rt.take_flags() == [0] * 16
    assert bad == []


def test_s2_is_symmetric_bit_for_bit_and_stats_repeat(rt):
    for shape in gc.REAL_SHAPES + ((2 * gc.SPLIT_ROWS + 3, 17, 2),):
        if shape in gc.REAL_SHAPES:
            dat = gc.real_data(shape)
            x, gamma, mu = dat["x"], dat["gamma"], dat["mu"]
        else:
            rng = np.random.RandomState(9)
            x, gamma, mu = rng.standard_normal(shape[:2]), rng.dirichlet(np.ones(shape[2]), size=shape[0]), rng.standard_normal(shape[1:][::-1])
        a, b = gc.stats_all(rt, x, gamma, mu), gc.stats_all(rt, x, gamma, mu)
        for k in ("s0", "s1", "s2"):
            assert gc.same_bits(a[k], b[k]), (shape, k)
        assert gc.same_bits(a["s2"], np.ascontiguousarray(np.transpose(a["s2"], (0, 2, 1)))), shape


# ---- real data within the derived bounds -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", gc.REAL_SHAPES, ids=lambda s: "n%d-d%d-M%d" % s)
def test_real_data_within_the_derived_bounds(rt, shape):
    dat, got = gc.real_data(shape), gc.run_real(rt, shape)
    n, d, m = shape
    ll, bll = ref.loglik(dat["x"], dat["mu"], dat["whiten"], dat["logc"], LD)
    ref.check("ll %s" % (shape,), got["ll"], ll, bll)
    # the reduction over m on the device's own ll, so that the two stages' errors do not compound
    gamma, rowll, best, bg, br = ref.reduce(got["ll"], LD)
    ref.check("gamma %s" % (shape,), got["gamma"], gamma, bg)
    ref.check("rowll %s" % (shape,), got["rowll"], rowll, br)
    assert np.array_equal(got["best"], best) and got["best"].dtype == np.int32
    assert np.all(np.abs(np.sum(got["gamma"], axis=1) - 1.0) <= (m + 4) * 2.0 ** -52)
    s0, s1, s2, b0, b1, b2 = ref.stats(dat["x"], dat["gamma"], dat["mu"], LD, splits=(n + gc.SPLIT_ROWS - 1) // gc.SPLIT_ROWS)
    ref.check("s0 %s" % (shape,), got["s0"], s0, b0)
    ref.check("s1 %s" % (shape,), got["s1"], s1, b1)
    ref.check("s2 %s" % (shape,), got["s2"], s2, b2)
    xs = dat["x"][:, :dat["dx"]]
    out, bo = ref.convert_best(xs, dat["mu_x"], dat["a"], dat["mu_y"], dat["best"], LD)
    ref.check("convert-best %s" % (shape,), got["out_best"], out, bo)
    out, bo = ref.convert_mmse(xs, dat["mu_x"], dat["a"], dat["mu_y"], dat["gamma"], LD)
    ref.check("convert-mmse %s" % (shape,), got["out_mmse"], out, bo)
    assert rt.take_flags() == [0] * 16


def test_stats_over_several_splits_within_the_bound(rt):
    """Two splits + 3 rows of real data: the partial sums are combined in ascending order."""
    n, d, m = 2 * gc.SPLIT_ROWS + 3, 17, 2
    rng = np.random.RandomState(10)
    x, gamma, mu = 3.0 + rng.standard_normal((n, d)), rng.dirichlet(np.ones(m), size=n), 3.0 + 0.1 * rng.standard_normal((m, d))
    got = gc.stats_all(rt, x, gamma, mu)
    s0, s1, s2, b0, b1, b2 = ref.stats(x, gamma, mu, LD, splits=3)
    ref.check("s0 splits", got["s0"], s0, b0)
    ref.check("s1 splits", got["s1"], s1, b1)
    ref.check("s2 splits", got["s2"], s2, b2)


# ---- strides ---------------------------------------------------------------------------------------------------------------
def test_strides_and_nothing_else_read_or_written(rt):
    got = gc.run_strided(rt)
    assert bool(got["untouched"][0]), "a cell outside the outputs' rows was written"
    dense = gc.run_real(rt, gc.STRIDE_SHAPE)  # (NaN beside the rows would show in any result that read it)
    for key in ("ll", "gamma", "rowll", "best", "s0", "s1", "s2", "out_best", "out_mmse"):
        assert np.all(np.isfinite(got[key])), key
        assert gc.same_bits(got[key], dense[key]), key


# ---- independence ----------------------------------------------------------------------------------------------------------
def test_a_row_has_the_bits_of_the_same_row_computed_alone(rt):
    dat = gc.real_data((300, 156, 3))
    whole = gc.run_real(rt, (300, 156, 3))
    dx = dat["dx"]
    for row in (0, 137, 299):
        one = gc.estep_all(rt, dat["x"][row:row + 1], dat["mu"], dat["whiten"], dat["logc"])
        for k in ("ll", "gamma", "rowll", "best"):
            assert gc.same_bits(one[k], whole[k][row:row + 1]), (row, k)
        xs = np.ascontiguousarray(dat["x"][row:row + 1, :dx])
        assert gc.same_bits(gc.convert_all(rt, xs, dat["mu_x"], dat["a"], dat["mu_y"], best=dat["best"][row:row + 1])["out"],
                            whole["out_best"][row:row + 1])
        assert gc.same_bits(gc.convert_all(rt, xs, dat["mu_x"], dat["a"], dat["mu_y"], g=dat["gamma"][row:row + 1])["out"],
                            whole["out_mmse"][row:row + 1])


# ---- edges -----------------------------------------------------------------------------------------------------------------
def test_one_component_gives_gamma_one_and_rowll_ll(rt):
    dat = gc.real_data((129, 39, 5))
    got = gc.estep_all(rt, dat["x"], dat["mu"][:1], dat["whiten"][:1], dat["logc"][:1])
    assert np.all(got["gamma"] == 1.0) and gc.same_bits(got["rowll"], got["ll"][:, 0]) and np.all(got["best"] == 0)


def test_far_components_underflow_to_zero_and_ties_take_the_smaller_index(rt):
    one = np.ones((3, 1, 1))
    x = np.zeros((5, 1))
    got = gc.estep_all(rt, x, np.zeros((3, 1)), one, np.array([0.0, -1e4, 0.0]))
    assert np.all(got["gamma"][:, 1] == 0.0) and np.all(np.isfinite(got["gamma"])) and np.all(np.isfinite(got["rowll"]))
    assert np.all(got["gamma"][:, 0] == 0.5) and np.all(got["gamma"][:, 2] == 0.5) and np.all(got["best"] == 0)
    assert np.all(np.abs(got["rowll"] - np.log(2.0)) <= 2.0 ** -52)  # (log within one ulp)
    got = gc.estep_all(rt, x, np.zeros((3, 1)), one, np.array([-1.0, 2.0, 2.0]))
    assert np.all(got["best"] == 1)
    # wh_gmm_convert: a component index outside [0, M) selects nothing
    out = gc.convert_all(rt, np.ones((4, 2)), np.zeros((2, 2)), np.ones((2, 2, 3)), np.ones((2, 3)), best=np.array([0, 1, 2, -1]))["out"]
    assert np.array_equal(out, np.array([[3.0] * 3, [3.0] * 3, [0.0] * 3, [0.0] * 3]))


def test_a_nan_row_gives_nan_in_that_row_only(rt):
    dat = gc.real_data((129, 39, 5))
    clean = gc.run_real(rt, (129, 39, 5))
    x = np.array(dat["x"])
    x[77, 5] = np.nan
    got = gc.estep_all(rt, x, dat["mu"], dat["whiten"], dat["logc"])
    keep = np.arange(129) != 77
    for k in ("ll", "gamma", "rowll"):
        assert np.all(np.isnan(got[k][77])), k
        assert gc.same_bits(got[k][keep], clean[k][keep]), k
    assert 0 <= got["best"][77] < 5 and np.array_equal(got["best"][keep], clean["best"][keep])
    xs = np.ascontiguousarray(x[:, :dat["dx"]])
    for kw, key in (({"best": dat["best"]}, "out_best"), ({"g": dat["gamma"]}, "out_mmse")):
        out = gc.convert_all(rt, xs, dat["mu_x"], dat["a"], dat["mu_y"], **kw)["out"]
        assert np.all(np.isnan(out[77])) and gc.same_bits(out[keep], clean[key][keep]), key
    inf = np.array(dat["x"])
    inf[3, 0] = np.inf
    got = gc.estep_all(rt, inf, dat["mu"], dat["whiten"], dat["logc"])
    assert not np.any(np.isfinite(got["ll"][3])) and gc.same_bits(got["ll"][4:], clean["ll"][4:])
    assert rt.take_flags() == [0] * 16


def test_no_rows_is_no_error_and_wrong_arguments_fail_before_a_launch(rt):
    import torch
    from world import _hip

    mu, w, lc = rt.zeros((2, 3)), rt.zeros((2, 3, 3)), rt.zeros((2,))
    guard = torch.full((8,), gc.SENTINEL, dtype=torch.float64, device=rt.device)
    x0 = rt.zeros((1, 3))
    gc.raw_estep(rt, x0, mu, w, lc, guard.view(4, 2), guard.view(4, 2), guard, None, n=0)
    gc.raw_stats(rt, x0, rt.zeros((1, 2)), mu, guard[:2], guard[:6], guard, n=0)
    gc.raw_convert(rt, x0, mu, rt.zeros((2, 3, 2)), rt.zeros((2, 2)), guard.view(4, 2), g=rt.zeros((1, 2)), n=0)
    assert torch.all(guard == gc.SENTINEL)
    lib, ctx, st, p = rt.lib, rt.ctx, rt.stream(), rt.ptr
    big = rt.zeros((1, 161))
    bad = [
        lambda: lib.wh_gmm_estep(ctx, st, p(big), 1, 161, 161, 2, p(mu), p(w), p(lc), None, 2, None, 2, None, None),   # d
        lambda: lib.wh_gmm_estep(ctx, st, p(x0), 1, 3, 3, 65, p(mu), p(w), p(lc), None, 65, None, 65, None, None),     # M
        lambda: lib.wh_gmm_estep(ctx, st, p(x0), 1, 2, 3, 2, p(mu), p(w), p(lc), None, 2, None, 2, None, None),        # ldx < d
        lambda: lib.wh_gmm_estep(ctx, st, p(x0), 1, 3, 3, 2, p(mu), p(w), p(lc), p(guard), 1, None, 2, None, None),    # ldl < M
        lambda: lib.wh_gmm_estep(ctx, st, p(x0), 1, 3, 3, 2, p(mu), None, p(lc), None, 2, None, 2, None, None),        # null table
        lambda: lib.wh_gmm_estep(ctx, st, None, 1, 3, 3, 2, p(mu), p(w), p(lc), None, 2, None, 2, None, None),         # null x
        lambda: lib.wh_gmm_stats(ctx, st, p(x0), 1, 3, 3, 2, p(guard), 1, p(mu), p(guard), p(guard), p(guard)),        # ldg < M
        lambda: lib.wh_gmm_stats(ctx, st, p(x0), 1, 3, 3, 2, p(guard), 2, p(mu), p(guard), None, p(guard)),            # null s1
        lambda: lib.wh_gmm_stats(ctx, st, p(x0), 1, 3, 0, 2, p(guard), 2, p(mu), p(guard), p(guard), p(guard)),        # d = 0
        lambda: lib.wh_gmm_convert(ctx, st, p(x0), 1, 3, 3, 2, 2, p(mu), p(w), p(mu), None, None, 2, p(guard), 2),     # neither
        lambda: lib.wh_gmm_convert(ctx, st, p(x0), 1, 3, 3, 2, 2, p(mu), p(w), p(mu), p(lc), p(lc), 2, p(guard), 2),   # both
        lambda: lib.wh_gmm_convert(ctx, st, p(x0), 1, 3, 3, 2, 2, p(mu), p(w), p(mu), None, p(lc), 2, p(guard), 1),    # ldo < dy
        lambda: lib.wh_gmm_convert(ctx, st, p(x0), 1, 3, 3, 0, 2, p(mu), p(w), p(mu), None, p(lc), 2, p(guard), 2),    # dy = 0
        lambda: lib.wh_gmm_convert(ctx, st, p(x0), 1, 100, 100, 61, 2, p(mu), p(w), p(mu), None, p(lc), 2, p(guard), 61),  # dx + dy
        lambda: lib.wh_gmm_convert(ctx, st, p(x0), -1, 3, 3, 2, 2, p(mu), p(w), p(mu), None, p(lc), 2, p(guard), 2),   # n_rows < 0
    ]
    for i, call in enumerate(bad):
        assert call() != 0, i
        assert _hip.load_library().wh_last_error()
    torch.cuda.synchronize()
    assert torch.all(guard == gc.SENTINEL) and rt.take_flags() == [0] * 16


# ---- the workspace in groups ---------------------------------------------------------------------------------------------
def test_grouped_workspace_gives_the_regrouped_sum(rt):
    """stats_device and fit_device with a workspace limit of one run per call: the groups' results are added in group
    order.  Both forms are within B of the exact sums (B of tests/_gmm_reference.py with the splits of either form), so
    they differ by at most 2 B; one m_step later, to first order with a factor 2 for the rest,
        |d mu| <= 2 (2 B1 + 2 B0 |delta|) / nk,   |d Sigma| <= 2 (2 B2 + 2 B0 |s2 / nk|) / nk + 4 |delta| |d mu|."""
    from world import gmm

    n, d, m = 2 * gc.SPLIT_ROWS + 3, 8, 3
    rng = np.random.RandomState(11)
    w, mu, cov = ref.random_mixture(m, d, rng, 100.0)
    x, _ = ref.sample(w, mu, cov, n, rng)
    z = rt.to_device(x)
    init = gmm.JointGMM(w, mu, cov, 4)
    small = gmm.workspace_bytes(gc.SPLIT_ROWS, d, m)
    assert len(gmm.plan_row_groups(n, d, m, small)) == 3
    gamma = gmm.posteriors_device(rt, z, init)[0]
    mu_d = rt.to_device(mu)
    one = [t.cpu().numpy() for t in gmm.stats_device(rt, z, gamma, mu_d)]
    three = [t.cpu().numpy() for t in gmm.stats_device(rt, z, gamma, mu_d, max_workspace_bytes=small)]
    s = ref.stats(x, gamma.cpu().numpy(), mu, LD, splits=3)
    for k in range(3):
        ref.check("stats one-group", one[k], s[k], s[k + 3])
        ref.check("stats three-groups", three[k], s[k], s[k + 3])
    a, ha = gmm.fit_device(rt, z, 4, m, 1, init=init)
    b, hb = gmm.fit_device(rt, z, 4, m, 1, init=init, max_workspace_bytes=small)
    assert ha == hb  # (the E-step does not depend on the grouping)
    nk = s[0]
    delta = np.abs(s[1] / nk[:, None])
    b_mu = 2 * (2 * s[4] + 2 * s[3][:, None] * delta) / nk[:, None]
    b_cov = 2 * (2 * s[5] + 2 * s[3][:, None, None] * np.abs(s[2] / nk[:, None, None])) / nk[:, None, None] \
        + 4 * (delta[:, :, None] * b_mu[:, None, :] + delta[:, None, :] * b_mu[:, :, None])
    ref.check("regrouped means", b.means, a.means.astype(LD), b_mu)
    ref.check("regrouped covariances", b.covariances, a.covariances.astype(LD), b_cov)
    ref.check("regrouped weights", b.weights, a.weights.astype(LD), 4 * (s[3] / nk + ref.U) * a.weights)
