"""CPU: the reference of the GMM tests (tests/_gmm_reference.py) checked on its own — against identities in long double,
against scikit-learn where it imports, and its comparators against the mutants a kernel or a table could realise.

Bounds used here on top of the module's own.  kappa_m = cond_2(Sigma_m), computed in the test.
  * Tables from (w, mu, Sigma) in FP64 (any Cholesky, any triangular inverse): the factor's relative error is at most
    c d u kappa in norm (Higham, section 10.1: backward error gamma_(d+1) |L||L'|, times the condition number), and so is
    the inverse's; with c = 4 d:   |dW| <= EW = 4 d^2 u kappa ||W||_2 per entry, each log diag L moves by <= 4 d^2 u kappa.
  * scikit-learn evaluates z as x P - mu P (two products and a difference, not a product of the difference), so its
    evaluation error is relative to (|x| + |mu|) |W|, not to |x - mu| |W|:
        Bz_j = (d + 3) u sum_k (|x_k| + |mu_k|) |W_kj| + EW ||x - mu||_1
        B_ll = 0.5 sum_j (2 |z_j| Bz_j + Bz_j^2) + 0.5 (d + 2) u sum_j (|z_j| + Bz_j)^2 + 4 d^3 u kappa + u (|ll| + d log 2 pi)
    The FP64 reference (the product of the difference) is inside the same bound a fortiori.
  * Softmax: moving every ll_m by at most E moves log s by at most E and gamma_m by at most gamma_m (e^(2E) - 1):
        B_rowll = E + B_rowll(reduce),   B_gamma = gamma_m (e^(2E) - 1) + B_gamma(reduce),   E = max_m B_ll.
  * One EM step: with |d gamma_nm| <= G_nm, nk' = sum G / nk and e = x - mu_new,
        B_mu_i    = sum_n G |x_i - mu_i| / nk + 2 nk' |delta_i| + stats and m_step bounds / nk
        B_Sigma_ij = sum_n G |e_i e_j| / nk + 2 nk' |Sigma_ij| + 2 B_mu_i |..| ... (second order dropped into a factor 2)
    plus the evaluation error of the sums themselves, (n + 8) u sum gamma |e_i| |e_j| / nk, for scikit-learn's and for
    the reference's own order of summation.
"""
import numpy as np
import pytest

import _gmm_reference as ref

LD = ref.LD
U = ref.U


def _ld_inverse_spd(a):
    w = np.triu(ref.inv_lower(ref.cholesky(a, LD), LD).T)
    return w @ w.T


def test_conditional_tables_against_the_block_precision_identity():
    """Sigma_y|x = Lambda_yy^-1 and A = -Lambda_xy Lambda_yy^-1 with Lambda the inverse of the joint covariance: two
    independent routes in long double, agreeing to eps_LD * kappa."""
    rng = np.random.RandomState(1)
    for d, dx, cond in ((6, 3, 1e3), (8, 2, 1e6), (2, 1, 10.0), (9, 8, 1e4)):
        w, mu, cov = ref.random_mixture(3, d, rng, cond)
        t = ref.conditional(w, mu, cov, dx, LD)
        for k in range(3):
            kappa = np.linalg.cond(cov[k])
            lam = _ld_inverse_spd(cov[k].astype(LD))
            syx = _ld_inverse_spd(lam[dx:, dx:])
            a_id = -(lam[:dx, dx:] @ syx)
            tol = 64 * d * d * float(np.finfo(LD).eps) * kappa * kappa
            scale_a = float(np.max(np.abs(a_id))) + 1.0
            assert float(np.max(np.abs(t["a"][k] - a_id))) <= tol * scale_a, (d, dx, k)
            assert float(np.max(np.abs(t["cvar"][k] - np.diag(syx)))) <= tol * float(np.max(np.abs(np.diag(syx)))), (d, dx, k)
            assert np.all(t["cvar"][k] > 0)
        # the float64 tables against the long-double ones: 4 d^2 u kappa^2 (two solves), relative to the largest entry
        t64 = ref.conditional(w, mu, cov, dx, np.float64)
        for k in range(3):
            kappa = np.linalg.cond(cov[k][:dx, :dx])
            assert float(np.max(np.abs(t64["a"][k] - t["a"][k]))) <= 8 * d * d * U * kappa * (float(np.max(np.abs(t["a"][k]))) + 1.0)


def test_centred_statistics_and_m_step_against_the_textbook_sums():
    """stats about the current means + m_step equals the uncentred textbook estimate, in long double, for any centre."""
    rng = np.random.RandomState(2)
    w, mu, cov = ref.random_mixture(3, 5, rng, 1e3)
    x, _ = ref.sample(w, mu, cov, 300, rng)
    x += 50.0  # far from the origin: the uncentred sums cancel, the centred ones do not
    gamma = rng.dirichlet(np.ones(3), size=300)
    for centre in (mu + 50.0, np.zeros((3, 5)), x[:3]):
        s0, s1, s2, _, _, _ = ref.stats(x, gamma, centre, LD)
        w1, mu1, cov1, _, _, _ = ref.m_step(centre, s0, s1, s2, 1e-6, LD)
        w2, mu2, cov2 = ref.textbook_m_step(x, gamma, 1e-6, LD)
        eps = float(np.finfo(LD).eps)
        big = float(np.max(np.abs(x))) ** 2
        assert float(np.max(np.abs(w1 - w2))) <= 8 * eps
        assert float(np.max(np.abs(mu1 - mu2))) <= 1200 * eps * 60.0
        assert float(np.max(np.abs(cov1 - cov2))) <= 1200 * eps * big
    # and in float64 the centred form keeps what the uncentred one loses: within its own derived bound
    s0, s1, s2, b0, b1, b2 = ref.stats(x, gamma, mu + 50.0, LD)
    g0, g1, g2, _, _, _ = ref.stats(x, gamma, mu + 50.0, np.float64)
    assert ref.compare(g0, s0, b0)[0] <= 1 and ref.compare(g1, s1, b1)[0] <= 1 and ref.compare(g2, s2, b2)[0] <= 1


def _case(seed=3, m=3, d=6, n=200, cond=1e3):
    rng = np.random.RandomState(seed)
    w, mu, cov = ref.random_mixture(m, d, rng, cond)
    x, _ = ref.sample(w, mu, cov, n, rng)
    return w, mu, cov, x


def _chain_bounds(w, mu, cov, x):
    """Long-double ll / gamma / rowll from (w, mu, Sigma) and the bounds of the module docstring for an FP64 evaluation
    that builds its own tables."""
    m, d = mu.shape
    wl, lc = ref.prepare(w, mu, cov, LD)
    ll, _ = ref.loglik(x, mu, wl, lc, LD)
    bll = np.zeros(ll.shape, dtype=LD)
    xl, mul = x.astype(LD), mu.astype(LD)
    for k in range(m):
        kappa = LD(np.linalg.cond(cov[k]))
        ew = 4 * d * d * LD(U) * kappa * LD(np.linalg.norm(wl[k].astype(np.float64), 2))
        e = xl - mul[k]
        z = e @ wl[k]
        bz = LD((d + 3) * U) * ((np.abs(xl) + np.abs(mul[k])) @ np.abs(wl[k])) + ew * np.sum(np.abs(e), axis=1)[:, None]
        bll[:, k] = (np.sum(2 * np.abs(z) * bz + bz * bz, axis=1) + LD((d + 2) * U) * np.sum((np.abs(z) + bz) ** 2, axis=1)) / 2 \
            + 4 * d ** 3 * LD(U) * kappa + LD(U) * (np.abs(ll[:, k]) + d * np.log(2 * np.pi))
    gamma, rowll, best, bg, br = ref.reduce(ll, LD)
    e_max = np.max(bll, axis=1)
    return ll, bll, gamma, gamma * np.expm1(2 * e_max)[:, None] + bg, rowll, e_max + br, best


def test_float64_reference_is_within_the_chain_bound_of_the_long_double_one():
    w, mu, cov, x = _case()
    ll, bll, gamma, bg, rowll, br, best = _chain_bounds(w, mu, cov, x)
    w64, lc64 = ref.prepare(w, mu, cov)
    l64, _ = ref.loglik(x, mu, w64, lc64)
    g64, r64, b64, _, _ = ref.reduce(l64)
    assert ref.check("ll float64-reference", l64, ll, bll) <= 1
    assert ref.check("gamma float64-reference", g64, gamma, bg) <= 1
    assert ref.check("rowll float64-reference", r64, rowll, br) <= 1
    assert float(np.max(bll)) < 1e-6  # the bound says something
    assert np.array_equal(b64, best)


def test_score_samples_and_predict_proba_against_sklearn():
    mixture = pytest.importorskip("sklearn.mixture")
    w, mu, cov, x = _case()
    ll, bll, gamma, bg, rowll, br, _ = _chain_bounds(w, mu, cov, x)
    gm = mixture.GaussianMixture(n_components=3, covariance_type="full", weights_init=w, means_init=mu,
                                 precisions_init=np.linalg.inv(cov), reg_covar=1e-6, max_iter=1, tol=0.0)
    # (the fitted attributes set by hand: scoring under the given parameters, no step taken)
    gm.weights_, gm.means_, gm.covariances_ = w, mu, cov
    gm.precisions_cholesky_ = np.stack([np.linalg.inv(np.linalg.cholesky(c)).T for c in cov])
    assert ref.check("rowll sklearn.score_samples", gm.score_samples(x), rowll, br) <= 1
    assert ref.check("gamma sklearn.predict_proba", gm.predict_proba(x), gamma, bg) <= 1


def _step_bounds(w, mu, cov, x, reg):
    """One EM step in long double from (w, mu, Sigma), and the bounds of the module docstring for an FP64 step."""
    m, d = mu.shape
    n = len(x)
    _, _, gamma, bg, _, _, _ = _chain_bounds(w, mu, cov, x)
    s0, s1, s2, b0, b1, b2 = ref.stats(x, gamma, mu, LD)
    w1, mu1, cov1, bw, bmu, bcov = ref.m_step(mu, s0, s1, s2, reg, LD)
    nk = s0 + LD(10 * np.finfo(np.float64).eps)
    xl = x.astype(LD)
    ev = LD((n + 8) * U)
    b_mu, b_cov = np.zeros(mu.shape, dtype=LD), np.zeros(cov.shape, dtype=LD)
    for k in range(m):
        g, big_g = gamma[:, k], bg[:, k]
        nkp = np.sum(big_g) / nk[k]
        e0, e1 = np.abs(xl - mu[k].astype(LD)), np.abs(xl - mu1[k])
        b_mu[k] = 2 * ((big_g @ e0) / nk[k] + 2 * nkp * np.abs(mu1[k] - mu[k]) + ev * (g @ (np.abs(xl) + np.abs(mu[k]))) / nk[k]) + bmu[k]
        b_cov[k] = 2 * (((e1 * big_g[:, None]).T @ e1) / nk[k] + 2 * nkp * np.abs(cov1[k]) + ev * ((e1 * g[:, None]).T @ e1) / nk[k]
                        + 2 * np.add.outer(b_mu[k], b_mu[k]) * float(np.max(np.sqrt(np.abs(np.diag(cov1[k])))))) + bcov[k]
    b_w = 2 * (np.sum(bg, axis=0) / nk + LD((n + 8) * U)) * w1 + bw
    return (w1, mu1, cov1), (b_w, b_mu, b_cov)


def test_one_em_step_against_sklearn_and_the_float64_reference():
    w, mu, cov, x = _case(seed=4)
    reg = 1e-6
    (w1, mu1, cov1), (b_w, b_mu, b_cov) = _step_bounds(w, mu, cov, x, reg)
    # the float64 reference: tables, ll, gamma, centred statistics, m_step
    w64, lc64 = ref.prepare(w, mu, cov)
    g64 = ref.reduce(ref.loglik(x, mu, w64, lc64)[0])[0]
    s0, s1, s2, _, _, _ = ref.stats(x, g64, mu)
    rw, rmu, rcov, _, _, _ = ref.m_step(mu, s0, s1, s2, reg)
    assert ref.check("em-step weights float64-reference", rw, w1, b_w) <= 1
    assert ref.check("em-step means float64-reference", rmu, mu1, b_mu) <= 1
    assert ref.check("em-step covariances float64-reference", rcov, cov1, b_cov) <= 1
    assert float(np.max(b_cov)) < 1e-3 and float(np.max(b_mu)) < 1e-3  # (kappa up to 1e3 enters twice: still a check)
    mixture = pytest.importorskip("sklearn.mixture")
    import warnings
    gm = mixture.GaussianMixture(n_components=3, covariance_type="full", weights_init=w, means_init=mu,
                                 precisions_init=np.linalg.inv(cov), reg_covar=reg, max_iter=1, tol=0.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gm.fit(x)
    assert ref.check("em-step weights sklearn", gm.weights_, w1, b_w) <= 1
    assert ref.check("em-step means sklearn", gm.means_, mu1, b_mu) <= 1
    assert ref.check("em-step covariances sklearn", gm.covariances_, cov1, b_cov) <= 1


def test_comparators_reject_the_mutants():
    """Each way a kernel or a table could be wrong is outside the bounds the GPU tests use; the float64 reference is
    inside them."""
    rng = np.random.RandomState(5)
    m, d, dx, n = 3, 6, 3, 64
    w, mu, cov = ref.random_mixture(m, d, rng, 1e3)
    x, _ = ref.sample(w, mu, cov, n, rng)
    whiten, logc = ref.prepare(w, mu, cov)
    ll, bll = ref.loglik(x, mu, whiten, logc, LD)
    assert ref.compare(ref.loglik(x, mu, whiten, logc)[0], ll, bll)[0] <= 1
    # a dropped -sum log diag L
    bad_logc = ref.prepare(w, mu, cov, drop_logdet=True)[1]
    assert ref.compare(ref.loglik(x, mu, whiten, bad_logc)[0], ll, bll)[0] > 1
    # gamma not normalised
    l64 = ref.loglik(x, mu, whiten, logc)[0]
    gamma, rowll, best, bg, br = ref.reduce(l64, LD)
    good = ref.reduce(l64)
    assert ref.compare(good[0], gamma, bg)[0] <= 1 and ref.compare(good[1], rowll, br)[0] <= 1
    assert ref.compare(ref.reduce(l64, normalise=False)[0], gamma, bg)[0] > 1
    # best taking the last instead of the first maximum
    tie = l64.copy()
    tie[:, 2] = tie[:, 0] = np.max(tie, axis=1) + 1.0
    assert np.array_equal(ref.reduce(tie)[2], ref.reduce(tie, LD)[2]) and np.all(ref.reduce(tie)[2] == 0)
    assert not np.array_equal(ref.reduce(tie, last_max=True)[2], ref.reduce(tie, LD)[2])
    # statistics accumulated about the wrong component's mean
    s = ref.stats(x, good[0], mu, LD)
    ok = ref.stats(x, good[0], mu)
    wrong = ref.stats(x, good[0], mu, centre_shift=1)
    for i in (1, 2):
        assert ref.compare(ok[i], s[i], s[i + 3])[0] <= 1
        assert ref.compare(wrong[i], s[i], s[i + 3])[0] > 1
    assert ref.compare(ok[0], s[0], s[3])[0] <= 1
    # A_m transposed
    t = ref.conditional(w, mu, cov, dx)
    tt = ref.conditional(w, mu, cov, dx, transpose_a=True)
    out, bnd = ref.convert_best(x[:, :dx], t["mu_x"], t["a"], t["mu_y"], good[2], LD)
    assert ref.compare(ref.convert_best(x[:, :dx], t["mu_x"], t["a"], t["mu_y"], good[2])[0], out, bnd)[0] <= 1
    assert ref.compare(ref.convert_best(x[:, :dx], t["mu_x"], tt["a"], t["mu_y"], good[2])[0], out, bnd)[0] > 1
    o2, b2 = ref.convert_mmse(x[:, :dx], t["mu_x"], t["a"], t["mu_y"], good[0], LD)
    assert ref.compare(ref.convert_mmse(x[:, :dx], t["mu_x"], t["a"], t["mu_y"], good[0])[0], o2, b2)[0] <= 1
    assert ref.compare(ref.convert_mmse(x[:, :dx], t["mu_x"], tt["a"], t["mu_y"], good[0])[0], o2, b2)[0] > 1


def test_conversion_modes_of_the_reference_agree_where_they_must():
    """With one component the three modes differ only by MLPG; with unit-variance-free rows 'frame' is the static part of
    the best component's mean, and 'mmse' with a one-hot posterior equals it."""
    import _mlpg_reference as mref

    rng = np.random.RandomState(6)
    win = mref.HTS_WINDOWS[:2]
    w, mu, cov = ref.random_mixture(1, 8, rng, 100.0)
    lens = (7, 12)
    stat = np.cumsum(rng.standard_normal((sum(lens), 2)), axis=0)
    x = np.concatenate([mref.delta_features(stat[a:b], win) for a, b in ((0, 7), (7, 19))])
    frame = ref.convert(x, w, mu, cov, 4, "frame", win, lens)
    mmse = ref.convert(x, w, mu, cov, 4, "mmse", win, lens)
    mlpg = ref.convert(x, w, mu, cov, 4, "mlpg", win, lens)
    assert frame.shape == mmse.shape == mlpg.shape == (19, 2)
    assert np.max(np.abs(frame - mmse)) <= 1e-13 * (1 + np.max(np.abs(frame)))
    assert np.all(np.isfinite(mlpg)) and not np.array_equal(mlpg, frame)
