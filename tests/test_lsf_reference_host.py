"""CPU: the reference of the line-spectral-frequency kernels (tests/_lsf_reference.py) against independent arithmetic on
every frame of the two committed spectrogram fixtures at p in {2, 4, 10, 24, 40, 64}: its frequencies against
mpmath.polyroots of P and Q at 60 digits built from the same double predictor, within the bound its docstring derives;
its Levinson recursion against a long-double elimination of the Toeplitz system, the bound scaled by the condition
number; its product-form envelope against E / |rfft(a)|^2 in long double; the grid refinement on predictors built from
chosen frequencies; the degenerate rows; and three mutants of the reference, each caught by the mpmath comparison.
The polyroots runs (2 x 342 frames x 6 orders) are spread over worker processes."""
import functools
import multiprocessing
import os

import numpy as np
import pytest

import _lsf_cases as lc
import _lsf_reference as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("golden_syn16k", "golden_syn48k")
ORDERS = (2, 4, 10, 24, 40, 64)
LD = np.longdouble


@functools.lru_cache(maxsize=None)
def spectrogram(name):
    s = np.ascontiguousarray(np.load(os.path.join(GOLDEN, name + ".npz"))["ct_spectrogram"].T)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def predictors(name, p):
    a, e, refl, bad = ref.levinson(ref.autocorr(spectrogram(name), p), p)
    assert not bad.any()
    return a, e


def exact_frequencies(a_row):
    """(wP, wQ): the angles in (0, pi) of the unit-circle roots of P = A + z^-(p+1) A~ and Q = A - z^-(p+1) A~, ascending,
    by mpmath.polyroots at 60 digits (started from numpy.roots); the polynomials are formed exactly from the doubles."""
    import mpmath

    p = len(a_row) - 1
    with mpmath.workdps(60):
        a = [mpmath.mpf(float(v)) for v in a_row] + [mpmath.mpf(0)]
        out = []
        for sign in (1, -1):
            poly = [a[i] + sign * a[p + 1 - i] for i in range(p + 2)]
            init = [mpmath.mpc(complex(z)) for z in np.roots([float(c) for c in poly])]
            roots = mpmath.polyroots(poly, maxsteps=100, extraprec=60, roots_init=init)
            tiny = mpmath.mpf(10) ** -40
            w = sorted(mpmath.arg(z) for z in roots if abs(abs(z) - 1) < tiny and z.imag > tiny)
            out.append([float(v) for v in w])
    return out


@pytest.fixture(scope="module")
def pool():
    with multiprocessing.get_context("spawn").Pool(min(8, os.cpu_count() or 1)) as p:
        yield p


_EXACT = {}


def exact(pool, name, p):
    """(wP [F][m], wQ [F][m]) of every frame of a fixture, computed once; a frame with another count raises."""
    if (name, p) not in _EXACT:
        a, _ = predictors(name, p)
        res = pool.map(exact_frequencies, list(a), chunksize=4)
        assert all(len(wp) == p // 2 and len(wq) == p // 2 for wp, wq in res), "P or Q has roots off the unit circle"
        _EXACT[(name, p)] = (np.array([r[0] for r in res]), np.array([r[1] for r in res]))
    return _EXACT[(name, p)]


def slope(c, w):
    """|f'(x)| of the series sum c_k T_k(x) at x = cos w, rows side by side, in long double: T_k' = k sin(k w) / sin w."""
    k = np.arange(c.shape[1], dtype=LD)[None, :, None]
    wl = w.astype(LD)[:, None, :]
    return np.abs(np.sum(c.astype(LD)[:, :, None] * k * np.sin(k * wl), axis=1) / np.sin(wl[:, 0, :]))


def worst_ratio(x, level, a, w_p, w_q):
    """max over frames and roots of |w_ref - w_exact| / bound, or inf where the reference lacks a root."""
    if np.any(level == 0) or np.any(np.isnan(x)):
        return np.inf
    cp, cq = ref.chebyshev_series(a)
    worst = 0.0
    with np.errstate(invalid="ignore"):
        w_ref = np.arccos(x)
    for c, w_exact, got in ((cp, w_p, w_ref[:, 0::2]), (cq, w_q, w_ref[:, 1::2])):
        d = slope(c, w_exact).astype(np.float64)
        for f in range(len(a)):
            bound = ref.root_bound(c[f], w_exact[f], d[f])
            worst = max(worst, float(np.max(np.abs(got[f] - w_exact[f]) / bound)))
    return worst


# ---- a. the frequencies against mpmath -------------------------------------------------------------------------------
@pytest.mark.parametrize("p", ORDERS)
@pytest.mark.parametrize("name", FIXTURES)
def test_frequencies_against_polyroots(pool, name, p):
    a, _ = predictors(name, p)
    w_p, w_q = exact(pool, name, p)
    x, level = ref.lsf_from_lpc(a)
    assert np.all(level > 0) and not np.isnan(x).any()  # the same number of roots: p / 2 of each, every frame
    assert np.all(np.diff(x, axis=1) < 0)
    err = max(float(np.max(np.abs(np.arccos(x[:, 0::2]) - w_p))), float(np.max(np.abs(np.arccos(x[:, 1::2]) - w_q))))
    ratio = worst_ratio(x, level, a, w_p, w_q)
    print("%s p=%d: worst |w_ref - w_exact| %.3g rad, worst error / bound %.3g" % (name, p, err, ratio))
    assert ratio <= 1.0


# ---- b. mutants ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", ["deflation_sign", "wrong_half", "swapped_interlace"])
def test_the_comparison_catches_a_wrong_reference(pool, mutant):
    """A wrong sign in P's deflation, a bisection that keeps the wrong half, P's and Q's roots interlaced the other way
    round: each is far outside the bound (p = 24 on the 16 kHz fixture; the exact roots are the ones of the test above)."""
    name, p = FIXTURES[0], 24
    a, _ = predictors(name, p)
    w_p, w_q = exact(pool, name, p)
    x, level = ref.lsf_from_lpc(a, mutant=mutant)
    assert worst_ratio(x, level, a, w_p, w_q) > 1e3
    assert worst_ratio(*ref.lsf_from_lpc(a), a, w_p, w_q) <= 1.0


# ---- c. Levinson against a long-double elimination -------------------------------------------------------------------
def toeplitz_solve_ld(r, p):
    """The solutions of T a = -r[1:] (T[i][j] = r[|i - j|]) by Gauss-Jordan elimination in long double, frames side by
    side; and T."""
    idx = np.abs(np.arange(p)[:, None] - np.arange(p)[None, :])
    t = r.astype(LD)[:, idx]
    m = np.concatenate([t, -r.astype(LD)[:, 1:p + 1, None]], axis=2)
    for i in range(p):
        m[:, i, :] = m[:, i, :] / m[:, i, i][:, None].copy()
        for j in range(p):
            if j != i:
                m[:, j, :] -= m[:, j, i][:, None].copy() * m[:, i, :]
    return m[:, :, p], t


@pytest.mark.parametrize("p", ORDERS)
@pytest.mark.parametrize("name", FIXTURES)
def test_levinson_against_long_double_elimination(name, p):
    """|a - a_exact| <= 4 (p + 1)^2 u kappa(T) max(1, max|a|): the recursion's (p + 1)^2 / 2 multiply-adds with a factor 8
    for the two operations and the accumulation of the orders, times the sensitivity of the system; the gain against
    r[0] + sum a[i] r[i] with the same bound scaled by sum |r|."""
    r = ref.autocorr(spectrogram(name), p)
    a, e, refl, bad = ref.levinson(r, p)
    assert not bad.any() and np.all(np.abs(refl) < 1) and np.all(a[:, 0] == 1.0) and np.array_equal(refl[:, -1], a[:, -1])
    want, t = toeplitz_solve_ld(r, p)
    kappa = np.array([np.linalg.cond(m.astype(np.float64)) for m in t])
    bound = 4 * (p + 1) ** 2 * ref.U * kappa * np.maximum(1.0, np.max(np.abs(a), axis=1))
    err = np.max(np.abs(a[:, 1:] - want), axis=1).astype(np.float64)
    e_want = r[:, 0].astype(LD) + np.sum(want * r[:, 1:p + 1].astype(LD), axis=1)
    e_err = np.abs(e - e_want).astype(np.float64)
    e_bound = bound * np.sum(np.abs(r[:, :p + 1]), axis=1)
    print("%s p=%d: kappa up to %.3g, worst error / bound %.3g (a), %.3g (E)"
          % (name, p, kappa.max(), np.max(err / bound), np.max(e_err / e_bound)))
    assert np.all(err <= bound) and np.all(e_err <= e_bound)


# ---- d. the product form against the transform of the predictor ------------------------------------------------------
@pytest.mark.parametrize("p", ORDERS)
@pytest.mark.parametrize("name", FIXTURES)
def test_envelope_against_the_transform_of_the_predictor(name, p):
    """E / |A(e^jw)|^2 on the fixture's own bins, A evaluated as a long-double sum.  The product form's own rounding is
    2 (p + 4) u; a root it is given is within dx_i of the exact one, which moves the factor 2 c - 2 x_i by at most
    dx_i / |c - x_i| of itself, twice in the square — so the tolerance is 2 (p + 4) u + the sum over the roots of
    2 dx_i / |c - x_i|, with dx_i = sin w_i times the reference's derived bound on its frequencies (root_bound)."""
    a, e = predictors(name, p)
    k_bins = spectrogram(name).shape[1]
    x, level = ref.lsf_from_lpc(a)
    got = ref.envelope(e, x, k_bins)
    w = (np.arccos(LD(-1)) * np.arange(k_bins, dtype=LD) / (k_bins - 1))[None, :, None]
    n = np.arange(p + 1, dtype=LD)[None, None, :]
    al = a.astype(LD)[:, None, :]
    re, im = np.sum(al * np.cos(w * n), axis=2), np.sum(al * np.sin(w * n), axis=2)
    want = e.astype(LD)[:, None] / (re * re + im * im)
    cp, cq = ref.chebyshev_series(a)
    w_ref = np.arccos(x)
    dx = np.empty_like(x)
    for c, cols in ((cp, slice(0, None, 2)), (cq, slice(1, None, 2))):
        d = slope(c, w_ref[:, cols]).astype(np.float64)
        for f in range(len(a)):
            dx[f, cols] = ref.root_bound(c[f], w_ref[f, cols], d[f]) * np.sin(w_ref[f, cols])
    dist = np.abs(ref.bin_table(k_bins)[None, :, None] - x[:, None, :])
    tol = 2 * (p + 4) * ref.U + np.sum(2 * dx[:, None, :] / dist, axis=2)
    rel = np.abs(got - want) / want
    print("%s p=%d: worst relative difference %.3g, worst difference / tolerance %.3g"
          % (name, p, float(rel.max()), float(np.max(rel / tol))))
    assert np.all(rel <= tol)


def test_table_of_distortions():
    """The figures of the issue's table, from the reference alone."""
    for name, p, db in (("golden_syn16k", 24, 2.158), ("golden_syn16k", 40, 1.559), ("golden_syn16k", 64, 0.984),
                        ("golden_syn48k", 40, 3.301), ("golden_syn48k", 64, 2.771)):
        spec = spectrogram(name)
        rows, level, bad = ref.lsf_rows(ref.autocorr(spec, p), p)
        assert not bad.any()
        assert abs(ref.lsd_db(ref.ilsf_rows(rows, spec.shape[1]), spec) - db) < 5e-4


# ---- e. grid refinement ----------------------------------------------------------------------------------------------
def test_grid_refinement_levels():
    """Predictors from chosen frequencies (expanded in mpmath, rounded once): two of P's roots in one cell of every grid
    coarser than the level named, on either side of one of its points; the last pair shares a cell of the finest grid."""
    a, levels, w = lc.refinement_predictors()
    x, level = lc.refinement_reference()
    assert level.tolist() == levels.tolist() == [256, 512, 1024, 4096, 0]
    assert np.all(np.isnan(x[4])) and not np.isnan(x[:4]).any()
    # found roots are the chosen frequencies, to the sensitivity of close roots to the rounding of a (1e-16 / gap)
    for i in range(4):
        assert np.max(np.abs(np.arccos(x[i]) - w[i])) < 1e-11
    # the levels are the grid's doing: the same predictors searched on the finest level only lose nothing but the last
    for i, g in enumerate((256, 512, 1024, 4096)):
        cells = np.floor(w[i] * g / np.pi)
        for coarser in (c for c in (256, 512, 1024, 2048) if c < g):
            cc = np.floor(w[i][0::2] * coarser / np.pi)
            assert len(set(cc)) < len(cc), (g, coarser)  # two of P's roots share a cell there
        assert len(set(cells[0::2])) == len(cells[0::2]) and len(set(cells[1::2])) == len(cells[1::2])


def test_a_frame_does_not_depend_on_its_neighbours():
    a, _, _ = lc.refinement_predictors()
    x, level = lc.refinement_reference()
    for i in range(len(a)):
        xi, li = ref.lsf_from_lpc(a[i:i + 1])
        assert lc.same_bits(xi[0], x[i]) and li[0] == level[i]


# ---- f. degenerate rows ----------------------------------------------------------------------------------------------
def test_degenerate_rows():
    p = 24
    r, odd = lc.degenerate_rows(p)
    want = lc.stages(r, p, 129)
    flagged = sorted(i for i, kind in odd.items() if kind != "zero")
    assert np.nonzero(want["bad"])[0].tolist() == flagged
    assert np.all(np.isnan(want["a"][flagged])) and np.all(np.isnan(want["e"][flagged]))
    assert np.all(np.isnan(want["refl"][flagged])) and np.all(np.isnan(want["x"][flagged]))
    assert np.all(want["level"][flagged] == 0)
    # the all-zero row: A = 1, E = 0, its frequencies those of 1 +- z^-(p+1): equally spaced, and an envelope of zeros
    assert want["a"][3].tolist() == [1.0] + [0.0] * p and want["e"][3] == 0.0 and not want["bad"][3]
    assert np.allclose(np.arccos(want["x"][3]), np.pi * (np.arange(p) + 1) / (p + 1), rtol=0, atol=1e-14)
    assert np.all(want["env"][3] == 0.0)
    # clean rows are what they are alone
    keep = np.array([i for i in range(len(r)) if i not in odd])
    alone = lc.stages(r[keep], p, 129)
    for key in lc.KEYS:
        assert lc.same_bits(alone[key], want[key][keep]), key
    rows, level, bad = ref.lsf_rows(r, p)
    assert rows[3, 0] == -np.inf and np.nonzero(bad)[0].tolist() == flagged


def test_odd_and_large_orders_are_refused():
    for p in (1, 3, 25, 66):
        with pytest.raises(ValueError):
            ref.lsf_from_lpc(np.ones((1, p + 1)))


def test_repair():
    w = np.array([[0.5, 0.4, 0.4, 3.2, -1.0, 1.0], [0.1, 0.2, 0.3, 0.4, 0.5, 0.6]])
    fixed = ref.repair(w, 0.01)
    assert np.all(np.diff(fixed, axis=1) >= 0.01 - 1e-15) and fixed.min() >= 0.01 and fixed.max() <= np.pi - 0.01
    assert np.array_equal(fixed[1], w[1]) and np.array_equal(ref.repair(w, 0.0), w)
