"""CPU: tests/_mlpg_reference.py, the contract the device is held to, measured against things that are not it: the dense
normal equations built in long double, the residual of its own solution under a rounding bound counted from the
operations, scipy.linalg.solveh_banded under the same criterion, np.correlate, the round trip through
the features, and the smoothing a tight delta variance must produce.  The comparators used here and on the device are
then shown to reject four near-misses of the contract."""
import numpy as np
import pytest

import _mlpg_cases as mc
import _mlpg_reference as ref

LD = np.longdouble
LENGTHS = {half: tuple(sorted({1, 2, 3, 2 * half, 2 * half + 1, 4 * half + 1, 65, 300})) for half in (1, 2)}
D = 3  # columns per case: independent systems side by side


def _inputs(T, half, seed, uniform):
    win = mc.WINDOWS[half][:3]
    rng = np.random.RandomState(seed * 1000 + T)
    x = np.cumsum(rng.randn(T, D), axis=0)
    mean = ref.delta_features(x, win) + 0.1 * rng.randn(T, 3 * D)
    var = np.full(3 * D, 0.37) if uniform else 10.0 ** rng.uniform(-8, 8, size=(T, 3 * D))
    return win, x, mean, var


def _dense(win, mean, var, col):
    """sum W' P W [T][T], sum W' P mu [T] and the sums of the terms' magnitudes, in long double, for column ``col``."""
    win = np.asarray(win, dtype=np.float64)
    T = len(mean)
    var = np.broadcast_to(var, mean.shape)
    R, r, Ra, ra = np.zeros((T, T), LD), np.zeros(T, LD), np.zeros((T, T), LD), np.zeros(T, LD)
    for w in range(len(win)):
        W = ref.dense_w(win, T, w)
        p = LD(1) / var[:, w * D + col].astype(LD)
        mu = mean[:, w * D + col].astype(LD)
        R += W.T @ (p[:, None] * W)
        Ra += np.abs(W).T @ (p[:, None] * np.abs(W))
        r += W.T @ (p * mu)
        ra += np.abs(W).T @ (p * np.abs(mu))
    return R, r, Ra, ra


CASES = [(half, T, uniform) for half in (1, 2) for T in LENGTHS[half] for uniform in (False, True)]
IDS = ["L=%d T=%d %s" % (h, T, "uniform" if u else "16 decades") for h, T, u in CASES]


# ---- a. the normal equations -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half,T,uniform", CASES, ids=IDS)
def test_normal_equations_equal_the_dense_ones_within_their_rounding(half, T, uniform):
    """An entry is a sum of at most n = n_win (2L + 1) terms, each two products of a once-rounded precision: three
    roundings per term and at most n - 1 additions on top — gamma_(n+2) times the sum of the terms' magnitudes; the long
    double side adds its own n + 3 roundings at 2^-64."""
    win, _, mean, var = _inputs(T, half, 1, uniform)
    Rb, r = ref.normal_equations(mean, var, win)
    n = 3 * (2 * half + 1)
    g = ref.gamma(n + 2) + (n + 3) * np.finfo(LD).eps
    for col in range(D):
        R, rr, Ra, ra = _dense(win, mean, var, col)
        assert np.all(np.abs(ref.band_to_dense(Rb[:, :, col]) - R) <= g * Ra)
        assert np.all(np.abs(r[:, col].astype(LD) - rr) <= g * ra)
        outside = np.abs(np.subtract.outer(np.arange(T), np.arange(T))) > 2 * half
        assert np.all(R[outside] == 0)


# ---- b. the solution ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half,T,uniform", CASES, ids=IDS)
def test_solution_by_its_residual_and_against_scipy(half, T, uniform):
    """|R c - r| <= gamma_k (|L||D||L'||c| + |r|) component by component with k = 3 B + 7 (derived in DESIGN section 15),
    for the reference's solution and for scipy.linalg.solveh_banded's of the same banded system; every pivot positive."""
    from scipy.linalg import solveh_banded

    win, _, mean, var = _inputs(T, half, 2, uniform)
    Rb, r = ref.normal_equations(mean, var, win)
    c, dv, lm = ref.ldl_solve(Rb, r)
    assert np.all(dv > 0) and np.all(np.isfinite(c))
    k = ref.residual_ops(2 * half)
    for col in range(D):
        res, bound = ref.residual_and_bound(Rb[:, :, col], r[:, col], c[:, col], dv[:, col], lm[:, :, col], k)
        assert np.all(res <= bound), float(np.max(res / bound))
        ab = np.ascontiguousarray(Rb[:, :min(2 * half, T - 1) + 1, col].T)  # lower form: ab[k][t] = R[t+k][t]
        cs = solveh_banded(ab, r[:, col], lower=True)
        res_s, bound_s = ref.residual_and_bound(Rb[:, :, col], r[:, col], cs, dv[:, col], lm[:, :, col], k)
        assert np.all(res_s <= bound_s), float(np.max(res_s / bound_s))


# ---- c. the features ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", (0, 1, 2))
def test_features_equal_np_correlate_on_integers(half):
    win = mc.WINDOWS[half]
    iwin = tuple(tuple(float(round(8 * t)) for t in w) for w in win[1:])
    static = tuple(1.0 if a == half else 0.0 for a in range(2 * half + 1))
    windows = (static,) + iwin
    rng = np.random.RandomState(half)
    for T in (1, 2, 3, 4, 5, 9, 65):
        x = rng.randint(-50, 50, size=(T, 4)).astype(np.float64)
        y = ref.delta_features(x, windows)
        assert y.shape == (T, len(windows) * 4)
        for w, taps in enumerate(windows):
            for d in range(4):
                full = np.correlate(np.concatenate([np.zeros(half), x[:, d], np.zeros(half)]), np.asarray(taps), "valid")
                assert y[:, w * 4 + d].tobytes() == full.tobytes()
                if T >= len(taps):  # ('same' centres on the longer argument: the signal, from this length on)
                    assert y[:, w * 4 + d].tobytes() == np.correlate(x[:, d], np.asarray(taps), "same").tobytes()


@pytest.mark.parametrize("half,T", [(h, T) for h in (1, 2) for T in (1, 2, 5, 65, 300)])
def test_unit_variances_give_the_track_back(half, T):
    """c solves R c = r^ where r^ is the rounded W' y^ of the rounded features y^ = W x.  With E the residual bound of
    the solve and F the rounding of r^ against R x, |c - x| <= |R^-1| (E + F) <= ||R^-1|| (max E + max F): the residual
    bound times the condition number, both computed here.  F: a feature is 2L + 1 products and 2L additions (gamma_(2L+1)
    of sum |w||x|), an entry of r^ and of R another n + 2 roundings each."""
    win = mc.WINDOWS[half][:3]
    rng = np.random.RandomState(T)
    x = np.cumsum(rng.randn(T, D), axis=0)
    y = ref.delta_features(x, win)
    Rb, r = ref.normal_equations(y, np.ones(3 * D), win)
    c, dv, lm = ref.ldl_solve(Rb, r)
    n = 3 * (2 * half + 1)
    for col in range(D):
        _, bound = ref.residual_and_bound(Rb[:, :, col], r[:, col], c[:, col], dv[:, col], lm[:, :, col], ref.residual_ops(2 * half))
        R = ref.band_to_dense(Rb[:, :, col])
        absW = sum(np.abs(ref.dense_w(np.asarray(win), T, w)) for w in range(3))
        F = ref.gamma(2 * (n + 2) + 2 * half + 1) * (absW.T @ (absW @ np.abs(x[:, col]).astype(LD)))
        inv_norm = np.max(np.sum(np.abs(np.linalg.inv(R.astype(np.float64))), axis=1))
        cond = inv_norm * np.max(np.sum(np.abs(R), axis=1))
        limit = inv_norm * (np.max(bound) + np.max(F))
        err = np.max(np.abs(c[:, col] - x[:, col]))
        assert err <= limit, (float(err), float(limit), float(cond))
        assert limit < 1e-9 * max(1.0, np.max(np.abs(x[:, col])))  # (the bound itself says something)


def test_tight_delta_variances_smooth_a_noisy_track():
    rng = np.random.RandomState(7)
    T = 200
    smooth = np.sin(np.arange(T) / 15.0)[:, None] * np.ones((1, 2))
    mean = np.zeros((T, 6))
    mean[:, :2] = smooth + 0.2 * rng.randn(T, 2)
    mean[:, 2:] = ref.delta_features(smooth, ref.HTS_WINDOWS)[:, 2:]
    var = np.concatenate([np.full(2, 1.0), np.full(4, 1e-3)])
    c, piv = ref.mlpg(mean, var, ref.HTS_WINDOWS)
    rough = lambda v: np.sum(np.diff(v, 2, axis=0) ** 2, axis=0)  # noqa: E731
    assert np.all(piv > 0)
    assert np.all(rough(c) < 0.01 * rough(mean[:, :2]))
    assert np.all(np.mean((c - smooth) ** 2, axis=0) < 0.25 * np.mean((mean[:, :2] - smooth) ** 2, axis=0))


# ---- d. the comparators reject near-misses -------------------------------------------------------------------------------
def _features_clamped(x, windows):
    """A dropped edge tap put back: the index clamped to the utterance instead."""
    win, L = ref.check_windows(windows)
    T, Dx = x.shape
    y = np.zeros((T, len(win) * Dx))
    for w in range(len(win)):
        for s in range(T):
            acc = np.zeros(Dx)
            for a in range(-L, L + 1):
                acc = acc + win[w][a + L] * x[min(max(s + a, 0), T - 1)]
            y[s, w * Dx:(w + 1) * Dx] = acc
    return y


def test_comparators_reject_near_misses():
    win = ref.HTS_WINDOWS
    rng = np.random.RandomState(11)
    T = 40
    x = rng.randint(-50, 50, size=(T, D)).astype(np.float64)
    want = ref.delta_features(x, win)
    assert mc.same_bits(want, ref.delta_features(x, win))
    # a dropped edge tap put back
    assert not mc.same_bits(want, _features_clamped(x, win))
    # windows applied in the wrong order
    assert not mc.same_bits(want, ref.delta_features(x, (win[0], win[2], win[1])))
    # k and -k swapped in an asymmetric window
    asym = mc.ASYMMETRIC
    flipped = (asym[0], asym[1][::-1])
    assert not mc.same_bits(ref.delta_features(x, asym), ref.delta_features(x, flipped))
    # the same three against the dense normal equations: the bound of test a refuses each
    mean = want + 0.1 * rng.randn(T, 3 * D)
    var = 10.0 ** rng.uniform(-2, 2, size=(T, 3 * D))
    g = ref.gamma(11) + 12 * np.finfo(LD).eps

    def r_fits(mean_used, win_ref, win_dense, clamp=False):
        Rb, r = ref.normal_equations(mean_used, var, win_ref)
        R, rr, Ra, ra = _dense(win_dense, mean, var, 0)
        if clamp:  # the dense side built with the clamped W
            R, rr = np.zeros((T, T), LD), np.zeros(T, LD)
            for w in range(3):
                W = np.zeros((T, T), LD)
                for s in range(T):
                    for a in (-1, 0, 1):
                        W[s, min(max(s + a, 0), T - 1)] += win_dense[w][a + 1]
                p = LD(1) / var[:, w * D].astype(LD)
                R += W.T @ (p[:, None] * W)
                rr += W.T @ (p * mean[:, w * D].astype(LD))
        return bool(np.all(np.abs(ref.band_to_dense(Rb[:, :, 0]) - R) <= g * Ra) and np.all(np.abs(r[:, 0].astype(LD) - rr) <= g * ra))

    assert r_fits(mean, win, win)
    assert not r_fits(mean, win, win, clamp=True)
    assert not r_fits(mean, (win[0], win[2], win[1]), win)
    asym3 = (win[0], (0.25, -1.0, 0.5), win[2])
    assert r_fits(mean, asym3, asym3)
    assert not r_fits(mean, (asym3[0], asym3[1][::-1], asym3[2]), asym3)
    # one subtraction of the factorisation out of order: the pivot's two products taken nearest first
    found = False
    for seed in range(5):
        _, _, m2, v2 = _inputs(65, 2, 20 + seed, False)
        a, pa = ref.mlpg(m2, v2, mc.WINDOWS[2][:3])
        b, pb = ref.mlpg(m2, v2, mc.WINDOWS[2][:3], order="near_first")
        found = found or not (mc.same_bits(a, b) and mc.same_bits(pa, pb))
    assert found
