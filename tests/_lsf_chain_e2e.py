"""The conversion chain over line spectral frequencies on the CPU, from the references alone — the record the device's
end-to-end figures are held to (tests/test_lsf_chain_host.py checks it, tests/test_hip_lsf_conversion.py compares).

Input: the committed 48 kHz spectrogram fixture (tests/golden/golden_syn48k.npz, 101 frames of 1025 bins).  Speaker a is
its LSF rows (tests/_lsf_reference.py, order 8).  Speaker b is made the way tests/test_hip_gmm_fit.py makes its pair — a
map per regime and a little noise — on the angles: w' = w + a_c sin w + b_c sin 2 w with |a_c| + 2 |b_c| < 1 (monotone, 0
and pi fixed, so ascending angles stay ascending inside (0, pi)), the regime c changing every 20 frames, on another
timing (90 frames, a power-law warp), the gain 0.3 up.

    align      tests/_dtw_reference.py over the angles
    features   tests/_mlpg_reference.py: static + delta of the angles, joined along the path
    fit        world.gmm.fit_device's default start (rows picked by default_rng(0), the global covariance) and 3 EM steps
               of tests/_gmm_reference.py, 2 components, reg_covar 1e-4; covariances symmetrised
    convert    the tables of JointGMM.host_tables (NumPy on the host), the best component under the marginal of x and its
               conditional mean rows by tests/_gmm_reference.py, MLPG by tests/_mlpg_reference.py, the repair by
               tests/_lsf_chain_reference.py with the target's smallest gap
    score      the aligned gain-free log-spectral distortion to the target: tests/_lsf_chain_reference.py on np.cos of the
               rows, the mean over the path

How far a device run of the same chain (the same model handed over) may be from this record — record()'s dw, tol_before and tol_after.  The path
is the reference's bit for bit (wh_dtw's contract), and so are the delta rows, the variances, the MLPG factorisation
(it depends on the variances alone) and the repair.  What differs:
  * the conditional mean rows: each side is within B of the exact ones (convert_best's bound, evaluated in long double),
    so 2 B apart, provided the best component is the same — record() asserts that every frame's margin between its two
    best log-likelihoods is more than the two evaluations' bounds, and the GPU test compares the indices;
  * MLPG is linear in the means: c = G mu, G = R^-1 [W_0' P_0 | W_1' P_1] per column, so the tracks are |G| (2 B) apart,
    plus each solve's own rounding: at most |R^-1| (the residual bound of the banded solve, _mlpg_reference, + gamma_8 of
    the right-hand side's terms) on either side (G and R^-1 by numpy.linalg.inv of the small dense matrices);
  * the repair is max / min against constants and neighbours +- gap: it moves no angle further than its inputs moved
    (sup norm), and rounds p times (2 p u0 pi);   together: dw, the bound on every converted angle;
  * the cosines: the device library's is documented to 2 ulp, NumPy's is within one: 3 ulp = 6 u0 |x| apart.
An angle moved by dw moves its cosine by at most dw, the factor 2 c - 2 x_i by the fraction r_i = dx_i / |c - x_i| of
itself, and t = log(A2_a / A2_b) — A2 a non-negative combination of u^2 and v^2 — by at most 2 sum_i r_i / (1 - r_i) over
the roots of both sides.  The gain-free cell value c sqrt(var_k t) moves by at most c sqrt(mean_k dt^2) (a standard
deviation is 1-Lipschitz in the RMS norm); db_bound(order_bounds) covers the two evaluations of the same rows, and the
mean over n cells rounds n times."""
import functools
import os

import numpy as np

import _dtw_reference as dref
import _gmm_reference as gref
import _lsf_chain_reference as cref
import _lsf_reference as ref
import _mlpg_reference as mref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FS, FFT_SIZE, K_BINS = 48000, 2048, 1025
P, M, N_ITER, REG, SEED = 8, 2, 3, 1e-4, 0
WIN = mref.HTS_WINDOWS[:2]
U = 2.0 ** -53


def _speakers():
    spec = np.ascontiguousarray(np.load(os.path.join(GOLDEN, "golden_syn48k.npz"))["ct_spectrogram"].T)
    rows_a, _, bad = ref.lsf_rows(ref.autocorr(spec, P), P)
    assert not bad.any() and spec.shape[1] == K_BINS
    rng = np.random.RandomState(7)
    fa = len(rows_a)
    fb = int(0.9 * fa)
    src = np.round((fa - 1) * (np.arange(fb) / (fb - 1.0)) ** 1.15).astype(np.int64)
    regime = np.repeat(rng.randint(0, 2, size=fb // 20 + 1), 20)[:fb]
    a_c, b_c = np.array([0.15, -0.12]), np.array([-0.06, 0.08])
    w = rows_a[src, 1:]
    w = w + a_c[regime][:, None] * np.sin(w) + b_c[regime][:, None] * np.sin(2.0 * w) + 0.002 * rng.standard_normal(w.shape)
    w, _ = cref.repair(w, *cref.gap_hi(1e-3))
    rows_b = np.concatenate([rows_a[src, :1] + 0.3, w], axis=1)
    return rows_a, rows_b


def _fit(z, dx):
    n, d = z.shape
    pick = np.sort(np.random.default_rng(SEED).choice(n, size=M, replace=False))
    mu = z[pick]
    s0, s1, s2 = gref.stats(z, np.ones((n, 1)), mu[:1])[:3]
    delta = s1[0] / s0[0]
    glob = s2[0] / s0[0] - np.outer(delta, delta) + REG * np.eye(d)
    w, cov = np.full(M, 1.0 / M), np.repeat(glob[None], M, axis=0)
    for _ in range(N_ITER):
        cov = 0.5 * (cov + cov.transpose(0, 2, 1))
        whiten, logc = gref.prepare(w, mu, cov)
        gamma = gref.reduce(gref.loglik(z, mu, whiten, logc)[0])[0]
        w, mu, cov = gref.m_step(mu, *gref.stats(z, gamma, mu)[:3], REG)[:3]
    return w, mu, 0.5 * (cov + cov.transpose(0, 2, 1))


def _aligned_lsd(rows_a, rows_b, pa, pb):
    """(the mean over the path of the gain-free cell distortion, the cells, their s1, s2)."""
    ex_a = np.concatenate([rows_a[:, :1], np.cos(rows_a[:, 1:])], axis=1)
    ex_b = np.concatenate([rows_b[:, :1], np.cos(rows_b[:, 1:])], axis=1)
    s = cref.distortion(ex_a, ex_b, K_BINS, pa, pb)
    cells = cref.distortion_db(np.zeros(len(pa)), s[:, 0], s[:, 1], K_BINS, gain=False)
    return float(np.mean(cells)), cells, s


def _cell_tolerance(rows_a, rows_b, pa, pb, dw_a):
    """The docstring's bound on the mean over the path, side a's angles within dw_a of the record's."""
    xa, xb = np.cos(rows_a[pa, 1:]), np.cos(rows_b[pb, 1:])
    c = ref.bin_table(K_BINS)
    dt = np.zeros((len(pa), K_BINS))
    for x, dx in ((xa, dw_a + 6.0 * U * np.abs(xa)), (xb, 6.0 * U * np.abs(xb))):
        with np.errstate(all="ignore"):
            r = dx[:, None, :] / np.abs(c[None, :, None] - x[:, None, :])
        assert np.all(r < 0.5), "a root within the tolerance of a bin: the first-order bound does not hold"
        dt += 2.0 * np.sum(r / (1.0 - r), axis=2)
    t = cref.log_ratio(xa, xb, K_BINS)
    s1, s2 = np.sum(t, axis=1), np.sum(t * t, axis=1)
    b1, b2 = cref.order_bounds(t)
    cells = cref.LSD_SCALE * np.sqrt(np.mean(dt * dt, axis=1)) + cref.db_bound(0.0 * s1, s1, s2, b1, b2, K_BINS, gain=False)
    n = len(pa)
    return float(np.mean(cells)) * (1.0 + n * U) + n * U * float(np.mean(np.abs(cref.distortion_db(0.0 * s1, s1, s2, K_BINS, False))))


def _track_tolerance(mean, b_mean, var):
    """dw of the docstring: the bound on every angle of the converted track."""
    win, _ = mref.check_windows(WIN)
    T, d = mean.shape[0], mean.shape[1] // len(win)
    Rb, r = mref.normal_equations(mean, var, WIN)
    c, dv, lm = mref.ldl_solve(Rb, r)
    worst = 0.0
    for col in range(d):
        R = mref.band_to_dense(Rb[:, :, col]).astype(np.float64)
        Rinv = np.abs(np.linalg.inv(R))
        wp = [mref.dense_w(win, T, w).astype(np.float64).T / var[None, :, w * d + col] for w in range(len(win))]
        G = np.abs(np.linalg.inv(R) @ np.concatenate(wp, axis=1))
        moved = G @ np.concatenate([2.0 * b_mean[:, w * d + col] for w in range(len(win))])
        _, res = mref.residual_and_bound(Rb[:, :, col], r[:, col], c[:, col], dv[:, col], lm[:, :, col],
                                         mref.residual_ops(Rb.shape[1] - 1))
        rhs = sum(np.abs(wp[w]) @ np.abs(mean[:, w * d + col]) for w in range(len(win)))
        solve = 2.0 * (Rinv @ (res.astype(np.float64) + 8.0 * U * rhs))
        worst = max(worst, float(np.max(moved + solve)))
    return worst + 2.0 * d * U * np.pi


@functools.lru_cache(maxsize=None)
def record():
    """Everything of the chain, computed once: rows, path, model, converted rows, the two scores and their tolerances."""
    from world import gmm

    rows_a, rows_b = _speakers()
    al = dref.dtw(rows_a[:, 1:], rows_b[:, 1:])
    pa, pb = al["path_a"], al["path_b"]
    assert dref.well_formed(pa, pb, len(rows_a), len(rows_b))
    fa, fb = mref.delta_features(rows_a[:, 1:], WIN), mref.delta_features(rows_b[:, 1:], WIN)
    z = np.concatenate([fa[pa], fb[pb]], axis=1)
    dx = len(WIN) * P
    w, mu, cov = _fit(z, dx)
    gap = gmm.lsf_min_gap(rows_b)
    model = gmm.JointGMM(w, mu, cov, dx, "lsf", P, gap)
    t = model.host_tables()
    ll, b_ll = gref.loglik(fa, t["mu_x"], t["whiten_x"], t["logc_x"], gref.LD)
    best = gref.reduce(ll)[2]
    order = np.sort(ll.astype(np.float64), axis=1)
    margin = order[:, -1] - order[:, -2]
    assert np.all(margin > 2.0 * np.sum(b_ll.astype(np.float64), axis=1)), "a frame whose best component is a toss-up"
    _, b_mean = gref.convert_best(fa, t["mu_x"], t["a"], t["mu_y"], best, gref.LD)
    mean = gref.convert_best(fa, t["mu_x"], t["a"], t["mu_y"], best)[0]
    var = t["cvar"][best]
    track = mref.mlpg(mean, var, WIN)[0]
    conv = np.concatenate([rows_a[:, :1], cref.repair(track, *cref.gap_hi(gap))[0]], axis=1)
    dw = _track_tolerance(mean, b_mean.astype(np.float64), var)
    before, _, _ = _aligned_lsd(rows_a, rows_b, pa, pb)
    after, _, _ = _aligned_lsd(conv, rows_b, pa, pb)
    out = {"rows_a": rows_a, "rows_b": rows_b, "path_a": pa, "path_b": pb, "model": model, "best": best, "conv": conv,
           "dw": dw, "before": before, "after": after,
           "tol_before": _cell_tolerance(rows_a, rows_b, pa, pb, 0.0),
           "tol_after": _cell_tolerance(conv, rows_b, pa, pb, dw)}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
