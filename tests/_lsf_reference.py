"""The contract of wh_lpc_levinson / wh_lsf_from_lpc / wh_lsf_envelope (include/world_hip.h) in plain
NumPy: every operation in its order.  float64 element by element — NumPy's elementwise +, -, *, / are IEEE operations
without contraction — so the device can be held to it bit for bit; the frames are independent and are carried side by
side as NumPy rows, nothing is summed across them.  No transcendental is evaluated per frame: the only trigonometry is
the three host tables below (the device is handed the same arrays) and the acos / cos between the cosine domain
x = cos w of the kernels and the radians of the stored rows.

    tables       autocorr_table(K, p)[k][m] = w_k cos(2 pi k m / N) / N, N = 2 (K - 1), w = 1 at k = 0 and K - 1, else 2
                 grid_table()[g] = cos(pi g / 4096), g = 0 .. 4096: level G uses every (4096 / G)-th entry
                 bin_table(K)[k] = cos(pi k / (K - 1))
    levinson     E = r[0];  a[0] = 1
                 order n = 1 .. p:  acc = r[n];  for i = 1 .. n-1 ascending: acc = acc + a[i] * r[n-i]
                                    k = -(acc / E)                                       (the order's only division)
                                    for i = 1 .. n/2:  (a[i], a[n-i]) = (a[i] + k * a[n-i], a[n-i] + k * a[i])
                                    a[n] = k;  E = E * (1.0 - k * k)
                 r[0] == 0: a = e0, E = 0, k = 0, no flag.  r[0] < 0 or not finite, or an E that is not positive and
                 finite after any order: the frame's outputs are NaN and it is flagged.
    series       p = 2 m.  P_i = a[i] + a[p+1-i], Q_i = a[i] - a[p+1-i], i = 1 .. m;  g[0] = h[0] = a[0];
                 g[i] = P_i - g[i-1]  (P / (1 + 1/z));   h[i] = Q_i + h[i-1]  (Q / (1 - 1/z));
                 c[0] = g[m], c[k] = 2.0 * g[m-k]: the series sum c[k] T_k(x) whose roots are P's; the same with h for Q's.
    clenshaw     b1 = b2 = 0.0;  for k = m .. 1: (b1, b2) = ((2.0 * x) * b1 - b2) + c[k], b1;  f = (x * b1 - b2) + c[0]
    search       level G = 256, 512 .. 4096: points x_j = grid[j * 4096 / G], j = 0 .. G (x descending, w ascending);
                 n_j = (f(x_j) < 0.0);  a bracket is a j >= 1 with n_j != n_(j-1);  the first m of each series are taken,
                 and a level at which either series has fewer than m is replaced by the next; past 4096 the frame's row is
                 NaN and it is flagged.
    bisection    hi = x_(j-1), lo = x_j, n_hi = n_(j-1);  at most 60 times: mid = 0.5 * (lo + hi); stop if mid == lo or
                 mid == hi;  if (f(mid) < 0.0) == n_hi: hi = mid else lo = mid.   root = 0.5 * (lo + hi).
    interlace    x[2 i] = P's root i, x[2 i + 1] = Q's root i  (the lowest line spectral frequency is P's)
    envelope     per bin, c = bin_table[k]:  u = prod over P's roots in order of (2.0 * c - 2.0 * x_i), from 1.0; v the same
                 over Q's;  A2 = 0.25 * ((2.0 * (1.0 + c)) * (u * u) + (2.0 * (1.0 - c)) * (v * v));  S = E / A2
    repair       (radians, min_gap > 0 only)  w = min(max(w, gap), pi - gap);  forward i = 1 .. p-1: w[i] = max(w[i],
                 w[i-1] + gap);  w[p-1] = min(w[p-1], pi - gap);  backward i = p-2 .. 0: w[i] = min(w[i], w[i+1] - gap)

How far the reference's frequencies are from the exact roots (tests/test_lsf_reference_host.py compares with
mpmath.polyroots at 60 digits).  Let u = 2^-53, S = sum |c_k|, kappa = min(m + 1, 1 / sin w).  The recurrence's b_k are
sums of c_j U_(j-k)(x) with |U_n(x)| <= kappa, so |b_k| <= kappa S; a step rounds three times, an error of at most
3 u (3 kappa S) — and an error made at step k reaches f multiplied by U_k(x), again at most kappa.  m + 1 steps:
|fl(f) - f| <= 9 (m + 1) kappa^2 u S.  The series itself is not the exact one either: P_i and every step of the deflation
round once, g[i] carries at most (i + 1) of those, each at most u max|g| <= u S: in f a further 2 (m + 2) u S.  The sign
of fl(f) is right wherever |f| exceeds the sum of the two, so the bracket closes on a point within
dx = (9 (m + 1) kappa^2 + 2 (m + 2)) u S / |f'(x*)| of the root x*, plus the two neighbouring doubles the bisection ends
between and the rounding of the last midpoint, 2 u |x*|.  acos turns dx into dx / sin w and rounds once more (u pi):

    |w_ref - w*| <= ((9 (m + 1) kappa^2 + 2 (m + 2)) u S / |f'(x*)| + 2 u) / sin w* + 4 u

root_bound() evaluates it with f' taken at the exact root.  (First order in dx: it holds while dx is small against the
distance to the neighbouring root, which the division by f' looks after.)"""
import numpy as np

G_MIN, G_MAX = 256, 4096
MAX_BISECT = 60
MAX_ORDER = 64
U = 2.0 ** -53


# ---- tables ----------------------------------------------------------------------------------------------------------
def autocorr_table(k_bins, p):
    n = 2 * (k_bins - 1)
    k = np.arange(k_bins, dtype=np.int64)[:, None]
    m = np.arange(p + 1, dtype=np.int64)[None, :]
    w = np.full((k_bins, 1), 2.0)
    w[0] = w[-1] = 1.0
    return np.ascontiguousarray(w * np.cos(2 * np.pi * ((k * m) % n) / n) / n)


def grid_table():
    g = np.cos(np.pi * np.arange(G_MAX + 1) / G_MAX)
    g[0], g[-1] = 1.0, -1.0
    return g


def bin_table(k_bins):
    c = np.cos(np.pi * np.arange(k_bins) / (k_bins - 1))
    c[0], c[-1] = 1.0, -1.0
    return c


def autocorr(spec, p):
    """Lags 0 .. p of power-spectrum rows [F][K] as the table product (summation order: NumPy's)."""
    spec = np.asarray(spec, dtype=np.float64)
    return spec @ autocorr_table(spec.shape[1], p)


def autocorr_ld(spec, p):
    """The same in long double, with its own cosines."""
    spec = np.asarray(spec, dtype=np.longdouble)
    k_bins = spec.shape[1]
    n = 2 * (k_bins - 1)
    k = np.arange(k_bins, dtype=np.int64)[:, None]
    m = np.arange(p + 1, dtype=np.int64)[None, :]
    w = np.full((k_bins, 1), 2.0, dtype=np.longdouble)
    w[0] = w[-1] = 1.0
    ang = (2 * np.arccos(np.longdouble(-1))) * ((k * m) % n).astype(np.longdouble) / n
    return spec @ (w * np.cos(ang) / n)


# ---- b. Levinson-Durbin ----------------------------------------------------------------------------------------------
def levinson(r, p):
    """r [F][>= p + 1] -> (a [F][p + 1], E [F], refl [F][p], flagged [F] bool)."""
    r = np.asarray(r, dtype=np.float64)
    nf = r.shape[0]
    a = np.zeros((nf, p + 1))
    a[:, 0] = 1.0
    refl = np.zeros((nf, p))
    with np.errstate(all="ignore"):
        e = np.array(r[:, 0])
        zero = e == 0.0
        bad = ~zero & ~((e > 0.0) & (e < np.inf))
        for n in range(1, p + 1):
            acc = np.array(r[:, n])
            for i in range(1, n):
                acc = acc + a[:, i] * r[:, n - i]
            k = -(acc / e)
            for i in range(1, n // 2 + 1):
                ai, aj = np.array(a[:, i]), np.array(a[:, n - i])
                a[:, i] = ai + k * aj
                a[:, n - i] = aj + k * ai
            a[:, n] = k
            refl[:, n - 1] = k
            e = e * (1.0 - k * k)
            bad |= ~zero & ~((e > 0.0) & (e < np.inf))
    a[zero, 1:] = 0.0
    a[zero, 0] = 1.0
    refl[zero] = 0.0
    e[zero] = 0.0
    a[bad] = np.nan
    refl[bad] = np.nan
    e[bad] = np.nan
    return a, e, refl, bad


# ---- c. line spectral frequencies ------------------------------------------------------------------------------------
def chebyshev_series(a, mutant=None):
    """a [F][p + 1] -> (cP, cQ) [F][m + 1]."""
    a = np.asarray(a, dtype=np.float64)
    p = a.shape[1] - 1
    m = p // 2
    g = np.empty((a.shape[0], m + 1))
    h = np.empty((a.shape[0], m + 1))
    g[:, 0] = h[:, 0] = a[:, 0]
    for i in range(1, m + 1):
        if mutant == "deflation_sign":
            g[:, i] = (a[:, i] + a[:, p + 1 - i]) + g[:, i - 1]
        else:
            g[:, i] = (a[:, i] + a[:, p + 1 - i]) - g[:, i - 1]
        h[:, i] = (a[:, i] - a[:, p + 1 - i]) + h[:, i - 1]
    cp, cq = np.empty_like(g), np.empty_like(h)
    cp[:, 0], cq[:, 0] = g[:, m], h[:, m]
    for k in range(1, m + 1):
        cp[:, k] = 2.0 * g[:, m - k]
        cq[:, k] = 2.0 * h[:, m - k]
    return cp, cq


def clenshaw(c, x):
    """c [F][m + 1], x [F][n] -> f [F][n]."""
    m = c.shape[1] - 1
    tx = 2.0 * x
    b1 = np.zeros_like(x)
    b2 = np.zeros_like(x)
    for k in range(m, 0, -1):
        b1, b2 = (tx * b1 - b2) + c[:, k:k + 1], b1
    return (x * b1 - b2) + c[:, 0:1]


def _brackets(c, xs, m):
    """First m brackets of every row at the points xs: (found [F] bool, j [F][m], n_hi [F][m] bool)."""
    f = clenshaw(c, np.broadcast_to(xs, (c.shape[0], len(xs))))
    neg = f < 0.0
    change = neg[:, 1:] != neg[:, :-1]
    found = change.sum(axis=1) >= m
    j = np.ones((c.shape[0], m), dtype=np.int64)
    for row in np.nonzero(found)[0]:
        j[row] = np.nonzero(change[row])[0][:m] + 1
    return found, j, np.take_along_axis(neg, j - 1, axis=1)


def _bisect(c, lo, hi, n_hi, mutant=None):
    lo, hi = np.array(lo), np.array(hi)
    for _ in range(MAX_BISECT):
        mid = 0.5 * (lo + hi)
        live = (mid != lo) & (mid != hi)
        if not live.any():
            break
        same = (clenshaw(c, mid) < 0.0) == n_hi
        if mutant == "wrong_half":
            same = ~same
        hi = np.where(live & same, mid, hi)
        lo = np.where(live & ~same, mid, lo)
    return 0.5 * (lo + hi)


def lsf_from_lpc(a, grid=None, mutant=None):
    """a [F][p + 1] -> (x [F][p] = cos of the line spectral frequencies, x descending; level [F]: the grid level that
    found every root, 0 for a flagged frame whose row is NaN)."""
    a = np.asarray(a, dtype=np.float64)
    p = a.shape[1] - 1
    if p % 2 or not 2 <= p <= MAX_ORDER:
        raise ValueError("the order must be even and in [2, %d], got %d" % (MAX_ORDER, p))
    grid = grid_table() if grid is None else grid
    m = p // 2
    nf = a.shape[0]
    x = np.full((nf, p), np.nan)
    level = np.zeros(nf, dtype=np.int32)
    with np.errstate(all="ignore"):
        cp, cq = chebyshev_series(a, mutant)
        todo = np.arange(nf)
        g = G_MIN
        while g <= G_MAX and len(todo):
            xs = grid[::G_MAX // g]
            okp, jp, np_hi = _brackets(cp[todo], xs, m)
            okq, jq, nq_hi = _brackets(cq[todo], xs, m)
            ok = okp & okq
            rows = todo[ok]
            if len(rows):
                rp = _bisect(cp[rows], xs[jp[ok]], xs[jp[ok] - 1], np_hi[ok], mutant)
                rq = _bisect(cq[rows], xs[jq[ok]], xs[jq[ok] - 1], nq_hi[ok], mutant)
                if mutant == "swapped_interlace":
                    rp, rq = rq, rp
                x[rows, 0::2] = rp
                x[rows, 1::2] = rq
                level[rows] = g
            todo = todo[~ok]
            g *= 2
    return x, level


# ---- d. envelope -----------------------------------------------------------------------------------------------------
def repair(w, min_gap):
    """Rows of radians made decodable: inside [gap, pi - gap] and at least gap apart."""
    w = np.array(w, dtype=np.float64)
    if not min_gap > 0:
        return w
    p = w.shape[1]
    with np.errstate(all="ignore"):
        w = np.minimum(np.maximum(w, min_gap), np.pi - min_gap)
        for i in range(1, p):
            w[:, i] = np.maximum(w[:, i], w[:, i - 1] + min_gap)
        w[:, p - 1] = np.minimum(w[:, p - 1], np.pi - min_gap)
        for i in range(p - 2, -1, -1):
            w[:, i] = np.minimum(w[:, i], w[:, i + 1] - min_gap)
    return w


def envelope(e, x, k_bins, ctab=None):
    """e [F], x [F][p] (cosines, as lsf_from_lpc returns them) -> power spectrum [F][K]."""
    e = np.asarray(e, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    c = (bin_table(k_bins) if ctab is None else ctab)[None, :]
    tc = 2.0 * c
    with np.errstate(all="ignore"):
        u = np.ones((x.shape[0], k_bins))
        v = np.ones((x.shape[0], k_bins))
        for i in range(0, x.shape[1], 2):
            u = u * (tc - (2.0 * x[:, i])[:, None])
            v = v * (tc - (2.0 * x[:, i + 1])[:, None])
        a2 = 0.25 * ((2.0 * (1.0 + c)) * (u * u) + (2.0 * (1.0 - c)) * (v * v))
        return e[:, None] / a2


# ---- the chain: what world.lsf computes ------------------------------------------------------------------------------
def lsf_rows(r, p):
    """Autocorrelations [F][p + 1] -> (rows [F][p + 1] = [log E, w_1 .. w_p], level, flagged)."""
    a, e, _, bad = levinson(r, p)
    x, level = lsf_from_lpc(a)
    with np.errstate(all="ignore"):
        rows = np.concatenate([np.log(e)[:, None], np.arccos(x)], axis=1)
    return rows, level, bad | (level == 0)


def ilsf_rows(rows, k_bins, min_gap=0.0):
    rows = np.asarray(rows, dtype=np.float64)
    with np.errstate(all="ignore"):
        return envelope(np.exp(rows[:, 0]), np.cos(repair(rows[:, 1:], min_gap)), k_bins)


def lsd_db(s_a, s_b):
    """Log-spectral distortion: the mean over frames of the RMS over bins of the dB difference of two power spectra."""
    d = 10.0 * np.log10(np.asarray(s_a, dtype=np.float64) / np.asarray(s_b, dtype=np.float64))
    return float(np.mean(np.sqrt(np.mean(d * d, axis=1))))


# ---- what the host tests measure the reference with ------------------------------------------------------------------
def root_bound(c, w_exact, dfdx):
    """The docstring's bound on |w_ref - w*| for roots w_exact [n] of the series c [m + 1] with |f'(x*)| = dfdx [n]."""
    m = len(c) - 1
    s = float(np.sum(np.abs(c)))
    sin_w = np.sin(w_exact)
    kappa = np.minimum(m + 1.0, 1.0 / sin_w)
    dx = (9.0 * (m + 1) * kappa ** 2 + 2.0 * (m + 2)) * U * s / dfdx + 2.0 * U
    return dx / sin_w + 4.0 * U
