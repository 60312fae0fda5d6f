"""The contract of wh_delta_features / wh_mlpg (include/world_hip.h) in plain NumPy and Python: the
windows, the edge rule, the order of every sum and of every subtraction.  float64 element by element — NumPy's scalar
and elementwise +, -, *, / are IEEE operations without contraction — so the device can be held to it bit for bit.  The
columns of one utterance are independent systems and are carried side by side as NumPy rows; nothing is summed across
them.

    windows      win[n_win][2L + 1], window 0 the static one (centre tap 1.0, all others 0.0), L in {0, 1, 2}
    edges        a tap that reaches outside the utterance is dropped (np.correlate(x, win[::-1], 'same'))
    features     y[s][w D + d] = sum over a = -L .. L ascending, 0 <= s + a < T, of win[w][a + L] * x[s + a][d], from 0.0
    generation   p_w[s] = 1.0 / var[s][w D + d]
                 R[t][t+k] = sum over w ascending, s ascending in max(0, t+k-L) .. min(T-1, t+L), of
                             (win[w][t-s+L] * p_w[s]) * win[w][t+k-s+L], from 0.0           k = 0 .. B = 2L, t + k < T
                 r[t]      = the same sum of (win[w][t-s+L] * p_w[s]) * mean[s][w D + d], s in max(0, t-L) .. min(T-1, t+L)
                 LDL', row t with m = min(B, t):  for k = m .. 1:  v_k = R[t-k][t];  for n = m .. k+1: v_k -= v_n * l[t-k][n-k];
                                                                    l[t][k] = v_k * q[t-k]
                       d[t] = R[t][t];  for k = m .. 1: d[t] -= v_k * l[t][k];     q[t] = 1.0 / d[t]
                       z[t] = r[t];     for k = m .. 1: z[t] -= l[t][k] * z[t-k];  y[t] = z[t] * q[t]
                 back, t = T-1 .. 0:  c[t] = y[t];  for k = min(B, T-1-t) .. 1: c[t] -= l[t+k][k] * c[t+k]
"""
import numpy as np

HTS_WINDOWS = ((0.0, 1.0, 0.0), (-0.5, 0.0, 0.5), (1.0, -2.0, 1.0))


def check_windows(windows):
    """(win [n_win][2L + 1] float64, L) or ValueError."""
    rows = [np.asarray(w, dtype=np.float64) for w in windows]
    if not 1 <= len(rows) <= 4:
        raise ValueError("1 .. 4 windows, got %d" % len(rows))
    if any(r.ndim != 1 for r in rows) or len({len(r) for r in rows}) != 1:
        raise ValueError("the windows must all have the same number of taps")
    n = len(rows[0])
    if n not in (1, 3, 5):
        raise ValueError("windows of 1, 3 or 5 taps (half-width 0, 1 or 2), got %d" % n)
    win = np.stack(rows)
    half = n // 2
    static = np.zeros(n)
    static[half] = 1.0
    if not np.array_equal(win[0], static):
        raise ValueError("window 0 must be the static window: centre tap 1.0, every other tap 0.0")
    return win, half


def delta_features(x, windows):
    """x [T][D] -> y [T][n_win D]."""
    win, L = check_windows(windows)
    x = np.asarray(x, dtype=np.float64)
    T, D = x.shape
    y = np.zeros((T, len(win) * D))
    for w in range(len(win)):
        for s in range(T):
            acc = np.zeros(D)
            for a in range(-L, L + 1):
                if 0 <= s + a < T:
                    acc = acc + win[w][a + L] * x[s + a]
            y[s, w * D:(w + 1) * D] = acc
    return y


def normal_equations(mean, var, windows):
    """Rb [T][B + 1][D] with Rb[t][k] = R[t][t+k] (0.0 where t + k >= T), r [T][D], for mean [T][n_win D] and var
    [T][n_win D] or [n_win D]."""
    win, L = check_windows(windows)
    mean = np.asarray(mean, dtype=np.float64)
    T, width = mean.shape
    nw, B = len(win), 2 * L
    D = width // nw
    var = np.broadcast_to(np.asarray(var, dtype=np.float64), (T, width))
    with np.errstate(all="ignore"):
        p = 1.0 / var
        Rb, r = np.zeros((T, B + 1, D)), np.zeros((T, D))
        for t in range(T):
            for k in range(B + 1):
                if t + k >= T:
                    break
                acc = np.zeros(D)
                for w in range(nw):
                    for s in range(max(0, t + k - L), min(T - 1, t + L) + 1):
                        acc = acc + (win[w][t - s + L] * p[s, w * D:(w + 1) * D]) * win[w][t + k - s + L]
                Rb[t, k] = acc
            acc = np.zeros(D)
            for w in range(nw):
                for s in range(max(0, t - L), min(T - 1, t + L) + 1):
                    acc = acc + (win[w][t - s + L] * p[s, w * D:(w + 1) * D]) * mean[s, w * D:(w + 1) * D]
            r[t] = acc
    return Rb, r


def ldl_solve(Rb, r, order="far_first"):
    """The sequential banded LDL' of the contract.  Returns c [T][D], the pivots d [T][D] and the multipliers l [T][B + 1][D]
    (l[t][k] = L[t][t-k]; l[t][0] = 1).  ``order`` = 'near_first' runs the pivot's subtractions the other way round: a
    mutant for the tests of the comparators, not part of the contract."""
    T, B1, D = Rb.shape
    B = B1 - 1
    lm, dv, q, z = np.zeros((T, B1, D)), np.zeros((T, D)), np.zeros((T, D)), np.zeros((T, D))
    lm[:, 0] = 1.0
    y, c = np.zeros((T, D)), np.zeros((T, D))
    with np.errstate(all="ignore"):
        for t in range(T):
            m = min(B, t)
            v = [None] * (B + 1)
            for k in range(m, 0, -1):
                a = Rb[t - k, k]
                for n in range(m, k, -1):
                    a = a - v[n] * lm[t - k, n - k]
                v[k] = a
                lm[t, k] = a * q[t - k]
            dd, zz = Rb[t, 0], r[t]
            for k in (range(m, 0, -1) if order == "far_first" else range(1, m + 1)):
                dd = dd - v[k] * lm[t, k]
            for k in range(m, 0, -1):
                zz = zz - lm[t, k] * z[t - k]
            dv[t], z[t] = dd, zz
            q[t] = 1.0 / dd
            y[t] = zz * q[t]
        for t in range(T - 1, -1, -1):
            cc = y[t]
            for k in range(min(B, T - 1 - t), 0, -1):
                cc = cc - lm[t + k, k] * c[t + k]
            c[t] = cc
    return c, dv, lm


def mlpg(mean, var, windows, order="far_first"):
    """(track [T][D], pivots [T][D])."""
    Rb, r = normal_equations(mean, var, windows)
    c, dv, _ = ldl_solve(Rb, r, order)
    return c, dv


# ---- what the host tests measure the reference with -------------------------------------------------------------------
def gamma(k):
    """Higham's gamma_k = k u / (1 - k u), u = 2^-53, in long double."""
    u = np.longdouble(2.0) ** -53
    return k * u / (1 - k * u)


def dense_w(win, T, w):
    """W_w [T][T] in long double: row s holds win[w][a + L] at column s + a, taps outside dropped."""
    L = win.shape[1] // 2
    W = np.zeros((T, T), dtype=np.longdouble)
    for s in range(T):
        for a in range(-L, L + 1):
            if 0 <= s + a < T:
                W[s, s + a] = win[w][a + L]
    return W


def band_to_dense(Rb):
    """Rb [T][B + 1] of ONE column -> the symmetric [T][T] in long double."""
    T, B1 = Rb.shape
    R = np.zeros((T, T), dtype=np.longdouble)
    for t in range(T):
        for k in range(B1):
            if t + k < T:
                R[t, t + k] = R[t + k, t] = Rb[t, k]
    return R


def residual_and_bound(Rb, r, c, dv, lm, k_ops):
    """For ONE column: |R c - r| and gamma_k (|L||D||L'||c| + |r|), both [T] in long double (R the banded matrix as
    given)."""
    T = len(r)
    R = band_to_dense(Rb)
    Lm = np.zeros((T, T), dtype=np.longdouble)
    for t in range(T):
        for k in range(lm.shape[1]):
            if t - k >= 0:
                Lm[t, t - k] = lm[t, k]
    cl, rl = c.astype(np.longdouble), r.astype(np.longdouble)
    res = np.abs(R @ cl - rl)
    ldl = np.abs(Lm) @ (np.abs(dv.astype(np.longdouble)) * (np.abs(Lm).T @ np.abs(cl)))
    return res, gamma(k_ops) * (ldl + np.abs(rl))


def residual_ops(B):
    """k of the residual bound, counted per entry: 3 B + 7."""
    return 3 * B + 7
