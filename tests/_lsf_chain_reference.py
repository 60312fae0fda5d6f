"""The contract of wh_lsf_repair / wh_lsf_distortion (include/world_hip.h) in plain NumPy, and what
world.lsf makes of the distortion kernel's two sums.

    repair       (radians; gap > 0 and hi from the caller — world.lsf passes min_gap and the double pi - min_gap)
                 1. w[i] = min(max(w[i], gap), hi) for every i     2. w[i] = max(w[i], w[i-1] + gap), i = 1 .. p-1 ascending
                 3. w[p-1] = min(w[p-1], hi)                        4. w[i] = min(w[i], w[i+1] - gap), i = p-2 .. 0 descending
                 max / min are np.maximum / np.minimum (a NaN operand gives NaN, as torch.maximum / minimum / clamp do);
                 every + and - is one IEEE operation: the device is held to it bit for bit.
                 changed[f] = the number of angles of frame f whose output bits differ from the input bits.
    distortion   rows [., x_1 .. x_p] (cosines, descending), per bin c = bin_table(K)[k] and per side, exactly as
                 _lsf_reference.envelope forms them:  u = prod over i = 0, 2, .. of (2.0 * c - 2.0 * x[i]) from 1.0, v the
                 same over i = 1, 3, ..;  A2 = 0.25 * ((2.0 * (1.0 + c)) * (u * u) + (2.0 * (1.0 - c)) * (v * v));
                 q = A2_a / A2_b;  t = log q;   out = (sum_k t, sum_k t * t).
                 The order of the two sums is not part of the contract (np.sum here).  An index outside [0, n_rows)
                 gives (NaN, NaN).
    dB           S = E / A2, so ln S_a - ln S_b = g - t with g = log E_a - log E_b: the gain enters with the sign
                 OPPOSITE to t.  c = 10 / ln 10, K bins:
                 gain=True   c sqrt(max(0, g^2 - 2 g s1 / K + s2 / K))   (the RMS over the bins of the dB difference)
                 gain=False  c sqrt(max(0, s2 / K - (s1 / K)^2))         (the same, the best constant gain taken out)

How far the sums are from the exact ones of the same double rows (tests/test_lsf_chain_reference_host.py compares with
a long-double evaluation).  u0 = 2^-53, gamma(n) = n u0 / (1 - n u0).  Doubling is exact, so a factor 2 c - 2 x_i is ONE
rounded subtraction; a product of m = p / 2 factors takes m rounded multiplies: u and v carry (1 + d)^(2 m), a relative
error of at most gamma(2 m).  u * u: gamma(4 m + 1).  2 (1 + c) is one rounded addition (the doubling exact) and its product
with u * u one more multiply: gamma(4 m + 3) = gamma(2 p + 3) on each of the two terms.  Both terms are non-negative, so
their sum has the relative error of the worse one plus one rounding — no cancellation —: gamma(2 p + 4); the factor 0.25
is exact.  The quotient of two such values, one division: gamma(2 (2 p + 4) + 1) = gamma(4 p + 9) on q.  The logarithm
turns a relative error e of its argument into an absolute one of at most e / (1 - e), and its own evaluation is within
1 ulp <= 2 u0 |t| of the logarithm of what it was given:

    |fl(t) - t| <= e_t = gamma(4 p + 9) / (1 - gamma(4 p + 9)) + 2 u0 (|t| + gamma(4 p + 9) / (1 - gamma(4 p + 9)))

A sum of K terms in any order is within gamma(K - 1) sum |terms| of the exact sum of the same terms, t * t is one rounded
multiply, and |fl(t)^2 - t^2| <= e_t (2 |t| + e_t):

    |fl(s1) - s1| <= b1 = sum e_t + gamma(K - 1) sum (|t| + e_t)
    |fl(s2) - s2| <= b2 = sum e_t (2 |t| + e_t) + (u0 + gamma(K - 1) (1 + u0)) sum (|t| + e_t)^2

(no underflow or overflow on the way, which holds for rows inside [-1, 1]: a factor is at most 4 in magnitude, 4^32 = 2^64,
and a factor below 2^-52 needs a root on a bin).  sum_bounds() evaluates b1 and b2 from the exact t.

The device forms q with the same operations in the same order as this file — the same bits — and differs in the
logarithm (each side within 1 ulp of the logarithm of the same q) and in the order of the two sums.  order_bounds() is
the bound between two such evaluations: per term 2 ulp = 4 u0 |t|, per sum gamma(K - 1) on each side."""
import numpy as np

import _lsf_reference as ref

U = 2.0 ** -53
LD = np.longdouble
LSD_SCALE = 10.0 / np.log(10.0)


# ---- repair ------------------------------------------------------------------------------------------------------------
def repair(w, gap, hi):
    """w [F][p] radians -> (repaired [F][p], changed int32 [F])."""
    w0 = np.array(w, dtype=np.float64)
    w = np.array(w0)
    p = w.shape[1]
    with np.errstate(all="ignore"):
        w = np.minimum(np.maximum(w, gap), hi)
        for i in range(1, p):
            w[:, i] = np.maximum(w[:, i], w[:, i - 1] + gap)
        w[:, p - 1] = np.minimum(w[:, p - 1], hi)
        for i in range(p - 2, -1, -1):
            w[:, i] = np.minimum(w[:, i], w[:, i + 1] - gap)
    changed = np.sum(w.view(np.int64) != w0.view(np.int64), axis=1).astype(np.int32)
    return w, changed


def gap_hi(min_gap):
    """What world.lsf hands the kernel for ``min_gap``: (float(min_gap), float(np.pi - min_gap))."""
    return float(min_gap), float(np.pi - min_gap)


# ---- distortion --------------------------------------------------------------------------------------------------------
def a2(x, k_bins, dtype=np.float64, mutant=None):
    """|A|^2 [F][K] of rows of cosines x [F][p] in product form, in ``dtype``; the bins' cosines are the double table."""
    x = np.asarray(x, dtype=np.float64).astype(dtype)
    c = ref.bin_table(k_bins).astype(dtype)[None, :]
    two, one, quarter = dtype(2.0), dtype(1.0), dtype(0.25)
    tc = two * c
    with np.errstate(all="ignore"):
        u = np.ones((x.shape[0], k_bins), dtype=dtype)
        v = np.ones((x.shape[0], k_bins), dtype=dtype)
        for i in range(0, x.shape[1], 2):
            u = u * (tc - (two * x[:, i])[:, None])
            v = v * (tc - (two * x[:, i + 1])[:, None])
        if mutant == "swapped":
            u, v = v, u
        out = (two * (one + c)) * (u * u) + (two * (one - c)) * (v * v)
        return out if mutant == "no_quarter" else quarter * out


def log_ratio(x_a, x_b, k_bins, dtype=np.float64, mutant=None):
    """t [F][K] = log(A2_a / A2_b) row by row; a mutant changes side a only."""
    with np.errstate(all="ignore"):
        return np.log(a2(x_a, k_bins, dtype, mutant) / a2(x_b, k_bins, dtype))


def distortion(rows_a, rows_b, k_bins, idx_a=None, idx_b=None, mutant=None):
    """rows [n_rows][p + 1] = [., x_1 .. x_p] -> out [n_pairs][2] = (sum t, sum t * t); column 0 is not read."""
    rows_a, rows_b = np.asarray(rows_a, dtype=np.float64), np.asarray(rows_b, dtype=np.float64)
    ia = np.arange(len(rows_a)) if idx_a is None else np.asarray(idx_a, dtype=np.int64)
    ib = np.arange(len(rows_b)) if idx_b is None else np.asarray(idx_b, dtype=np.int64)
    ok = (ia >= 0) & (ia < len(rows_a)) & (ib >= 0) & (ib < len(rows_b))
    out = np.full((len(ia), 2), np.nan)
    if ok.any():
        t = log_ratio(rows_a[ia[ok], 1:], rows_b[ib[ok], 1:], k_bins, mutant=mutant)
        with np.errstate(all="ignore"):
            out[ok, 0] = np.sum(t, axis=1)
            out[ok, 1] = np.sum(t * t, axis=1)
    return out


def gamma(n):
    return n * U / (1.0 - n * U)


def sum_bounds(t_exact, p):
    """(b1, b2) [F] of the docstring from the exact t [F][K] (any float type)."""
    t = np.abs(np.asarray(t_exact, dtype=np.float64))
    k = t.shape[1]
    e_q = gamma(4 * p + 9) / (1.0 - gamma(4 * p + 9))
    e_t = e_q + 2.0 * U * (t + e_q)
    b1 = np.sum(e_t, axis=1) + gamma(k - 1) * np.sum(t + e_t, axis=1)
    b2 = np.sum(e_t * (2.0 * t + e_t), axis=1) + (U + gamma(k - 1) * (1.0 + U)) * np.sum((t + e_t) ** 2, axis=1)
    return b1, b2


def order_bounds(t):
    """(b1, b2) [F] between two evaluations that share q bit for bit and differ in the logarithm's last ulp and in the
    order of the sums (docstring, last paragraph); t [F][K] is either side's."""
    t = np.abs(np.asarray(t, dtype=np.float64))
    k = t.shape[1]
    e_t = 4.0 * U * t
    b1 = np.sum(e_t, axis=1) + 2.0 * gamma(k - 1) * np.sum(t + e_t, axis=1)
    b2 = np.sum(e_t * (2.0 * t + e_t), axis=1) + 2.0 * (U + gamma(k - 1) * (1.0 + U)) * np.sum((t + e_t) ** 2, axis=1)
    return b1, b2


# ---- dB ------------------------------------------------------------------------------------------------------------------
def distortion_db(g, s1, s2, k_bins, gain=True):
    g, s1, s2 = (np.asarray(a, dtype=np.float64) for a in (g, s1, s2))
    m1, m2 = s1 / k_bins, s2 / k_bins
    with np.errstate(all="ignore"):
        v = (g * g - 2.0 * g * m1 + m2) if gain else (m2 - m1 * m1)
        return LSD_SCALE * np.sqrt(np.maximum(v, 0.0))


def db_bound(g, s1, s2, b1, b2, k_bins, gain=True):
    """How far distortion_db moves when s1 and s2 move by up to b1 and b2, plus its own roundings: the radicand v moves by
    dv = 2 |g| b1 / K + b2 / K (gain) or b2 / K + (2 |s1| / K + b1 / K) b1 / K (no gain), its evaluation rounds each of at most
    eight operations on terms bounded by T = g^2 + 2 |g s1| / K + |s2| / K (resp. |s2| / K + (s1 / K)^2), and
    |sqrt(v + dv) - sqrt(v)| <= min(sqrt(dv), dv / sqrt(v)) (<= sqrt(dv) always: a radicand clamped at 0 included)."""
    g, s1, s2 = (np.abs(np.asarray(a, dtype=np.float64)) for a in (g, s1, s2))
    if gain:
        dv = 2.0 * g * b1 / k_bins + b2 / k_bins
        big = g * g + 2.0 * g * s1 / k_bins + s2 / k_bins
        v = np.maximum(g * g - 2.0 * g * s1 / k_bins + s2 / k_bins, 0.0)
    else:
        dv = b2 / k_bins + (2.0 * s1 / k_bins + b1 / k_bins) * b1 / k_bins
        big = s2 / k_bins + (s1 / k_bins) ** 2
        v = np.maximum(s2 / k_bins - (s1 / k_bins) ** 2, 0.0)
    dv = dv + 8.0 * U * big
    with np.errstate(all="ignore"):
        move = np.minimum(np.sqrt(dv), np.where(v > 0, dv / np.sqrt(np.where(v > 0, v, 1.0)), np.inf))
    return LSD_SCALE * (move + 4.0 * U * np.sqrt(v + dv))


def lsd_long_double(rows_a, rows_b, k_bins, gain=True):
    """[F] dB from rows [log E, w_1 .. w_p] (radians) by the definition: 10 log10 of the ratio of the two envelopes
    E / A2, RMS over the bins, everything in long double (gain=False: the mean over the bins taken out first)."""
    rows_a, rows_b = np.asarray(rows_a, dtype=np.float64), np.asarray(rows_b, dtype=np.float64)
    k = k_bins
    sa = np.exp(rows_a[:, :1].astype(LD)) / a2(np.cos(rows_a[:, 1:]), k, LD)
    sb = np.exp(rows_b[:, :1].astype(LD)) / a2(np.cos(rows_b[:, 1:]), k, LD)
    d = LD(10.0) * np.log10(sa / sb)
    if not gain:
        d = d - np.mean(d, axis=1, keepdims=True)
    return np.sqrt(np.mean(d * d, axis=1))
