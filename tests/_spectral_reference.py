"""Plain high-precision references for the pieces between the transforms and the outputs of CheapTrick and D4C, and the
comparators the GPU tests judge the kernels with (tests/test_hip_d4c_select.py, tests/test_hip_spectral_helpers.py;
tests/test_spectral_reference_host.py checks this file against the oracle and against deliberate mistakes, on the CPU).

Selection (sum_smallest, csrc/wh_d4c_select.h; world/d4c.py:206-208): sort, then the exactly rounded sum of the first m values
(math.fsum), or Python integers where the data are integers.  The bound for data that are not: summing K non-negative
terms in ANY order is off by at most (K - 1) u times the sum, u = 2^-53 (each of the K - 1 additions rounds a partial sum
that is at most the total; first order in u) — so a selection that is right differs from the reference by no more than
that, whatever the distribution of the values over threads and waves.

Smoothing (BandWindow, csrc/wh_spectral.h): the windowed-sum identity of that header's comment,
    band(k) = sum_{i = k+b_lo+1}^{k+b_hi} v[i]  +  f_hi v[k+b_hi+1]  -  f_lo v[k+b_lo+1],     v = mirrored spectrum * fs / N,
every term exact (the two products split into head and tail), summed and rounded once by math.fsum.  b_lo, b_hi, f_lo, f_hi
are frame constants: they are computed in float64 by the kernel's own expressions (a floor taken in another precision is a
different question).  The bound for bin k0 + r of a run that starts at k0, W = b_hi - b_lo:
    |got - band| <= (W + 2 r + 6) u A,     A = sum of |v| over every index the run has touched up to step r.
Derivation: the first window is a sum of W terms in some order, at most (W - 1) u A; every slide s += v[hi] - v[lo] rounds
twice (the difference, at most u (|v[hi]| + |v[lo]|), and the sum, at most u |s|), both at most u A: 2 r u A after r
slides; the output (s + f_hi v) - f_lo v rounds two to four times more (fused or not), each at most u A; the reference
itself is rounded once, u / 2 of its own size.  W - 1 + 2 r + 4.5 <= W + 2 r + 6.  What the bound does NOT promise is
accuracy relative to the OUTPUT: a large bin that has left the window stays in A — u times that bin stays in s.

Replica (low_band_replica, low_band_replica_runs; world/cheaptrick.py:67-73, world/d4c.py:213-220): the nodes f0 - f_j of
the bins with f_j < reach, ascending; bin k with f_k < f0 gets slope * (f_k - x_lo) + y_lo of the bracketing pair
(end segments extrapolate) added.  Which bins are nodes, which are touched and which pair brackets are decisions on
float64 values and taken in float64 here as in the reference; the arithmetic on the chosen pair runs in np.longdouble.
The bound per touched bin, 4 u (|slope dx| + |y_lo| + |p[k]|): the quotient of two rounded differences times a rounded
difference is off by about 4 u of itself, the two additions by u of their results each."""
import math

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
D4C_FT = {512: 256, 1024: 128, 2048: 256, 4096: 512, 8192: 512}  # threads per frame at N: ft_of(n), csrc/wh_d4c_types.h


# ---- selection ----------------------------------------------------------------------------------------------------------
def select_reference(row, m, integer=False):
    """(sum of the m smallest, sum of all) of one row: Python ints where `integer`, else exactly rounded floats."""
    s = np.sort(np.asarray(row, dtype=np.float64))
    if integer:
        v = [int(x) for x in s]
        assert all(float(a) == b for a, b in zip(v, s))
        return sum(v[:m]), sum(v)
    return math.fsum(s[:m]), math.fsum(s)


def select_bound(k, ref):
    return (k - 1) * U * ref


def selection_failures(got, rows, m, exact):
    """Rows of `got` (count, 2) that are not the selection of `rows` (count, K): [(row, 'small' | 'total', got, reference)].
    exact: the sums must BE the integer sums; else within select_bound."""
    rows = np.asarray(rows, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == (rows.shape[0], 2)
    bad = []
    for c in range(rows.shape[0]):
        ref = select_reference(rows[c], m, integer=exact)
        for j, name in enumerate(("small", "total")):
            g = float(got[c, j])
            if exact:
                ok = math.isfinite(g) and g == float(int(g)) and int(g) == ref[j]
            else:
                ok = math.isfinite(g) and abs(LD(g) - LD(ref[j])) <= LD(select_bound(rows.shape[1], ref[j]))
            if not ok:
                bad.append((c, name, g, ref[j]))
    return bad


def d4c_fft_size(fs):
    return int(round(2.0 ** math.ceil(math.log2(4 * fs / 47.0 + 1))))


def d4c_boundary(fs, n=None):
    """`boundary` of d4c_launch_const (csrc/wh_d4c_types.h; world/d4c.py:197-199) at d4c()'s own transform length and band
    interval for the rate: the band stage leaves boundary + 1 values out."""
    n = n or d4c_fft_size(fs)
    interval = 2000 if fs < 16000 else 3000
    wlen = int(math.floor(interval / (fs / n)) * 2 + 1)
    return int(float(n) / wlen * 8 + 0.5)


# ---- smoothing ----------------------------------------------------------------------------------------------------------
def band_constants(n, fs, half):
    """(b_lo, b_hi, f_lo, f_hi) by BandWindow::init's own float64 expressions."""
    n, fs, half = int(n), float(fs), float(half)
    half_bin = fs / n / 2
    x0 = (0.0 / n * fs - fs) + half_bin
    x1 = (1.0 / n * fs - fs) + half_bin
    inv_dx = 1.0 / (x1 - x0)
    q_lo = ((0.0 - half) - x0) * inv_dx
    q_hi = ((0.0 + half) - x0) * inv_dx
    fl, fh = math.floor(q_lo), math.floor(q_hi)
    return int(fl), int(fh), q_lo - fl, q_hi - fh


def mirrored(p_half, n, fs):
    """v[0..n): the Hermitian mirror of the half spectrum times fs / n (fill_mirrored: one rounding per element, the same
    one the kernel makes)."""
    p = np.asarray(p_half, dtype=np.float64)
    assert p.shape == (n // 2 + 1,)
    return np.concatenate([p, p[-2:0:-1]]) * (float(fs) / n)


def _two_prod(a, b):
    """a * b = p + e exactly (Dekker; no overflow or underflow at the sizes used here)."""
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah = ca - (ca - a)
    bh = cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def band_reference(v, n, consts, ks=None, out=None):
    """band(k) of the header's identity for k in ks (default: all K bins), each the exactly rounded value of its exact sum."""
    b_lo, b_hi, f_lo, f_hi = consts
    w = b_hi - b_lo
    assert 0 <= w < n and len(v) == n
    mask = n - 1
    vl = v if isinstance(v, list) else [float(x) for x in v]
    vv = vl + vl
    if out is None:
        out = np.empty(n // 2 + 1)
    for k in (range(n // 2 + 1) if ks is None else ks):
        start = (k + b_lo + 1) & mask
        p1, e1 = _two_prod(f_hi, vl[(k + b_hi + 1) & mask])
        p0, e0 = _two_prod(f_lo, vl[start])
        out[k] = math.fsum(vv[start:start + w] + [p1, e1, -p0, -e0])
    return out


def band_integer_reference(p_half_int, n, fs, half):
    """The same for an integer spectrum at a dyadic fs / n with f_lo, f_hi in {0, 0.5}: integer arithmetic (running sums in
    int64), every value exact in float64."""
    b_lo, b_hi, f_lo, f_hi = band_constants(n, fs, half)
    assert f_lo in (0.0, 0.5) and f_hi in (0.0, 0.5) and 0 <= b_hi - b_lo < n
    p = np.asarray(p_half_int, dtype=np.int64)
    assert p.shape == (n // 2 + 1,) and 0 <= p.min() and p.max() < 2 ** 20
    full = np.concatenate([p, p[-2:0:-1]])
    c = np.concatenate([[0], np.cumsum(np.concatenate([full, full]))])
    k = np.arange(n // 2 + 1)
    start = (k + b_lo + 1) & (n - 1)
    twice = 2 * (c[start + (b_hi - b_lo)] - c[start])
    twice += int(2 * f_hi) * full[(k + b_hi + 1) & (n - 1)] - int(2 * f_lo) * full[start]
    assert np.abs(twice).max() < 2 ** 45
    return twice.astype(np.float64) * (float(fs) / n / 2)  # (fs / n dyadic with few bits: the product is exact)


def run_touched(n, consts, kr):
    """(start, length) per bin k = k0 + r of the index range [k0 + b_lo + 1, k0 + r + b_hi + 1] (modulo n) that the run
    owning k has read by the time it writes k; kr: bins per run."""
    b_lo, b_hi, _, _ = consts
    k = np.arange(n // 2 + 1)
    r = k % kr
    return ((k - r) + b_lo + 1) & (n - 1), (b_hi - b_lo) + 1 + r


def in_touched(n, consts, kr, index):
    """Per bin: whether element `index` of v lies in the range of run_touched."""
    start, length = run_touched(n, consts, kr)
    return ((int(index) - start) & (n - 1)) < length


def band_bound(v, n, consts, kr):
    """((W + 2 r + 6) u A, A) per bin (module docstring); A from running sums in long double."""
    start, length = run_touched(n, consts, kr)
    a = np.abs(np.asarray(v, dtype=np.float64)).astype(LD)
    assert int(length.max()) <= n
    c = np.concatenate([[LD(0)], np.cumsum(np.concatenate([a, a]))])
    big = (c[start + length] - c[start]).astype(np.float64)
    return band_factor(n, consts, kr) * U * big, big


def band_factor(n, consts, kr):
    return (consts[1] - consts[0]) + 2 * (np.arange(n // 2 + 1) % kr) + 6


def band_add_peak(ref_ks, ks, n, consts, index, delta):
    """band(k) for k in ks after element `index` of v has grown by `delta` (np.longdouble): the element's weight in bin k is
    1 inside the window, f_hi just above it, less f_lo on the window's first element.  ref_ks: band(k) before, long double.
    Evaluated in long double, so off by 2^-62 |delta| at most: with a base that was rounded once to float64 the reference
    stays within 0.502 u A of the truth, where the derivation of the bound allows it 0.5 u A of its 1.5 u A to spare."""
    b_lo, b_hi, f_lo, f_hi = consts
    e = ((int(index) - np.asarray(ks)) - (b_lo + 1)) & (n - 1)
    coef = (e < (b_hi - b_lo)).astype(LD) + LD(f_hi) * (e == (b_hi - b_lo)) - LD(f_lo) * (e == 0)
    return ref_ks + coef * delta


def band_failures(got, ref, bound):
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got.astype(LD) - np.asarray(ref).astype(LD))
    return [int(i) for i in np.nonzero(~(np.isfinite(got) & (err <= np.asarray(bound).astype(LD))))[0]]


# ---- replica ------------------------------------------------------------------------------------------------------------
def replica_nlow(n, fs, reach, cap):
    """Count of bins with k / n * fs < reach, at most cap (the kernels' closed form settled by the float64 predicate)."""
    nlow = min(int(float(reach) / fs * n) + 2, cap)
    while nlow > 0 and not ((nlow - 1) / n * fs < reach):
        nlow -= 1
    assert nlow == cap or not (nlow / n * fs < reach)
    return nlow


def replica_reference(p_half, n, fs, f0, reach, cap, less=np.less):
    """(out, touched, bound): out = p with the replica added (np.longdouble), touched = the bins that receive it, bound per
    bin (0 where untouched: those must keep their bits).  cap: the bins that can be nodes — n for the LDS form (bins above
    n / 2 are the mirror images of the stored half), n / 2 + 1 for the run-resident form.  `less`: the comparison that
    decides whether a bin lies below f0 (np.less; the host test passes np.less_equal as a deliberate mistake)."""
    p = np.asarray(p_half, dtype=np.float64)
    k_bins = n // 2 + 1
    assert p.shape == (k_bins,)
    fs, f0, reach = float(fs), float(f0), float(reach)
    out, touched, bound = p.astype(LD), np.zeros(k_bins, dtype=bool), np.zeros(k_bins)
    nlow = replica_nlow(n, fs, reach, cap)
    if nlow < 2:
        return out, touched, bound
    j = np.arange(nlow)
    f = j / float(n) * fs                          # f_j as the kernels and the reference form it
    y_all = p[np.where(j <= n // 2, j, n - j)]
    a = (f0 - f)[::-1]                             # ascending nodes
    y = y_all[::-1]
    kk = np.arange(min(nlow, k_bins))
    kk = kk[less(f[kk], f0)]
    if len(kk) == 0:
        return out, touched, bound
    hi = np.clip(np.searchsorted(a, f[kk], side="left"), 1, nlow - 1)
    lo = hi - 1
    slope = (y[hi].astype(LD) - y[lo].astype(LD)) / (a[hi].astype(LD) - a[lo].astype(LD))
    dx = f[kk].astype(LD) - a[lo].astype(LD)
    out[kk] = (slope * dx + y[lo].astype(LD)) + p[kk].astype(LD)
    touched[kk] = True
    bound[kk] = (4 * U * (np.abs(slope * dx) + np.abs(y[lo].astype(LD)) + np.abs(p[kk].astype(LD)))).astype(np.float64)
    return out, touched, bound


def replica_failures(got, p_half, ref, touched, bound):
    """Bins where `got` is not the reference's replica: an untouched bin whose bits moved, a touched one beyond its bound."""
    got = np.asarray(got, dtype=np.float64)
    p = np.asarray(p_half, dtype=np.float64)
    same = got.view(np.int64) == p.view(np.int64)
    close = np.isfinite(got) & (np.abs(got.astype(LD) - ref) <= bound.astype(LD))
    return [int(i) for i in np.nonzero(~np.where(touched, close, same))[0]]
