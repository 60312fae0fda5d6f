"""The contract of wh_wsola (include/world_hip.h) in plain NumPy: waveform-similarity overlap-add.

Per call an integer hop H (1 .. 1024), a tolerance D (0 .. 512), L = 2 H - 1 and the window win[j] = 0.5 - 0.5 cos(pi (j + 1) / H),
j < L (win[j] + win[j + H] = 1).  Per utterance x[0 .. n), an output length n_out, M = ceil(n_out / H) + 1 frames (none when
n_out == 0) and pos[0 .. M), the nominal input start of every frame.  A read of x outside [0, n) is 0.0; nothing is clipped.

    chain     delta_0 = 0;  c_m = pos[m] + delta_m;  for m >= 1 the template is t[j] = x[c_{m-1} + H + j], j < L, and
              candidate d in [-D, D] is g_d[j] = x[pos[m] + d + j].
    score     num = sum_j t[j] * g_d[j], den = sum_j g_d[j] * g_d[j], from +0.0, j ascending, every product and sum rounded on
              its own;  score = num / sqrt(den) when den > 0, else 0.0;  a NaN score counts as -inf.
    choice    the greatest score; among equal scores the smallest |d|, then the negative one.
    output    o_m = m H - H;  y[t] = sum over the frames with 0 <= t - o_m < L, m ascending, of win[t - o_m] x[c_m + t - o_m],
              from +0.0 and unfused.

wsola() is a loop over j with vector operations over the candidates (NumPy's elementwise multiply and add round each
result on its own); wsola_scalar() is the same contract as nested scalar loops, for tiny inputs.  The shifts and y are
compared bit for bit."""
import numpy as np

MAX_HOP, MAX_TOL = 1024, 512
MUTANTS = ("pairwise_sum", "fused_sum", "ties_lowest_index", "no_normalisation", "template_from_pos", "clipped_read")


def n_frames(n_out, hop):
    return 0 if n_out <= 0 else -(-int(n_out) // int(hop)) + 1


def window(hop):
    j = np.arange(2 * int(hop) - 1, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(np.pi * (j + 1.0) / float(hop))


def positions(n_out, hop, ratio):
    """floor((m H - 1) / ratio + 0.5) - (H - 1) in float64: the frame whose output centre is m H - 1 is taken around the
    input sample (m H - 1) / ratio."""
    m = np.arange(n_frames(n_out, hop), dtype=np.float64)
    return (np.floor((m * float(hop) - 1.0) / float(ratio) + 0.5) - (float(hop) - 1.0)).astype(np.int64)


def read(x, start, length, clipped=False):
    """x[start .. start + length) with 0.0 outside [0, n) (Python integers: any start)."""
    start, n = int(start), len(x)
    if clipped:  # (a mutant: the end samples repeated)
        return x[np.clip(np.arange(start, start + length), 0, max(n - 1, 0))] if n else np.zeros(length)
    out = np.zeros(length, dtype=np.float64)
    lo, hi = max(start, 0), min(start + length, n)
    if hi > lo:
        out[lo - start:hi - start] = x[lo:hi]
    return out


def _fma(a, b, c):
    """a * b + c rounded once (exact product by Dekker's splitting; enough for a mutant)."""
    import math
    from fractions import Fraction
    out = np.empty(len(a))
    for i in range(len(a)):
        if not (math.isfinite(a[i]) and math.isfinite(b[i]) and math.isfinite(c[i])):
            out[i] = a[i] * b[i] + c[i]
        else:
            out[i] = float(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
    return out


def scores(t, region, tol, mutant=None):
    """The 2 D + 1 scores of a frame: t [L], region [L + 2 D] = x[pos - D ..]."""
    ncand, length = 2 * tol + 1, len(t)
    with np.errstate(all="ignore"):
        if mutant == "pairwise_sum":
            g = np.lib.stride_tricks.sliding_window_view(region, length)
            num, den = np.sum(t[None, :] * g, axis=1), np.sum(g * g, axis=1)
        else:
            num, den = np.zeros(ncand), np.zeros(ncand)
            for j in range(length):
                g = region[j:j + ncand]
                if mutant == "fused_sum":
                    num, den = _fma(np.full(ncand, t[j]), g, num), _fma(g, g, den)
                else:
                    num = num + t[j] * g
                    den = den + g * g
        if mutant == "no_normalisation":
            s = num.copy()
        else:
            s = np.where(den > 0, num / np.sqrt(np.where(den > 0, den, 1.0)), 0.0)
        s[np.isnan(s)] = -np.inf
    return s


def choose(s, tol, mutant=None):
    """The shift of the greatest score; ties: the smallest |d|, then the negative one."""
    idx = np.flatnonzero(s == np.max(s))
    if mutant == "ties_lowest_index":
        return int(idx[0]) - tol
    d = idx - tol
    return int(d[np.lexsort((d, np.abs(d)))[0]])


def search(x, pos, hop, tol, mutant=None):
    """(delta int32 [M], c: list of Python integers)."""
    x = np.asarray(x, dtype=np.float64)
    length = 2 * hop - 1
    clipped = mutant == "clipped_read"
    delta, c = np.zeros(len(pos), dtype=np.int32), []
    for m in range(len(pos)):
        p = int(pos[m])
        if m == 0:
            c.append(p)
            continue
        start = (int(pos[m - 1]) if mutant == "template_from_pos" else c[m - 1]) + hop
        t = read(x, start, length, clipped)
        region = read(x, p - tol, length + 2 * tol, clipped)
        delta[m] = choose(scores(t, region, tol, mutant), tol, mutant)
        c.append(p + int(delta[m]))
    return delta, c


def overlap_add(x, c, n_out, hop, clipped=False):
    x = np.asarray(x, dtype=np.float64)
    length, win = 2 * hop - 1, window(hop)
    y = np.zeros(n_out, dtype=np.float64)
    with np.errstate(all="ignore"):
        for m in range(len(c)):
            o = m * hop - hop
            lo, hi = max(o, 0), min(o + length, n_out)
            if hi > lo:
                seg = read(x, c[m], length, clipped)
                y[lo:hi] = y[lo:hi] + win[lo - o:hi - o] * seg[lo - o:hi - o]
    return y


def wsola(x, n_out, pos, hop, tol, mutant=None):
    """(y float64 [n_out], delta int32 [M]) of one utterance."""
    if not (1 <= hop <= MAX_HOP and 0 <= tol <= MAX_TOL):
        raise ValueError("hop %r or tolerance %r outside the contract" % (hop, tol))
    if len(pos) != n_frames(n_out, hop):
        raise ValueError("%d positions for %d frames" % (len(pos), n_frames(n_out, hop)))
    delta, c = search(x, pos, hop, tol, mutant)
    return overlap_add(x, c, n_out, hop, mutant == "clipped_read"), delta


def wsola_scalar(x, n_out, pos, hop, tol):
    """The contract as scalar loops (Python floats are IEEE doubles; every operation is rounded on its own)."""
    import math
    x = [float(v) for v in x]
    n, length = len(x), 2 * hop - 1
    win = [float(v) for v in window(hop)]

    def rd(i):
        return x[i] if 0 <= i < n else 0.0

    c, delta = [], []
    for m in range(len(pos)):
        p = int(pos[m])
        if m == 0:
            c.append(p), delta.append(0)
            continue
        best = None
        for d in range(-tol, tol + 1):
            num = den = 0.0
            for j in range(length):
                t, g = rd(c[m - 1] + hop + j), rd(p + d + j)
                num = num + t * g
                den = den + g * g
            if den > 0:
                # (Python raises where IEEE gives inf or NaN)
                r = math.sqrt(den) if math.isfinite(den) else math.inf
                s = num / r if math.isfinite(num) and math.isfinite(r) else float(np.float64(num) / np.float64(r))
            else:
                s = 0.0
            if s != s:
                s = -math.inf
            if best is None or s > best[0] or (s == best[0] and (abs(d) < abs(best[1]) or (abs(d) == abs(best[1]) and d < best[1]))):
                best = (s, d)
        delta.append(best[1]), c.append(p + best[1])
    y = [0.0] * n_out
    for t in range(n_out):
        for m in range(len(pos)):
            j = t - (m * hop - hop)
            if 0 <= j < length:
                y[t] = y[t] + win[j] * rd(c[m] + j)
    return np.array(y, dtype=np.float64), np.array(delta, dtype=np.int32)
