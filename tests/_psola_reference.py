"""The contract of wh_psola (include/world_hip.h) in plain NumPy: time-domain pitch-synchronous
overlap-add.

Per call Params(grid G, hop U, tol, pmin, smin, norm); PMAX = 2048; eff(p) = p when pmin <= p <= PMAX, else 0 (unvoiced).
Per utterance x[0 .. n), an output length n_out and three tracks on the grid: per_a [n // G + 1] (the analysis period at
input sample k G), per_s [n_out // G + 1] (the target period at output sample k G) and src [n_out // G + 1] (the input
sample that output sample k G corresponds to, clamped to +- 2^62).  A read of x outside [0, n) is 0.0.

    stage A   a_0 = 0 (no marks when n == 0); P_i = eff(per_a[min(Ka - 1, a_i // G)]); a_i >= n ends the list with that
              mark in it; P_i == 0: a_{i+1} = a_i + U; else h = P_i // 2, D = min(tol, P_i // 4), template
              x[a_i - h + j], j < P_i, candidates x[a_i + P_i + d - h + j], d in [-D, D], wh_wsola's score and choice
              (tests/_wsola_reference.py: scores, choose), a_{i+1} = a_i + P_i + d*.
    stage B   s_0 = 0 (no marks when n_out == 0 or there is no analysis mark); k = min(Ks - 1, s_j // G);
              c = src[k] + (s_j - k G); sel_j = the nearest analysis mark to c, the lower on a tie; flip_j = 1 iff j >= 1,
              P_sel == 0, sel_j == sel_{j-1} and flip_{j-1} == 0; s_j >= n_out ends the list with that mark in it; with
              Q = eff(per_s[k]): Q > 0 and P_sel > 0: sp = a_{sel+1} - a_sel (P_sel at the last mark),
              step = max(smin, (sp Q + P_sel // 2) // P_sel); else step = U.
    stage C   grain j around i = sel_j: fb = P_i or U, Lw = a_i - a_{i-1} (fb at i == 0), Rw = a_{i+1} - a_i (fb at the last
              mark); tau = t - s_j, -Lw < tau < Rw: u = |tau| / (Lw or Rw), w = 1 - (u u) (3 - 2 u),
              v = x[a_i + (-tau if flip_j else tau)], num += w v, W += w, j ascending from +0.0, unfused;
              y[t] = num / max(W, 1.0) with norm, else num.

psola() is vectorised (over the candidates in stage A, over a grain's samples in stage C: NumPy's elementwise operations
round each result on its own); psola_scalar() is the same contract as scalar loops, for tiny inputs.  Everything — marks,
periods, synthesis marks, selection, flips and y — is compared bit for bit."""
import bisect
import collections
import math

import numpy as np

import _wsola_reference as wref

PMAX, MAX_GRID, MAX_HOP, MAX_TOL = 2048, 4096, 2048, 512
FAR = 2 ** 62
Params = collections.namedtuple("Params", "grid hop tol pmin smin norm")
MUTANTS = ("fused_sum", "pairwise_sum", "ties_lowest_index", "no_terminal_mark", "running_pointer", "hanning_window",
           "step_from_q", "clipped_read", "flip_dropped")


def check_params(p):
    for name, v, lo, hi in (("grid", p.grid, 1, MAX_GRID), ("hop", p.hop, 1, MAX_HOP), ("tol", p.tol, 0, MAX_TOL),
                            ("pmin", p.pmin, 2, PMAX), ("smin", p.smin, 1, PMAX), ("norm", p.norm, 0, 1)):
        if not lo <= int(v) <= hi:
            raise ValueError("%s = %r outside [%d, %d]" % (name, v, lo, hi))


def eff(period, pmin):
    period = int(period)
    return period if pmin <= period <= PMAX else 0


def min_step(p):
    """Every analysis step is at least this many samples."""
    return min(p.hop, p.pmin - min(p.tol, p.pmin // 4))


def mark_capacity(n, p):
    return -(-int(n) // min_step(p)) + 1


def smark_capacity(n_out, p):
    return -(-int(n_out) // min(p.hop, p.smin)) + 1


def analysis_marks(x, per_a, p, mutant=None):
    """(marks int64 [Ma], periods int32 [Ma])."""
    x = np.asarray(x, dtype=np.float64)
    n, G = len(x), p.grid
    if len(per_a) != n // G + 1:
        raise ValueError("%d analysis periods for %d samples on a grid of %d" % (len(per_a), n, G))
    marks, periods = [], []
    clipped = mutant == "clipped_read"
    a = 0
    while n > 0:
        P = eff(per_a[min(len(per_a) - 1, a // G)], p.pmin)
        if a >= n:
            if mutant != "no_terminal_mark":
                marks.append(a), periods.append(P)
            break
        marks.append(a), periods.append(P)
        if P == 0:
            a += p.hop
            continue
        h, D = P // 2, min(p.tol, P // 4)
        t = wref.read(x, a - h, P, clipped)
        region = wref.read(x, a + P - D - h, P + 2 * D, clipped)
        a += P + wref.choose(wref.scores(t, region, D, mutant), D, mutant)
    return np.array(marks, dtype=np.int64), np.array(periods, dtype=np.int32)


def nearest(marks, c):
    """The index of the mark nearest to c in the increasing list, the lower one on a tie."""
    r = bisect.bisect_right(marks, c)
    if r == 0:
        return 0
    if r < len(marks) and marks[r] - c < c - marks[r - 1]:
        return r
    return r - 1


def synthesis_marks(marks, periods, n_out, per_s, src, p, mutant=None):
    """(smarks int64 [Ms], sel int32 [Ms], flip uint8 [Ms])."""
    G = p.grid
    if len(per_s) != n_out // G + 1 or len(src) != n_out // G + 1:
        raise ValueError("%d / %d target entries for %d samples on a grid of %d" % (len(per_s), len(src), n_out, G))
    a, P_of = [int(v) for v in marks], [int(v) for v in periods]
    smarks, sel, flip = [], [], []
    s, prev_sel, prev_flip, ptr = 0, -1, 0, 0
    while n_out > 0 and a:
        k = min(len(src) - 1, s // G)
        c = min(max(int(src[k]), -FAR), FAR) + (s - k * G)
        if mutant == "running_pointer":
            while ptr + 1 < len(a) and abs(a[ptr + 1] - c) < abs(a[ptr] - c):
                ptr += 1
            i = ptr
        else:
            i = nearest(a, c)
        P = P_of[i]
        fl = int(len(smarks) >= 1 and P == 0 and i == prev_sel and prev_flip == 0 and mutant != "flip_dropped")
        if s >= n_out and mutant == "no_terminal_mark":
            break
        smarks.append(s), sel.append(i), flip.append(fl)
        prev_sel, prev_flip = i, fl
        if s >= n_out:
            break
        Q = eff(per_s[k], p.pmin)
        if Q > 0 and P > 0:
            sp = a[i + 1] - a[i] if i + 1 < len(a) else P
            s += max(p.smin, Q if mutant == "step_from_q" else (sp * Q + P // 2) // P)
        else:
            s += p.hop
    return np.array(smarks, dtype=np.int64), np.array(sel, dtype=np.int32), np.array(flip, dtype=np.uint8)


def widths(marks, periods, i, hop):
    fb = int(periods[i]) if periods[i] > 0 else hop
    left = int(marks[i] - marks[i - 1]) if i > 0 else fb
    right = int(marks[i + 1] - marks[i]) if i + 1 < len(marks) else fb
    return left, right


def _gather(x, idx, clipped):
    n = len(x)
    if clipped:  # (a mutant: the end samples repeated)
        return x[np.clip(idx, 0, n - 1)] if n else np.zeros(len(idx))
    out = np.zeros(len(idx), dtype=np.float64)
    ok = (idx >= 0) & (idx < n)
    out[ok] = x[idx[ok]]
    return out


def overlap_add(x, marks, periods, smarks, sel, flip, n_out, p, mutant=None):
    x = np.asarray(x, dtype=np.float64)
    num, wsum = np.zeros(n_out, dtype=np.float64), np.zeros(n_out, dtype=np.float64)
    with np.errstate(all="ignore"):
        for j in range(len(smarks)):
            i, s = int(sel[j]), int(smarks[j])
            left, right = widths(marks, periods, i, p.hop)
            lo, hi = max(0, s - left + 1), min(n_out, s + right)
            if hi <= lo:
                continue
            tau = np.arange(lo, hi, dtype=np.int64) - s
            u = np.abs(tau).astype(np.float64) / np.where(tau < 0, left, right).astype(np.float64)
            w = 0.5 + 0.5 * np.cos(np.pi * u) if mutant == "hanning_window" else 1.0 - (u * u) * (3.0 - 2.0 * u)
            v = _gather(x, int(marks[i]) + (-tau if flip[j] else tau), mutant == "clipped_read")
            num[lo:hi] = wref._fma(w, v, num[lo:hi]) if mutant == "fused_sum" else num[lo:hi] + w * v
            wsum[lo:hi] = wsum[lo:hi] + w
        return num / np.maximum(wsum, 1.0) if p.norm else num


def psola(x, n_out, per_a, per_s, src, p, mutant=None):
    """{y, marks, periods, smarks, sel, flip} of one utterance."""
    check_params(p)
    marks, periods = analysis_marks(x, per_a, p, mutant)
    smarks, sel, flip = synthesis_marks(marks, periods, n_out, per_s, src, p, mutant)
    y = overlap_add(x, marks, periods, smarks, sel, flip, n_out, p, mutant)
    return {"y": y, "marks": marks, "periods": periods, "smarks": smarks, "sel": sel, "flip": flip}


def psola_scalar(x, n_out, per_a, per_s, src, p):
    """The contract as scalar loops (Python floats are IEEE doubles; every operation is rounded on its own)."""
    check_params(p)
    x = [float(v) for v in x]
    n, G, U = len(x), p.grid, p.hop

    def rd(i):
        return x[i] if 0 <= i < n else 0.0

    marks, periods = [], []
    a = 0
    while n > 0:
        P = eff(per_a[min(n // G, a // G)], p.pmin)
        marks.append(a), periods.append(P)
        if a >= n:
            break
        if P == 0:
            a += U
            continue
        h, D = P // 2, min(p.tol, P // 4)
        best = None
        for d in range(-D, D + 1):
            num = den = 0.0
            for j in range(P):
                t, g = rd(a - h + j), rd(a + P + d - h + j)
                num = num + t * g
                den = den + g * g
            if den > 0:
                # (Python raises where IEEE gives inf or NaN)
                r = math.sqrt(den) if math.isfinite(den) else math.inf
                if math.isfinite(num) and math.isfinite(r):
                    sc = num / r
                else:
                    with np.errstate(all="ignore"):
                        sc = float(np.float64(num) / np.float64(r))
            else:
                sc = 0.0
            if sc != sc:
                sc = -math.inf
            if best is None or sc > best[0] or (sc == best[0] and (abs(d) < abs(best[1]) or (abs(d) == abs(best[1]) and d < best[1]))):
                best = (sc, d)
        a += P + best[1]
    smarks, sel, flip = [], [], []
    s = 0
    while n_out > 0 and marks:
        k = min(n_out // G, s // G)
        c = min(max(int(src[k]), -FAR), FAR) + (s - k * G)
        i = 0
        for q in range(1, len(marks)):  # (strictly nearer only: the lower index keeps a tie)
            if abs(marks[q] - c) < abs(marks[i] - c):
                i = q
        P = periods[i]
        fl = int(len(smarks) >= 1 and P == 0 and i == sel[-1] and flip[-1] == 0)
        smarks.append(s), sel.append(i), flip.append(fl)
        if s >= n_out:
            break
        Q = eff(per_s[k], p.pmin)
        if Q > 0 and P > 0:
            sp = marks[i + 1] - marks[i] if i + 1 < len(marks) else P
            s += max(p.smin, (sp * Q + P // 2) // P)
        else:
            s += U
    y = [0.0] * n_out
    for t in range(n_out):
        num = wsum = 0.0
        for j in range(len(smarks)):
            left, right = widths(marks, periods, sel[j], U)
            tau = t - smarks[j]
            if -left < tau < right:
                u = float(abs(tau)) / float(left if tau < 0 else right)
                w = 1.0 - (u * u) * (3.0 - 2.0 * u)
                v = rd(marks[sel[j]] + (-tau if flip[j] else tau))
                num = num + w * v  # (Python floats: inf and NaN propagate through * and + without an exception)
                wsum = wsum + w
        y[t] = num / max(wsum, 1.0) if p.norm else num
    return {"y": np.array(y, dtype=np.float64), "marks": np.array(marks, dtype=np.int64), "periods": np.array(periods, dtype=np.int32),
            "smarks": np.array(smarks, dtype=np.int64), "sel": np.array(sel, dtype=np.int32), "flip": np.array(flip, dtype=np.uint8)}
