"""Harvest's last stages restated one at a time, with branch counters: RemoveUnreliableCandidates, FixF0Contour (base pick,
FixStep1-4 with ExtendF0 and MergeF0) and SmoothF0, world/harvest.py:215-248, 301-495, 533-580.  Written from
oracle/pitch_harvest.py and the line references there, NOT from the kernels: tests/test_harvest_contour_reference_host.py
holds it against the oracle and against the reference's recorded results (tests/golden/golden_harvest_contour.npz) bit for
bit, tests/test_hip_harvest_contour.py holds wh_hv_refine.hip's prune and wh_hv_contour.hip's kernels against it.

Everything works on a dense candidate map: cands / scores of shape (rows, frames), zero = no candidate.  `run` returns a
Result whose fields are the stages' outputs and whose `count` (a collections.Counter) says which branches the input took:

  prune_killed / prune_kept        non-zero candidates of the inner frames that RemoveUnreliableCandidates zeroed / left
  prune_kept_by_prev_only / ..._by_next_only   survivors that only one neighbour frame vouches for
  prune_killed_word0..3            killed candidates by 32-row group of the row index
  base_row_ge64, base_max_twice    base picks from rows 64 and up; frames whose best score is held by two rows
  step1_drop, step2_removed        frames FixStep1 zeroed; runs FixStep2 removed
  fwd_stop_miss / fwd_stop_limit / bwd_stop_miss / bwd_stop_limit   how each ExtendF0 walk ended
  fwd_miss_at_step_mod4_0..3 / bwd_...   the step (counted from the section's end) on which the fourth miss fell, modulo 4
  fwd_clamped / bwd_clamped        walks whose limit was the contour's end (len - 2, resp. 1), not origin +- 100
  ext_three_miss_then_hit          a hit right after three misses
  pick_multi, pick_tie, pick_row_ge64   SelectBestF0 calls of the extension with >= 2 different values in range; with two
                                   different values at exactly the same, smallest error; with the winner in rows 64 and up
  pick_at_limit                    calls whose winner's error equals the allowed range exactly
  sec_total, sec_not_kept, no_section_kept
  merge_disjoint / merge_covered / merge_partial_first / merge_partial_second / merge_partial_equal
  merge_partial_after_disjoint     a partial merge after an earlier disjoint one (the running range matters)
  merge_score_row_ge64             SerachScore matches found in rows 64 and up
  tied_starts                      kept sections whose extended start another kept section shares
  step4_bridged / step4_left       unvoiced gaps FixStep4 filled / left
  smooth_runs
"""
import collections

import numpy as np
from scipy import signal

EPS = 2.220446049250313e-16
SMOOTH_B = np.array([0.0078202080334971724, 0.015640416066994345, 0.0078202080334971724])
SMOOTH_A = np.array([1.0, -1.7347257688092754, 0.76600660094326412])


class Result:
    pass


def select_best(ref, col, allowed):
    """SelectBestF0, harvest.py:238-248 -> (best value, its error, its row or -1).  Later rows win ties."""
    best, best_err, best_row = 0.0, allowed, -1
    for k in np.flatnonzero(col):  # a zero candidate's error is exactly 1: it only ever 'wins' with the value 0
        e = abs(ref - col[k]) / ref
        if e > best_err:
            continue
        best, best_err, best_row = col[k], e, int(k)
    return best, best_err, best_row


def prune(cands, scores, count=None):
    """RemoveUnreliableCandidates, harvest.py:215-234."""
    count = collections.Counter() if count is None else count
    out_c, out_s = np.array(cands, dtype=np.float64), np.array(scores, dtype=np.float64)
    n = cands.shape[1]
    for i in range(1, n - 1):
        for j in np.flatnonzero(cands[:, i]):
            ref = cands[j, i]
            e1 = select_best(ref, cands[:, i + 1], 1.0)[1]
            e2 = select_best(ref, cands[:, i - 1], 1.0)[1]
            if min(e1, e2) > 0.05:
                out_c[j, i] = 0
                out_s[j, i] = 0
                count["prune_killed"] += 1
                count["prune_killed_word%d" % (j // 32)] += 1
            else:
                count["prune_kept"] += 1
                if e1 > 0.05:
                    count["prune_kept_by_prev_only"] += 1
                if e2 > 0.05:
                    count["prune_kept_by_next_only"] += 1
    return out_c, out_s


def boundary_list(f0):
    """GetBoundaryList, harvest.py:572-580: [first0, last0, first1, last1, ...], the two end frames unvoiced."""
    v = (np.asarray(f0) != 0).astype(np.int64)
    v[0] = 0
    v[-1] = 0
    bl = np.flatnonzero(np.diff(v) != 0)
    bl[0::2] += 1
    return bl


def _pick(ref, col, allowed, count):
    best, err, row = select_best(ref, col, allowed)
    nz = np.flatnonzero(col)
    errs = np.array([abs(ref - col[k]) / ref for k in nz])
    ok = errs <= allowed
    vals = col[nz][ok]
    if len(set(vals.tolist())) >= 2:
        count["pick_multi"] += 1
        at_min = vals[errs[ok] == errs[ok].min()]
        if len(set(at_min.tolist())) >= 2:
            count["pick_tie"] += 1
    if row >= 64:
        count["pick_row_ge64"] += 1
    if row >= 0 and err == allowed:
        count["pick_at_limit"] += 1
    return best


def extend(f0, origin, last_point, shift, cands, allowed, count, tag):
    """ExtendF0, harvest.py:408-429 -> (extended contour, last frame reached)."""
    ext = np.array(f0)
    cur = ext[origin]
    reached = origin
    miss = 0
    stopped = False
    for step, i in enumerate(range(origin, last_point + shift, shift)):
        ext[i + shift] = _pick(cur, cands[:, i + shift], allowed, count)
        if ext[i + shift] != 0:
            if miss == 3:
                count["ext_three_miss_then_hit"] += 1
            cur = ext[i + shift]
            miss = 0
            reached = i + shift
        else:
            miss += 1
        if miss == 4:
            stopped = True
            count[tag + "_stop_miss"] += 1
            count["%s_miss_at_step_mod4_%d" % (tag, step % 4)] += 1
            break
    if not stopped:
        count[tag + "_stop_limit"] += 1
    return ext, reached


def search_score(f0, col, sc, count):
    """SerachScore, harvest.py:490-495."""
    s = 0
    for k in np.flatnonzero(col == f0):
        if s < sc[k]:
            s = sc[k]
            if k >= 64:
                count["merge_score_row_ge64"] += 1
    return s


def merge(channels, rng, cands, scores, count):
    """MergeF0 / MergeF0Sub, harvest.py:442-486, with a STABLE order of the extended starts (the reference asks for
    'quicksort', which NumPy does not promise to be stable)."""
    order = np.argsort(rng[:, 0], kind="stable")
    starts = rng[:, 0].tolist()
    count["tied_starts"] += sum(1 for v in starts if starts.count(v) > 1)
    f0 = np.array(channels[order[0]])
    R0, R1 = int(rng[order[0], 0]), int(rng[order[0], 1])
    seen_disjoint = False
    for q in range(1, len(order)):
        st2, ed2 = int(rng[order[q], 0]), int(rng[order[q], 1])
        f2 = channels[order[q]]
        if st2 - R1 > 0:
            count["merge_disjoint"] += 1
            seen_disjoint = True
            f0[st2 : ed2 + 1] = f2[st2 : ed2 + 1]
            R0, R1 = st2, ed2
            continue
        if R0 <= st2 and R1 >= ed2:
            count["merge_covered"] += 1
            continue
        s1 = 0
        s2 = 0
        for i in range(st2, R1 + 1):
            s1 = s1 + search_score(f0[i], cands[:, i], scores[:, i], count)
            s2 = s2 + search_score(f2[i], cands[:, i], scores[:, i], count)
        if seen_disjoint:
            count["merge_partial_after_disjoint"] += 1
        merged = f0.copy()
        if s1 > s2:
            count["merge_partial_first"] += 1
            merged[R1 : ed2 + 1] = f2[R1 : ed2 + 1]
        else:
            count["merge_partial_equal" if s1 == s2 else "merge_partial_second"] += 1
            merged[st2 : ed2 + 1] = f2[st2 : ed2 + 1]
        f0 = merged
        R1 = ed2
    return f0


def fix_contour(cands, scores, count=None):
    """FixF0Contour, harvest.py:301-404 -> Result(base, s1, s2, s3, s4, vuv, sections, means)."""
    count = collections.Counter() if count is None else count
    r = Result()
    n = cands.shape[1]
    # SearchF0Base: the first row holding the largest score
    top = np.argmax(scores, axis=0)
    r.base = cands[top, np.arange(n)]
    count["base_row_ge64"] += int(np.sum((top >= 64) & (r.base != 0)))
    count["base_max_twice"] += int(np.sum((np.sum(scores == scores.max(axis=0), axis=0) >= 2) & (r.base != 0)))
    # FixStep1
    r.s1 = r.base.copy()
    r.s1[0] = 0
    r.s1[1] = 0
    for i in range(2, n):
        if r.base[i] == 0:
            continue
        ref = r.base[i - 1] * 2 - r.base[i - 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            if np.abs((r.base[i] - ref) / (ref + EPS)) > 0.008 and \
                    np.abs((r.base[i] - r.base[i - 1]) / (r.base[i - 1] + EPS)) > 0.008:
                r.s1[i] = 0
                count["step1_drop"] += 1
    # FixStep2
    r.s2 = r.s1.copy()
    bl = boundary_list(r.s1)
    for i in range(len(bl) // 2):
        if bl[2 * i + 1] - bl[2 * i] < 6:
            r.s2[bl[2 * i] : bl[2 * i + 1] + 1] = 0
            count["step2_removed"] += 1
    # FixStep3
    bl = boundary_list(r.s2)
    r.sections, r.means = [], []
    kept_ch, kept_rng = [], []
    for i in range(len(bl) // 2):
        st, ed = int(bl[2 * i]), int(bl[2 * i + 1])
        ch = np.zeros(n)
        ch[st : ed + 1] = r.s2[st : ed + 1]
        lim1 = min(n - 2, ed + 100)
        lim0 = max(1, st - 100)
        count["fwd_clamped"] += int(lim1 == n - 2 and lim1 < ed + 100)
        count["bwd_clamped"] += int(lim0 == 1 and lim0 > st - 100)
        ext, r1 = extend(ch, ed, lim1, 1, cands, 0.18, count, "fwd")
        seq, r0 = extend(ext, st, lim0, -1, cands, 0.18, count, "bwd")
        mean = np.mean(seq[r0 : r1 + 1])
        kept = bool(2200 / mean < r1 - r0)
        r.sections.append((st, ed, r0, r1, int(kept)))
        r.means.append(float(mean))
        count["sec_total"] += 1
        if kept:
            kept_ch.append(seq)
            kept_rng.append((r0, r1))
        else:
            count["sec_not_kept"] += 1
    if kept_ch:
        r.s3 = merge(np.array(kept_ch), np.array(kept_rng, dtype=np.float64), cands, scores, count)
    else:
        r.s3 = r.s2.copy()
        if r.sections:
            count["no_section_kept"] += 1
    # FixStep4
    r.s4 = r.s3.copy()
    bl = boundary_list(r.s3)
    for i in range(1, len(bl) // 2):
        dist = bl[2 * i] - bl[2 * i - 1] - 1
        if dist >= 9:
            count["step4_left"] += 1
            continue
        count["step4_bridged"] += 1
        t0 = r.s3[bl[2 * i - 1]] + 1
        t1 = r.s3[bl[2 * i]] - 1
        c = (t1 - t0) / (dist + 1)
        k = 1
        for j in range(bl[2 * i - 1] + 1, bl[2 * i]):
            r.s4[j] = t0 + c * k
            k += 1
    r.vuv = (r.s4 != 0).astype(np.float64)
    return r


def smooth(f0, count=None, dtype=np.float64):
    """SmoothF0 / FilterF0, harvest.py:533-559.  dtype np.longdouble: the same recurrence (direct form II transposed, what
    scipy.signal.lfilter runs) carried out in extended precision — the yardstick for the rounding noise of the float64 one."""
    pad = 300
    buf = np.concatenate([np.zeros(pad), np.asarray(f0, dtype=np.float64), np.zeros(pad)])
    out = buf.astype(dtype)
    bl = boundary_list(buf)
    for i in range(len(bl) // 2):
        st, ed = int(bl[2 * i]), int(bl[2 * i + 1])
        ch = np.zeros(len(buf))
        ch[st : ed + 1] = buf[st : ed + 1]
        ch[:st] = ch[st]
        ch[ed + 1 :] = ch[ed]
        if dtype is np.float64:
            fwd = signal.lfilter(SMOOTH_B, SMOOTH_A, ch)
            bwd = signal.lfilter(SMOOTH_B, SMOOTH_A, fwd[::-1])[::-1]
        else:
            bwd = _lfilter_ld(_lfilter_ld(ch.astype(dtype))[::-1])[::-1]
        out[st : ed + 1] = bwd[st : ed + 1]
        if count is not None:
            count["smooth_runs"] += 1
    return out[pad : len(out) - pad]


def _lfilter_ld(x):
    b = SMOOTH_B.astype(np.longdouble)
    a = SMOOTH_A.astype(np.longdouble)
    y = np.empty(len(x), dtype=np.longdouble)
    z0 = z1 = np.longdouble(0)
    for i in range(len(x)):
        xi = x[i]
        yi = z0 + b[0] * xi
        z0 = z1 + b[1] * xi - a[1] * yi
        z1 = b[2] * xi - a[2] * yi
        y[i] = yi
    return y


def pick_index(tp, n):
    """harvest.py:48-49: the 1 ms row an output frame at time tp (seconds) reads."""
    v = np.asarray(tp, dtype=np.float64) * 1000
    r = np.where(v > 0, v + 0.5, v - 0.5)
    return np.minimum(float(n - 1), r).astype(np.int64)


def run(cands, scores):
    """Everything, stage by stage -> Result(pruned_c, pruned_s, base, s1, s2, s3, s4, vuv, sections, means, smoothed,
    count)."""
    count = collections.Counter()
    pc, ps = prune(cands, scores, count)
    r = fix_contour(pc, ps, count)
    r.pruned_c, r.pruned_s = pc, ps
    r.smoothed = smooth(r.s4, count)
    r.count = count
    return r
