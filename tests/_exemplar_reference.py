"""The contract of wh_knn and wh_frame_select (include/world_hip.h) in NumPy: what the device
reproduces bit for bit.  The vector forms below loop over the COLUMN and run NumPy operations over all pairs, so every
difference, product and sum is one IEEE operation rounded on its own, in the contract's order;
tests/test_exemplar_reference_host.py holds them against scalar loops of the same contract.

    knn(q, db, k, excl_lo, excl_hi)            -> idx [n][k] int32, dist [n][k]
    frame_select(frame_off, idx, tc, y, succ, weight) -> sel, slot (int32 [frames]), total [n_utt], acc [frames][k]
"""
import numpy as np

MAX_D, MAX_K, MAX_DY = 160, 32, 64


def sqdist(q, db):
    """s[n][r] = sum over c ascending, from +0.0, of (q[n][c] - db[r][c]) * (q[n][c] - db[r][c])."""
    q, db = np.asarray(q, dtype=np.float64), np.asarray(db, dtype=np.float64)
    s = np.zeros((q.shape[0], db.shape[0]))
    with np.errstate(all="ignore"):
        for c in range(q.shape[1]):
            e = q[:, c, None] - db[None, :, c]
            s = s + e * e
    return s


def knn(q, db, k, excl_lo=None, excl_hi=None):
    """The k candidates smallest under (key ascending, row ascending), key = s or +inf where s is NaN; rows with
    excl_lo[n] <= r < excl_hi[n] are no candidates; slots beyond the candidates hold -1 / +inf."""
    q, db = np.asarray(q, dtype=np.float64), np.asarray(db, dtype=np.float64)
    n, r = q.shape[0], db.shape[0]
    idx = np.full((n, k), -1, dtype=np.int32)
    dist = np.full((n, k), np.inf)
    if n == 0 or r == 0:
        return idx, dist
    s = sqdist(q, db)
    key = np.where(np.isnan(s), np.inf, s)
    rows = np.broadcast_to(np.arange(r, dtype=np.int64), (n, r))
    out = np.zeros((n, r), dtype=bool)
    if excl_lo is not None:
        lo, hi = np.asarray(excl_lo, dtype=np.int64)[:, None], np.asarray(excl_hi, dtype=np.int64)[:, None]
        out = (rows >= lo) & (rows < hi)
    order = np.lexsort((rows, key, out), axis=1)  # the excluded behind everything, then key, then row
    count = r - out.sum(axis=1)
    m = min(k, r)
    take = order[:, :m]
    have = np.arange(m)[None, :] < count[:, None]
    idx[:, :m] = np.where(have, take, -1)
    dist[:, :m] = np.where(have, np.take_along_axis(key, take, axis=1), np.inf)
    return idx, dist


def frame_select(frame_off, idx, tc, y, succ, weight):
    """Viterbi over every utterance's frames; see the header.  Returns sel, slot, total, acc."""
    frame_off = np.asarray(frame_off, dtype=np.int64)
    idx, tc = np.asarray(idx, dtype=np.int64), np.asarray(tc, dtype=np.float64)
    y, succ = np.asarray(y, dtype=np.float64), np.asarray(succ, dtype=np.int64)
    frames, k = idx.shape
    n_db = y.shape[0]
    weight = np.float64(weight)
    sel, slot = np.zeros(frames, dtype=np.int32), np.zeros(frames, dtype=np.int32)
    total = np.zeros(len(frame_off) - 1)
    acc = np.zeros((frames, k))
    valid = (idx >= 0) & (idx < n_db)
    safe = np.where(valid, idx, 0)
    nxt_row = succ[safe] if n_db else np.zeros_like(safe)
    nxt_ok = valid & (nxt_row >= 0) & (nxt_row < n_db)
    nxt_row = np.where(nxt_ok, nxt_row, 0)

    def first_min(v):  # over axis 0: v[0], replaced by a later entry only where that is strictly smaller
        best, at = v[0].copy(), np.zeros(v.shape[1:], dtype=np.int64)
        for j in range(1, v.shape[0]):
            m = v[j] < best
            best, at = np.where(m, v[j], best), np.where(m, j, at)
        return best, at

    with np.errstate(all="ignore"):
        for u in range(len(frame_off) - 1):
            f0, f1 = int(frame_off[u]), int(frame_off[u + 1])
            if f1 <= f0:
                continue
            bp = np.zeros((f1 - f0, k), dtype=np.int64)
            a = np.where(valid[f0], tc[f0], np.inf)
            acc[f0] = a
            for t in range(f0 + 1, f1):
                cur = y[safe[t]] if n_db else np.zeros((k, 1))        # [k][dy]
                nxt = y[nxt_row[t - 1]] if n_db else np.zeros((k, 1))  # [j][dy]
                cc = np.zeros((k, k))                                  # [j][k]
                for c in range(cur.shape[1]):
                    e = cur[None, :, c] - nxt[:, None, c]
                    cc = cc + e * e
                v = a[:, None] + weight * cc
                v[~nxt_ok[t - 1], :] = np.inf
                v[:, ~valid[t]] = np.inf
                best, at = first_min(v)
                a = np.where(valid[t], tc[t] + best, np.inf)
                bp[t - f0] = np.where(valid[t], at, 0)
                acc[t] = a
            best, at = first_min(a[:, None])
            total[u] = best[0]
            ks = int(at[0])
            for t in range(f1 - 1, f0 - 1, -1):
                slot[t] = ks
                sel[t] = idx[t, ks]
                ks = int(bp[t - f0, ks])
    return sel, slot, total, acc


def chain_succ(utt_off):
    """succ[r] = r + 1 inside an utterance, r at its last frame."""
    utt_off = np.asarray(utt_off, dtype=np.int64)
    succ = np.arange(1, int(utt_off[-1]) + 1, dtype=np.int32)
    last = utt_off[1:][np.diff(utt_off) > 0] - 1
    succ[last] = last
    return succ
