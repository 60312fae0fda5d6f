"""The arithmetic contract of wh_dtw (include/world_hip.h) in NumPy and plain Python: what the
device must reproduce bit for bit.  The local cost is a loop over the columns, vectorised over the cells (a sequential,
unfused sum from 0.0 and np.sqrt, which is correctly rounded); the recurrence runs over Python lists of floats (IEEE
doubles); the band is evaluated in int64."""
import numpy as np

MCD_SCALE = (10.0 / np.log(10.0)) * np.sqrt(2.0)


def local_cost(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    s = np.zeros((a.shape[0], b.shape[0]))
    for k in range(a.shape[1]):
        e = a[:, k][:, None] - b[:, k][None, :]
        s = s + e * e
    return np.sqrt(s)


def in_band(n, m, radius):
    """[n][m] bool: |j (n-1) - i (m-1)| <= radius max(n-1, m-1); radius None: everything."""
    if radius is None:
        return np.ones((n, m), dtype=bool)
    i = np.arange(n, dtype=np.int64)[:, None]
    j = np.arange(m, dtype=np.int64)[None, :]
    return np.abs(j * np.int64(n - 1) - i * np.int64(m - 1)) <= np.int64(radius) * np.int64(max(n - 1, m - 1))


def accumulate(cost, band):
    """(D, back-pointers) as lists of lists: code 0 diagonal, 1 (i-1, j), 2 (i, j-1), -1 at (0, 0).  The predecessors
    that exist are tried in that order and a later one wins only by strict <."""
    n, m = len(cost), len(cost[0])
    inf = float("inf")
    D = [[inf] * m for _ in range(n)]
    B = [[-1] * m for _ in range(n)]
    for i in range(n):
        ci, bi, Di, Bi = cost[i], band[i], D[i], B[i]
        Dp = D[i - 1] if i else None
        for j in range(m):
            if i == 0 and j == 0:
                Di[0] = ci[0]
                continue
            best, code = None, -1
            if i and j:
                best, code = Dp[j - 1], 0
            if i and (best is None or Dp[j] < best):
                best, code = Dp[j], 1
            if j and (best is None or Di[j - 1] < best):
                best, code = Di[j - 1], 2
            Bi[j] = code
            if bi[j]:
                Di[j] = ci[j] + best
    return D, B


def backtrack(B):
    n, m = len(B), len(B[0])
    i, j = n - 1, m - 1
    pa, pb = [i], [j]
    while i or j:
        code = B[i][j]
        if code != 2:
            i -= 1
        if code != 1:
            j -= 1
        pa.append(i)
        pb.append(j)
    return np.array(pa[::-1], dtype=np.int64), np.array(pb[::-1], dtype=np.int64)


def maps(path_a, path_b, n, m):
    """map_a2b[i] = (j_lo + j_hi) // 2 over the path cells sharing i; map_b2a[j] likewise over those sharing j."""
    a2b, b2a = np.zeros(n, dtype=np.int64), np.zeros(m, dtype=np.int64)
    for i in range(n):
        js = path_b[path_a == i]
        a2b[i] = (int(js.min()) + int(js.max())) // 2
    for j in range(m):
        is_ = path_a[path_b == j]
        b2a[j] = (int(is_.min()) + int(is_.max())) // 2
    return a2b, b2a


def dtw(a, b, radius=None):
    """One pair: dict with acc [n][m], path_a, path_b (local indices, forward order), length, cost = D(n-1, m-1),
    mean = cost / length, mcd = MCD_SCALE * mean, map_a2b, map_b2a."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n, m = a.shape[0], b.shape[0]
    D, B = accumulate(local_cost(a, b).tolist(), in_band(n, m, radius).tolist())
    pa, pb = backtrack(B)
    a2b, b2a = maps(pa, pb, n, m)
    cost = np.float64(D[-1][-1])
    mean = cost / np.float64(len(pa))
    return {"acc": np.array(D, dtype=np.float64), "path_a": pa, "path_b": pb, "length": len(pa), "cost": cost,
            "mean": mean, "mcd": np.float64(MCD_SCALE) * mean, "map_a2b": a2b, "map_b2a": b2a}


def well_formed(pa, pb, n, m):
    """The path starts at (0, 0), ends at (n-1, m-1) and every step is one of the three moves."""
    if len(pa) != len(pb) or len(pa) == 0 or (pa[0], pb[0]) != (0, 0) or (pa[-1], pb[-1]) != (n - 1, m - 1):
        return False
    da, db = np.diff(pa), np.diff(pb)
    return bool(np.all((da >= 0) & (da <= 1) & (db >= 0) & (db <= 1) & (da + db >= 1)))
