"""Inputs, runner and comparison shared by tests/test_hip_dtw.py and tests/_dtw_bounds_script.py: seeded feature rows,
the reference result of every pair (tests/_dtw_reference.py, computed once per process and kept), wh_dtw through
world.align.align_device, and a bit-for-bit comparison of everything the call returns."""
import collections
import functools

import numpy as np

import _dtw_reference as ref

Case = collections.namedtuple("Case", "name shapes d seed kind radius pad max_ws")
Case.__new__.__defaults__ = (0, "normal", None, 0, None)


def edge_sizes():
    """1, 2, 3, 63, 64, 65 (lanes and the wave) and every tile constant of the kernel -1, +0, +1 and 2x +1."""
    from world import align

    s = {1, 2, 3, 63, 64, 65}
    for t in (align.ROWS_PER_LANE, align.CHUNK_COLS, align.STRIP_ROWS):
        s |= {t - 1, t, t + 1, 2 * t + 1}
    return sorted(v for v in s if v >= 1)


@functools.lru_cache(maxsize=None)
def features(n, d, seed, kind):
    rng = np.random.RandomState((seed * 7919 + n * 31 + d) % (2 ** 31))
    x = rng.randn(n, d) if kind == "normal" else rng.randint(0, 2, size=(n, d)).astype(np.float64)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(n, m, d, seed, kind, radius):
    return ref.dtw(features(n, d, seed, kind), features(m, d, seed + 1, kind), radius)


@functools.lru_cache(maxsize=None)
def kernel_cases():
    s = edge_sizes()
    long_n, long_m = 2 * 128 + 1, 65
    cases = [Case("every N x every M, d=39", tuple((n, m) for n in s for m in s), 39)]
    for d in (1, 2, 24, 64):
        cases.append(Case("d=%d" % d, tuple((n, long_m) for n in s) + tuple((long_n, m) for m in s), d, seed=d))
    cases.append(Case("N=1 / M=1 against long", ((1, 300), (300, 1), (1, 1), (1, 33), (129, 1)), 39, seed=3))
    cases.append(Case("ties", ((129, 70), (257, 97), (64, 64), (130, 33), (65, 257), (3, 5)), 1, seed=4, kind="ties"))
    cases.append(Case("ties d=2", ((129, 70), (257, 97), (33, 130)), 2, seed=5, kind="ties"))
    band_shapes = ((65, 129), (129, 65), (1, 40), (40, 1), (257, 100), (33, 200), (2, 2), (3, 64), (300, 290))
    for radius in (1, 2, 17):
        cases.append(Case("band radius=%d" % radius, band_shapes, 5, seed=6, radius=radius))
    cases.append(Case("lda / ldb > d", ((70, 50), (129, 33), (2, 3)), 39, seed=7, pad=3))
    return tuple(cases)


RAGGED = Case("ragged batch", ((200, 150), (1, 7), (129, 257), (64, 2), (33, 33), (3, 300), (131, 66)), 24, seed=8)


def run(rt, case, only=None):
    """align_device on the case's pairs (``only``: that pair alone, as a batch of one), want_acc on."""
    from world.align import DEFAULT_MAX_WORKSPACE_BYTES, align_device

    shapes = case.shapes if only is None else (case.shapes[only],)
    a = [features(n, case.d, case.seed, case.kind) for n, _ in shapes]
    b = [features(m, case.d, case.seed + 1, case.kind) for _, m in shapes]

    def side(parts):
        x = np.concatenate(parts)
        off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
        if case.pad:  # rows inside a wider tensor; what lies beside them must never be read
            wide = np.full((x.shape[0], case.d + case.pad), np.nan)
            wide[:, 1:1 + case.d] = x
            x_d = rt.to_device(wide)[:, 1:1 + case.d]
        else:
            x_d = rt.to_device(x)
        return rt.make_batch(np.zeros(len(parts) + 1, dtype=np.int64), off), x_d

    ba, xa = side(a)
    bb, xb = side(b)
    return align_device(rt, ba, xa, bb, xb, radius=case.radius, want_acc=True,
                        max_workspace_bytes=case.max_ws or DEFAULT_MAX_WORKSPACE_BYTES)


def download(al):
    """Everything an Alignment holds, as host arrays per pair with pair-local indices."""
    pa, pb = al.path_a.cpu().numpy(), al.path_b.cpu().numpy()
    ln, cost = al.path_len.cpu().numpy(), al.cost.cpu().numpy()
    a2b, b2a, acc = al.map_a2b.cpu().numpy(), al.map_b2a.cpu().numpy(), al.acc.cpu().numpy()
    foa, fob = al.batch_a.frame_off, al.batch_b.frame_off
    out = []
    for u in range(al.n_utt):
        o, n, m = int(al.path_off_host[u]), int(foa[u + 1] - foa[u]), int(fob[u + 1] - fob[u])
        out.append({"path_a": pa[o:o + ln[u]] - foa[u], "path_b": pb[o:o + ln[u]] - fob[u], "length": int(ln[u]),
                    "cost": cost[u], "map_a2b": a2b[foa[u]:foa[u + 1]] - fob[u], "map_b2a": b2a[fob[u]:fob[u + 1]] - foa[u],
                    "acc": acc[al.acc_off_host[u]:al.acc_off_host[u + 1]].reshape(n, m)})
    return out


KEYS = ("acc", "length", "path_a", "path_b", "cost", "map_a2b", "map_b2a")


def same_bits(x, y):
    kind = np.float64 if "f" in (np.asarray(x).dtype.kind, np.asarray(y).dtype.kind) else np.int64
    x, y = np.ascontiguousarray(x, dtype=kind), np.ascontiguousarray(y, dtype=kind)
    return x.shape == y.shape and x.tobytes() == y.tobytes()


def compare(al, case, only=None):
    """[] when every pair of the alignment equals the reference bit for bit, else 'pair (n, m): key' strings."""
    shapes = case.shapes if only is None else (case.shapes[only],)
    bad = []
    for (n, m), got in zip(shapes, download(al)):
        want = reference(n, m, case.d, case.seed, case.kind, case.radius)
        for key in KEYS:
            if not same_bits(np.ascontiguousarray(got[key]), want[key]):
                bad.append("pair (%d, %d): %s" % (n, m, key))
    return bad
