"""tests/_exemplar_reference.py against itself (no GPU): its vector forms equal scalar loops of the same contract bit
for bit, its Viterbi total equals exhaustive enumeration on integer data, every mutant of the contract is told apart by
bits or by indices, and the properties that follow from the contract hold."""
import fractions
import itertools

import numpy as np
import pytest

import _exemplar_reference as xref

INF = float("inf")


# ---- scalar loops of the contract; ``mutant`` names one deliberate departure --------------------------------------------
def sq_scalar(a, b, mutant=None):
    terms = []
    s = 0.0
    with np.errstate(all="ignore"):
        for c in range(len(a)):
            e = np.float64(a[c]) - np.float64(b[c])
            if mutant == "fused" and np.isfinite(e) and np.isfinite(s):
                s = np.float64(float(fractions.Fraction(float(s)) + fractions.Fraction(float(e)) ** 2))
            else:
                s = s + e * e
            terms.append(e * e)
        if mutant == "pairwise":
            while len(terms) > 1:
                terms = [terms[i] + terms[i + 1] if i + 1 < len(terms) else terms[i] for i in range(0, len(terms), 2)]
            s = terms[0] if terms else 0.0
    return np.float64(s)


def knn_scalar(q, db, k, lo=None, hi=None, mutant=None):
    idx, dist = np.full((len(q), k), -1, dtype=np.int32), np.full((len(q), k), INF)
    for n in range(len(q)):
        cand = []
        for r in range(len(db)):
            if lo is not None and lo[n] <= r < hi[n]:
                continue
            s = sq_scalar(q[n], db[r], mutant)
            key = (-INF if mutant == "nan_first" else INF) if s != s else float(s)
            cand.append((key, -r if mutant == "ties_up" else r, r))
        cand.sort(key=lambda t: t[:2])
        for j, (key, _, r) in enumerate(cand[:k]):
            idx[n, j], dist[n, j] = r, key
    return idx, dist


def select_scalar(frame_off, idx, tc, y, succ, weight, mutant=None):
    frames, k = idx.shape
    n_db = len(y)
    sel, slot = np.zeros(frames, dtype=np.int32), np.zeros(frames, dtype=np.int32)
    total, acc = np.zeros(len(frame_off) - 1), np.zeros((frames, k))
    ok = lambda i: mutant == "read_invalid" or 0 <= i < n_db  # noqa: E731
    with np.errstate(all="ignore"):
        for u in range(len(frame_off) - 1):
            f0, f1 = int(frame_off[u]), int(frame_off[u + 1])
            if f1 <= f0:
                continue
            bp = np.zeros((f1 - f0, k), dtype=int)
            a = [np.float64(tc[f0, j]) if ok(idx[f0, j]) else INF for j in range(k)]
            acc[f0] = a
            for t in range(f0 + 1, f1):
                new = []
                for kk in range(k):
                    if not ok(idx[t, kk]):
                        new.append(INF)
                        continue
                    best, at = None, 0
                    for j in range(k):
                        v = INF
                        if ok(idx[t - 1, j]):
                            s = idx[t - 1, j] if mutant == "no_succ" else succ[idx[t - 1, j] % n_db]
                            if ok(s):
                                v = a[j] + np.float64(weight) * sq_scalar(y[idx[t, kk] % n_db], y[s % n_db])
                        if j == 0 or v < best:
                            best, at = v, j
                    new.append(np.float64(tc[t, kk]) + best)
                    bp[t - f0, kk] = at
                a = new
                acc[t] = a
            ks = 0
            for kk in range(1, k):
                if a[kk] < a[ks] or (mutant == "end_up" and a[kk] == a[ks]):
                    ks = kk
            total[u] = a[ks]
            for t in range(f1 - 1, f0 - 1, -1):
                slot[t], sel[t] = ks, idx[t, ks]
                ks = bp[t - f0, ks]
    return sel, slot, total, acc


def bits(a):
    a = np.asarray(a, dtype=np.float64)
    return np.where(np.isnan(a), np.uint64(0x7ff8000000000000), a.view(np.uint64) if a.flags.c_contiguous else np.ascontiguousarray(a).view(np.uint64))


def tiny_knn(seed, kind):
    rng = np.random.RandomState(seed)
    n, r, d = rng.randint(1, 6), rng.randint(1, 9), rng.randint(1, 6)
    if kind == "noise":
        q, db = rng.randn(n, d) * 1e3, rng.randn(r, d) * 1e-3
    else:
        q, db = rng.randint(-2, 3, (n, d)).astype(float), rng.randint(-2, 3, (r, d)).astype(float)
        if kind == "duplicates" and r > 2:
            db[r // 2] = db[0]
            db[-1] = db[0]
    return q, db


def tiny_select(seed, integer=True, k_max=3):
    rng = np.random.RandomState(seed)
    r, k, dy = rng.randint(2, 7), rng.randint(1, k_max + 1), rng.randint(1, 4)
    frames = [int(v) for v in rng.randint(0, 6, size=rng.randint(1, 4))]
    fo = np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)
    f = int(fo[-1])
    y = rng.randint(-2, 3, (r, dy)).astype(float) if integer else rng.randn(r, dy)
    tc = rng.randint(0, 4, (f, k)).astype(float) if integer else rng.rand(f, k)
    idx = rng.randint(0, r, (f, k)).astype(np.int32)
    succ = np.minimum(np.arange(1, r + 1), r - 1).astype(np.int32)
    return fo, idx, tc, y, succ


@pytest.mark.parametrize("kind", ["noise", "integers", "duplicates"])
def test_knn_vector_form_equals_scalar_loops(kind):
    for seed in range(25):
        q, db = tiny_knn(seed, kind)
        k = 1 + seed % 5
        lo = hi = None
        if seed % 3 == 0:
            lo = np.random.RandomState(seed).randint(0, len(db) + 1, len(q))
            hi = lo + seed % 4
        gi, gd = xref.knn(q, db, k, lo, hi)
        wi, wd = knn_scalar(q, db, k, lo, hi)
        assert np.array_equal(gi, wi) and np.array_equal(bits(gd), bits(wd)), (kind, seed)


def test_knn_non_finite_rows_are_listed_last_by_index():
    rng = np.random.RandomState(3)
    q, db = rng.randn(3, 4), rng.randn(7, 4)
    db[1, 2], db[4, 0] = np.nan, np.inf
    gi, gd = xref.knn(q, db, 7)
    wi, wd = knn_scalar(q, db, 7)
    assert np.array_equal(gi, wi) and np.array_equal(bits(gd), bits(wd))
    assert np.all(gi[:, -2:] == [1, 4]) and np.all(np.isinf(gd[:, -2:]))


def test_select_vector_form_equals_scalar_loops():
    for seed in range(40):
        fo, idx, tc, y, succ = tiny_select(seed, integer=seed % 2 == 0, k_max=4)
        if seed % 4 == 1:  # invalid slots, slot 0 kept
            idx[:, 1:][np.random.RandomState(seed).rand(*idx[:, 1:].shape) < 0.4] = -1
        if seed % 4 == 3:
            succ[0] = len(y) + 3
        w = (0.0, 0.5, 1.0, 3.0)[seed % 4]
        got, want = xref.frame_select(fo, idx, tc, y, succ, w), select_scalar(fo, idx, tc, y, succ, w)
        for g, wv, name in zip(got, want, ("sel", "slot", "total", "acc")):
            assert np.array_equal(bits(g), bits(wv)) if g.dtype == np.float64 else np.array_equal(g, wv), (seed, name)


def test_viterbi_total_equals_exhaustive_search():
    """Integer data: every sum is exact, so the cheapest of all K^F slot sequences is the Viterbi total."""
    done = 0
    for seed in range(200):
        fo, idx, tc, y, succ = tiny_select(seed)
        _, slot, total, _ = xref.frame_select(fo, idx, tc, y, succ, 1.0)
        k = idx.shape[1]
        for u in range(len(fo) - 1):
            f0, f1 = int(fo[u]), int(fo[u + 1])
            if f1 == f0:
                assert total[u] == 0.0
                continue
            best = INF
            for seq in itertools.product(range(k), repeat=f1 - f0):
                c = sum(tc[f0 + t, s] for t, s in enumerate(seq))
                c += sum(np.sum((y[idx[f0 + t, seq[t]]] - y[succ[idx[f0 + t - 1, seq[t - 1]]]]) ** 2) for t in range(1, f1 - f0))
                best = min(best, c)
            assert total[u] == best, (seed, u)
            done += 1
    assert done > 200


MUTANTS_KNN = ("pairwise", "fused", "ties_up", "nan_first")
MUTANTS_SELECT = ("no_succ", "end_up", "read_invalid")


@pytest.mark.parametrize("mutant", MUTANTS_KNN)
def test_knn_mutants_are_told_apart(mutant):
    told = 0
    for seed in range(30):
        q, db = tiny_knn(seed, "duplicates" if mutant == "ties_up" else "noise")
        if mutant in ("pairwise", "fused"):  # wide rows of mixed magnitude: the order and the fusing of the sum show in its last bits
            rng = np.random.RandomState(seed)
            q, db = rng.randn(4, 9) * 10.0 ** rng.randint(-3, 4, 9), rng.randn(6, 9)
        if mutant == "nan_first":
            db[0, 0] = np.nan
        k = min(3, len(db))
        gi, gd = xref.knn(q, db, k)
        mi, md = knn_scalar(q, db, k, mutant=mutant)
        told += not (np.array_equal(gi, mi) and np.array_equal(bits(gd), bits(md)))
    assert told >= 10, (mutant, told)


@pytest.mark.parametrize("mutant", MUTANTS_SELECT)
def test_select_mutants_are_told_apart(mutant):
    told = 0
    for seed in range(60):
        fo, idx, tc, y, succ = tiny_select(seed, k_max=4)
        if mutant == "read_invalid":
            idx[:, 1:][np.random.RandomState(seed).rand(*idx[:, 1:].shape) < 0.5] = -1
        if mutant == "end_up":
            tc[:] = 0.0
            y[:] = 0.0  # every path costs nothing: the end is slot 0 unless the tie is broken upwards
        got, mut = xref.frame_select(fo, idx, tc, y, succ, 1.0), select_scalar(fo, idx, tc, y, succ, 1.0, mutant)
        told += not all(np.array_equal(bits(g), bits(m)) if g.dtype == np.float64 else np.array_equal(g, m) for g, m in zip(got, mut))
    assert told >= 10, (mutant, told)


# ---- what follows from the contract -------------------------------------------------------------------------------------
def _own_rows(exclude):
    rng = np.random.RandomState(11)
    r, k, d = 300, 8, 5
    x, y = rng.randn(r, d), rng.randn(r, 4)
    utt_off = np.array([0, 100, 101, 300])
    succ = xref.chain_succ(utt_off)
    out = []
    for u in range(3):
        f0, f1 = int(utt_off[u]), int(utt_off[u + 1])
        lo = np.full(f1 - f0, f0 if exclude else 0)
        hi = np.full(f1 - f0, f1 if exclude else 0)
        idx, dist = xref.knn(x[f0:f1], x, k, lo, hi)
        out.append((f0, f1, idx, dist, xref.frame_select([0, f1 - f0], idx, dist, y, succ, 0.7)))
    return out


def test_an_utterance_of_the_database_selects_itself():
    for f0, f1, idx, dist, (sel, slot, total, _) in _own_rows(False):
        assert np.array_equal(sel, np.arange(f0, f1)) and not slot.any() and total[0] == 0.0


def test_an_excluded_utterance_is_never_selected():
    for f0, f1, idx, dist, (sel, _, total, _) in _own_rows(True):
        assert not np.any((idx >= f0) & (idx < f1)) and not np.any((sel >= f0) & (sel < f1)) and total[0] > 0.0


def test_weight_zero_selects_the_nearest():
    rng = np.random.RandomState(5)
    x, y = rng.randn(80, 3), rng.randn(80, 2)
    idx, dist = xref.knn(rng.randn(30, 3), x, 6)
    sel, slot, _, _ = xref.frame_select([0, 12, 30], idx, dist, y, xref.chain_succ([0, 80]), 0.0)
    assert np.array_equal(sel, idx[:, 0]) and not slot.any()


def test_chain_succ():
    assert xref.chain_succ([0, 3, 3, 4, 6]).tolist() == [1, 2, 2, 3, 5, 5]
