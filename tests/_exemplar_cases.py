"""Inputs, runners and references shared by tests/test_hip_exemplar.py and tests/_exemplar_bounds_script.py: the case
lists of wh_knn and wh_frame_select at the smallest shapes that reach every edge, the reference result of every case
(tests/_exemplar_reference.py, computed once per process and kept read-only) and the C entries called directly, the
outputs between guard values that must survive.

wh_knn cases: counts around the kernel's tiles (TILE_Q queries, TILE_R database rows, STRIP columns: restated from
world/exemplar.py, which tests/test_exemplar_host.py holds against csrc/wh_exemplar.hip), every K, strides wider than d,
integer rows drawn from a handful of vectors (exact ties across tile and split edges), non-finite rows, exclusions.
wh_frame_select cases: frame counts around the walk back's piece (CHUNK), every K and dy edge, ragged batches, ties,
invalid slots, the weights, non-finite rows of y that one utterance alone can reach."""
import collections
import functools

import numpy as np

import _exemplar_reference as xref

TILE_Q, TILE_R, STRIP, CHUNK = 64, 64, 16, 256  # world.exemplar.TILE_Q, TILE_R, STRIP, CHUNK

KnnCase = collections.namedtuple("KnnCase", "name n_q n_db d k pad data excl seed")
SelCase = collections.namedtuple("SelCase", "name frames k dy pad n_db data succ weight invalid seed")


def _frozen(a):
    a.setflags(write=False)
    return a


# ---- wh_knn -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def knn_cases():
    edge = (1, TILE_Q - 1, TILE_Q, TILE_Q + 1)
    cases = [KnnCase("n_q=%d n_db=%d" % (nq, nr), nq, nr, 7, 3, 0, "noise", None, 10 + i)
             for i, (nq, nr) in enumerate((a, b) for a in edge for b in edge)]
    cases += [KnnCase("three tiles each way", 2 * TILE_Q + 3, 3 * TILE_R - 1, 9, 5, 0, "noise", None, 40)]
    cases += [KnnCase("d=%d" % d, 70, 130, d, 5, 0, "noise", None, 50 + d)
              for d in (1, 2, 7, 8, 9, STRIP - 1, STRIP, STRIP + 1, 39, 78, 80, 159, 160)]
    cases += [KnnCase("K=%d" % k, 66, 150, 5, k, 0, "noise", None, 300 + k) for k in (1, 2, 15, 16, 31, 32)]
    cases += [KnnCase("K=8 > n_db=3", 5, 3, 4, 8, 0, "noise", None, 340),
              KnnCase("K=32 > n_db=31", 65, 31, 4, 32, 0, "int", None, 341),
              KnnCase("column slice", 67, 131, 39, 16, 5, "noise", None, 342),
              KnnCase("integer ties", 70, 200, 3, 16, 0, "int", None, 343),
              KnnCase("integer ties K=32 d=1", 65, 200, 1, 32, 2, "int", None, 344),
              KnnCase("NaN and Inf rows in the database, all listed", 9, 30, 6, 32, 0, "nonfinite_db", None, 345),
              KnnCase("NaN and Inf rows in the database", 66, 130, 6, 16, 0, "nonfinite_db", None, 346),
              KnnCase("NaN and Inf rows in the queries", 66, 130, 6, 8, 0, "nonfinite_q", None, 347),
              KnnCase("exclusions", 70, 140, 5, 8, 0, "noise", "mixed", 348),
              KnnCase("exclusions with ties", 70, 140, 2, 16, 1, "int", "mixed", 349)]
    return tuple(cases)


SPLIT_CASES = ("integer ties", "three tiles each way", "exclusions with ties", "NaN and Inf rows in the database")


def knn_splits(case):
    return (0, 1, 2, 7, case.n_db)


@functools.lru_cache(maxsize=None)
def knn_inputs(case):
    """{q, db: padded 2-D arrays whose first d columns count, lo, hi: int32 or None}."""
    rng = np.random.RandomState(7000 + case.seed)
    w = case.d + case.pad
    if case.data == "int":  # a handful of distinct vectors: many keys tie exactly, across every tile and split edge
        pool = rng.randint(-2, 3, size=(6, w)).astype(np.float64)
        db = pool[rng.randint(0, 6, size=case.n_db)]
        q = pool[rng.randint(0, 6, size=case.n_q)] + rng.randint(0, 2, size=(case.n_q, w))
    else:
        db, q = rng.randn(case.n_db, w), rng.randn(case.n_q, w)
    if case.data == "nonfinite_db":
        db[min(5, case.n_db - 1), case.d // 2] = np.nan
        db[case.n_db // 2, 0] = np.inf
        db[case.n_db - 1, case.d - 1] = -np.inf
    if case.data == "nonfinite_q":
        q[3, 1] = np.nan
        q[TILE_Q, 0] = np.inf
    lo = hi = None
    if case.excl == "mixed":
        n, r = case.n_q, case.n_db
        lo, hi = rng.randint(0, r, size=n).astype(np.int32), np.zeros(n, dtype=np.int32)
        hi[:] = np.minimum(lo + rng.randint(0, 40, size=n), r)
        lo[0], hi[0] = 5, 5            # empty
        lo[1], hi[1] = 9, 3            # empty the other way round
        lo[2], hi[2] = 0, r - 1        # everything but the last row
        lo[3], hi[3] = 1, r            # everything but the first
        lo[4], hi[4] = 0, 20           # the front end
        lo[5], hi[5] = r - 20, r       # the back end
        lo[6], hi[6] = 2, r - 2        # fewer than K are left
        lo[7], hi[7] = 0, r            # none is left
        lo[8], hi[8] = -7, TILE_R + 1  # from before the database to just behind a tile edge
        lo[9], hi[9] = r - 3, 2 ** 31 - 1
        lo, hi = _frozen(lo), _frozen(hi)
    return {"q": _frozen(q), "db": _frozen(db), "lo": lo, "hi": hi}


@functools.lru_cache(maxsize=None)
def knn_reference(case):
    inp = knn_inputs(case)
    idx, dist = xref.knn(inp["q"][:, :case.d], inp["db"][:, :case.d], case.k, inp["lo"], inp["hi"])
    return _frozen(idx), _frozen(dist)


I_GUARD, D_GUARD = -77777, -7.0


def knn_call(rt, q_d, n_q, ldq, db_d, n_db, lddb, d, k, lo_d, hi_d, splits, idx_d, dist_d):
    return rt.lib.wh_knn(rt.ctx, rt.stream(), rt.ptr(q_d), n_q, ldq, rt.ptr(db_d), n_db, lddb, d, k, rt.ptr(lo_d), rt.ptr(hi_d),
                         splits, rt.ptr(idx_d), rt.ptr(dist_d))


def knn_run(rt, case, splits=0, only=None, q=None):
    """wh_knn on a case -> {idx, dist, rc, guards}.  ``only``: that query alone.  ``q``: other queries than the case's."""
    torch = rt.torch
    inp = knn_inputs(case)
    q = inp["q"] if q is None else q
    lo, hi = inp["lo"], inp["hi"]
    if only is not None:
        q = q[only:only + 1]
        lo, hi = (None, None) if lo is None else (lo[only:only + 1], hi[only:only + 1])
    n = q.shape[0]
    q_d, db_d = rt.to_device(np.ascontiguousarray(q)), rt.to_device(np.ascontiguousarray(inp["db"]))
    lo_d = None if lo is None else rt.to_device(np.ascontiguousarray(lo), dtype=np.int32)
    hi_d = None if hi is None else rt.to_device(np.ascontiguousarray(hi), dtype=np.int32)
    idx_w = torch.full((n * case.k + 2,), I_GUARD, dtype=torch.int32, device=rt.device)
    dist_w = torch.full((n * case.k + 2,), D_GUARD, dtype=torch.float64, device=rt.device)
    w = case.d + case.pad
    rc = knn_call(rt, q_d, n, w, db_d, case.n_db, w, case.d, case.k, lo_d, hi_d, splits, idx_w[1:], dist_w[1:])
    idx_h, dist_h = idx_w.cpu().numpy(), dist_w.cpu().numpy()
    guards = bool(idx_h[0] == I_GUARD and idx_h[-1] == I_GUARD and dist_h[0] == D_GUARD and dist_h[-1] == D_GUARD)
    guards = guards and np.array_equal(db_d.cpu().numpy(), inp["db"], equal_nan=True)
    return {"idx": idx_h[1:-1].reshape(n, case.k).copy(), "dist": dist_h[1:-1].reshape(n, case.k).copy(), "rc": rc,
            "guards": guards}


def same_bits(a, b):
    """Bit for bit, but any NaN equals any NaN (its sign and payload are no part of the contract)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64)))


def knn_compare(case, got):
    if got["rc"] != 0:
        return ["rc %d" % got["rc"]]
    idx, dist = knn_reference(case)
    bad = []
    if got["idx"].tobytes() != idx.tobytes():
        rows = np.flatnonzero(np.any(got["idx"] != idx, axis=1))
        bad.append("idx differs in %d queries, the first %s: %s against %s" % (len(rows), rows[:1], got["idx"][rows[:1]], idx[rows[:1]]))
    if not same_bits(got["dist"], dist):
        bad.append("dist differs in %d slots" % np.count_nonzero(got["dist"] != dist))
    if not got["guards"]:
        bad.append("a guard value was written or the database changed")
    return bad


# ---- wh_frame_select ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sel_cases():
    ragged = (0, 3, 0, 0, 1, TILE_Q, 2, 0, TILE_Q + 1, 0)
    cases = [SelCase("frame counts", (0, 1, 2, 3, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 300), 5, 6, 2, 90, "noise", "chain", 1.0, None, 1),
             SelCase("ragged, empty first, last and in the middle", ragged, 7, 9, 1, 70, "noise", "chain", 0.5, None, 2)]
    cases += [SelCase("K=%d" % k, (40, 1, 17), k, 5, 1, 120, "noise", "chain", 1.0, None, 10 + k) for k in (1, 2, 31, 32)]
    cases += [SelCase("dy=%d" % dy, (33, 2, 9), 6, dy, 3, 80, "noise", "chain", 1.0, None, 50 + dy) for dy in (1, 7, 8, 9, 39, 40, 63, 64)]
    cases += [SelCase("K=32 dy=64", (20, 5), 32, 64, 1, 100, "noise", "chain", 1.0, None, 120),
              SelCase("integer ties", (50, 3, 31), 8, 3, 1, 60, "int", "chain", 1.0, None, 121),
              SelCase("integer ties, succ the identity", (50, 3, 31), 8, 3, 1, 60, "int", "identity", 1.0, None, 122),
              SelCase("integer ties K=32", (30, 12), 32, 2, 0, 40, "int", "chain", 0.5, None, 123),
              SelCase("invalid slots", (45, 1, 2, 30), 6, 5, 1, 50, "noise", "chain", 1.0, "some", 124),
              SelCase("only slot 0 valid in places", (45, 1, 2, 30), 6, 5, 1, 50, "int", "chain", 1.0, "rest", 125),
              SelCase("succ out of range in places", (45, 1, 2, 30), 6, 5, 1, 50, "noise", "broken", 1.0, None, 126),
              SelCase("NaN and Inf rows of y in utterance 1", (25, 25, 25), 6, 5, 1, 60, "nonfinite", "chain", 1.0, None, 127)]
    cases += [SelCase("weight=%g" % w, (30, 7), 9, 4, 1, 64, data, "chain", w, None, 130 + i)
              for i, (w, data) in enumerate(((0.0, "noise"), (0.5, "int"), (1.0, "noise"), (1e300, "noise"), (1e300, "int")))]
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def sel_inputs(case, clean=False):
    """{frame_off, idx [F][K] int32, tc [F][K], y [n_db][dy + pad], succ int32}.  ``clean``: the same without the
    non-finite values of a 'nonfinite' case."""
    rng = np.random.RandomState(8000 + case.seed)
    frame_off = np.concatenate([[0], np.cumsum(case.frames)]).astype(np.int64)
    f, k, r, w = int(frame_off[-1]), case.k, case.n_db, case.dy + case.pad
    if case.data == "int":
        y = rng.randint(-1, 2, size=(5, w)).astype(np.float64)[rng.randint(0, 5, size=r)]
        tc = rng.randint(0, 3, size=(f, k)).astype(np.float64)
    else:
        y, tc = rng.randn(r, w), rng.rand(f, k) * case.dy
    idx = rng.randint(0, r - 2, size=(f, k)).astype(np.int32)  # (the last two rows: only where a case sends them)
    succ = np.minimum(np.arange(1, r + 1), r - 1).astype(np.int32)
    succ[rng.randint(0, r - 3, size=4)] -= 1  # utterance ends inside the database
    if case.succ == "identity":
        succ = np.arange(r, dtype=np.int32)
    if case.succ == "broken":
        where = rng.permutation(r - 2)[:12]
        succ[where] = np.array([-1, r, r + 5, -2 ** 31, 2 ** 31 - 1, -3] * 2, dtype=np.int64).astype(np.int32)
    if case.invalid is not None:
        bad = rng.rand(f, k) < (0.3 if case.invalid == "some" else 0.8)
        bad[:, 0] = False
        idx[bad] = rng.choice(np.array([-1, -5, r, r + 9, 2 ** 31 - 1, -2 ** 31], dtype=np.int64), size=int(bad.sum())).astype(np.int32)
        if case.invalid == "rest" and f > 3:
            idx[3, 1:] = -1
    if case.data == "nonfinite":
        f0, f1 = int(frame_off[1]), int(frame_off[2])
        hit = rng.rand(f1 - f0, k) < 0.3
        idx[f0:f1][hit] = rng.choice([r - 2, r - 1], size=int(hit.sum()))
        succ[r - 2], succ[r - 3] = r - 2, r - 3  # (no other row leads to the two)
        if not clean:
            y[r - 2, case.dy // 2] = np.nan
            y[r - 1, 0] = np.inf
            tc[f0 + 2, 1] = np.nan
    return {"frame_off": _frozen(frame_off), "idx": _frozen(idx), "tc": _frozen(tc), "y": _frozen(y), "succ": _frozen(succ)}


@functools.lru_cache(maxsize=None)
def sel_reference(case, clean=False):
    inp = sel_inputs(case, clean)
    return tuple(_frozen(a) for a in xref.frame_select(inp["frame_off"], inp["idx"], inp["tc"], inp["y"][:, :case.dy],
                                                       inp["succ"], case.weight))


def sel_run(rt, case, only=None, clean=False, want_slot=True, want_acc=True):
    """wh_frame_select on a case -> {sel, slot, total, acc, rc, guards}.  ``only``: that utterance alone, a batch of one."""
    torch = rt.torch
    inp = sel_inputs(case, clean)
    fo = inp["frame_off"]
    utts = list(range(len(case.frames))) if only is None else [only]
    f0, f1 = int(fo[utts[0]]), int(fo[utts[-1] + 1])
    g_off = np.ascontiguousarray(fo[utts[0]:utts[-1] + 2] - f0)
    f, k = f1 - f0, case.k
    batch = rt.make_batch(np.zeros(len(g_off), dtype=np.int64), g_off)
    idx_d = rt.to_device(np.ascontiguousarray(inp["idx"][f0:f1]), dtype=np.int32)
    tc_d = rt.to_device(np.ascontiguousarray(inp["tc"][f0:f1]))
    y_d, succ_d = rt.to_device(np.ascontiguousarray(inp["y"])), rt.to_device(np.ascontiguousarray(inp["succ"]), dtype=np.int32)
    sel_w = torch.full((f + 2,), I_GUARD, dtype=torch.int32, device=rt.device)
    slot_w = torch.full((f + 2,), I_GUARD, dtype=torch.int32, device=rt.device)
    total_w = torch.full((len(utts) + 2,), D_GUARD, dtype=torch.float64, device=rt.device)
    acc_w = torch.full((f * k + 2,), D_GUARD, dtype=torch.float64, device=rt.device)
    rc = rt.lib.wh_frame_select(rt.ctx, rt.stream(), batch.handle, rt.ptr(idx_d), rt.ptr(tc_d), k, rt.ptr(y_d), case.n_db,
                                case.dy + case.pad, case.dy, rt.ptr(succ_d), float(case.weight), rt.ptr(sel_w[1:]),
                                rt.ptr(slot_w[1:]) if want_slot else None, rt.ptr(total_w[1:]),
                                rt.ptr(acc_w[1:]) if want_acc else None)
    sel_h, slot_h, total_h, acc_h = (t.cpu().numpy() for t in (sel_w, slot_w, total_w, acc_w))
    guards = all(bool(a[0] == g and a[-1] == g) for a, g in ((sel_h, I_GUARD), (slot_h, I_GUARD), (total_h, D_GUARD), (acc_h, D_GUARD)))
    if not want_slot:
        guards = guards and bool(np.all(slot_h == I_GUARD))
    if not want_acc:
        guards = guards and bool(np.all(acc_h == D_GUARD))
    guards = guards and np.array_equal(y_d.cpu().numpy(), inp["y"], equal_nan=True)
    return {"sel": sel_h[1:-1].copy(), "slot": slot_h[1:-1].copy() if want_slot else None, "total": total_h[1:-1].copy(),
            "acc": acc_h[1:-1].reshape(f, k).copy() if want_acc else None, "rc": rc, "guards": guards, "f0": f0, "f1": f1,
            "utts": utts}


def sel_compare(case, got, clean=False):
    if got["rc"] != 0:
        return ["rc %d" % got["rc"]]
    sel, slot, total, acc = sel_reference(case, clean)
    f0, f1, utts = got["f0"], got["f1"], got["utts"]
    bad = []
    if got["sel"].tobytes() != sel[f0:f1].tobytes():
        diff = np.flatnonzero(got["sel"] != sel[f0:f1])
        bad.append("sel differs in %d frames, the first %s" % (len(diff), diff[:1]))
    if got["slot"] is not None and got["slot"].tobytes() != slot[f0:f1].tobytes():
        bad.append("slot differs in %d frames" % np.count_nonzero(got["slot"] != slot[f0:f1]))
    if not same_bits(got["total"], total[utts[0]:utts[-1] + 1]):
        bad.append("total differs: %s against %s" % (got["total"], total[utts[0]:utts[-1] + 1]))
    if got["acc"] is not None and not same_bits(got["acc"], acc[f0:f1]):
        bad.append("acc differs in %d slots" % np.count_nonzero(got["acc"] != acc[f0:f1]))
    if not got["guards"]:
        bad.append("a guard value was written or y changed")
    return bad
