"""Inputs, runners and comparison shared by tests/test_hip_lsf_chain.py, tests/_lsf_chain_bounds_script.py and the host
tests: rows of angles of every kind a repair can meet, seeded rows of cosines with index lists for the distortion, the
reference result of every case (tests/_lsf_chain_reference.py, computed once per process and kept read-only) and the two C
entries called directly — inputs and outputs inside wider tensors whose NaN guard bands must survive."""
import collections
import functools

import numpy as np

import _lsf_cases as lc
import _lsf_chain_reference as cref

ORDERS = (2, 4, 24, 40, 64)
FRAMES = (1, 63, 64, 65, 129)
BINS = (129, 513, 1025, 2049)
PAIRS = (1, 7, 8, 9, 65)
ROW_KINDS = ("valid", "reversed", "equal", "outside", "plus_inf", "minus_inf", "nan_first", "nan_middle", "nan_last",
             "random")

RepairCase = collections.namedtuple("RepairCase", "name p frames gap pad seed")
DistCase = collections.namedtuple("DistCase", "name p pairs k_bins pad seed")


def tight_gap(p):
    """Just under pi / (p + 2), the largest gap world.lsf takes: the repaired row is all but forced."""
    return float(np.pi / (p + 2) * (1.0 - 2.0 ** -40))


@functools.lru_cache(maxsize=None)
def repair_cases():
    """Every order with every frame count, inside tensors one or two guard columns wider on either side; a usual gap and
    the tight one take turns."""
    cases = []
    for i, p in enumerate(ORDERS):
        for j, f in enumerate(FRAMES):
            n = i * len(FRAMES) + j
            tight = (i + j) % 2 == 1
            gap = tight_gap(p) if tight else 0.3 / (p + 2)
            cases.append(RepairCase("p=%d F=%d%s pad=%d" % (p, f, " tight" if tight else "", 2 if n % 3 else 1), p, f, gap,
                                    2 if n % 3 else 1, n))
    return tuple(cases)


def row_of_kind(kind, p, gap, rng):
    valid = np.pi * (np.arange(p) + 1.0) / (p + 1)  # evenly spread: at least pi / (p + 1) > gap apart, and from the ends
    if kind == "valid":
        return valid
    if kind == "reversed":
        return valid[::-1].copy()
    if kind == "equal":
        return np.full(p, 1.0)
    if kind == "outside":
        return np.linspace(-1.0, 5.0, p)
    w = np.sort(rng.uniform(-0.2, np.pi + 0.2, size=p)) if kind != "random" else rng.uniform(-0.2, np.pi + 0.2, size=p)
    at = {"plus_inf": p // 3, "minus_inf": (2 * p) // 3, "nan_first": 0, "nan_middle": p // 2, "nan_last": p - 1}.get(kind)
    if at is not None:
        w[at] = {"plus_inf": np.inf, "minus_inf": -np.inf}.get(kind, np.nan)
    return w


@functools.lru_cache(maxsize=None)
def repair_rows_of(case):
    """(w [F][p], kinds [F]): row r is of kind (r + seed) % 10, so every frame count meets other kinds first."""
    rng = np.random.RandomState(2000 + case.seed)
    kinds = [ROW_KINDS[(r + case.seed) % len(ROW_KINDS)] for r in range(case.frames)]
    w = np.stack([row_of_kind(k, case.p, case.gap, rng) for k in kinds])
    w.setflags(write=False)
    return w, tuple(kinds)


@functools.lru_cache(maxsize=None)
def repair_reference(case):
    out, changed = cref.repair(repair_rows_of(case)[0], *cref.gap_hi(case.gap))
    return lc._frozen(out, changed)


@functools.lru_cache(maxsize=None)
def all_kinds_case(p):
    """The ten kinds of row twice over (a NaN row next to clean ones on both sides), at the usual gap."""
    return RepairCase("p=%d every kind" % p, p, 2 * len(ROW_KINDS), 0.3 / (p + 2), 1, 0)


def run_repair(rt, w, gap, hi, pad=0, in_place=False, want_changed=True):
    """wh_lsf_repair -> {out, changed, guards, rc}; in place: the input's own wide tensor is the output."""
    from world import _hip

    w = np.ascontiguousarray(w, dtype=np.float64)
    f, p = w.shape
    torch = rt.torch
    if in_place:
        wide = np.full((f, p + 2 * pad), np.nan)
        wide[:, pad:pad + p] = w
        wide_d = rt.to_device(wide)
        src = dst = wide_d[:, pad:pad + p]
        ldo = p + 2 * pad
    else:
        src = lc._wide_in(rt, w, pad)
        out = lc._Out(rt, f, p, pad)
        dst, ldo, wide_d = out.view, out.ld, out.wide
    changed = torch.full((f + 2,), -7, dtype=torch.int32, device=rt.device) if want_changed else None
    rc = rt.lib.wh_lsf_repair(rt.ctx, rt.stream(), rt.ptr(src), f, _hip.ld(src) if not in_place else ldo, p, gap, hi,
                              rt.ptr(dst), ldo, rt.ptr(changed[1:]) if want_changed else None)
    host = wide_d.cpu().numpy()
    guards = bool(np.all(np.isnan(np.concatenate([host[:, :pad], host[:, pad + p:]], axis=1))))
    res = {"out": host[:, pad:pad + p].copy(), "guards": guards, "rc": rc}
    if want_changed:
        ch = changed.cpu().numpy()
        res["changed"] = ch[1:-1].copy()
        res["guards"] = guards and ch[0] == -7 and ch[-1] == -7
    if not in_place and pad:  # the input is left as it was
        res["guards"] = res["guards"] and lc.same_bits(src.cpu().numpy(), w)
    return res


def compare_repair(got, want_out, want_changed):
    bad = []
    if got["rc"] != 0:
        bad.append("rc %d" % got["rc"])
    if not lc.same_bits(got["out"], want_out):
        bad.append("out: %d of %d differ" % (int(np.sum(~((got["out"] == want_out) | (np.isnan(got["out"]) & np.isnan(want_out))))),
                                             want_out.size))
    if "changed" in got and not np.array_equal(got["changed"], want_changed):
        bad.append("changed differs in %d frames" % int(np.sum(got["changed"] != want_changed)))
    if not got["guards"]:
        bad.append("a guard band was written")
    return bad


# ---- distortion --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dist_cases():
    """Every order with every pair count; the bins and the guard bands take turns."""
    cases = []
    for i, p in enumerate(ORDERS):
        for j, n in enumerate(PAIRS):
            k = i * len(PAIRS) + j
            cases.append(DistCase("p=%d pairs=%d K=%d%s" % (p, n, BINS[k % 4], " wide" if k % 2 else ""), p, n, BINS[k % 4],
                                  3 if k % 2 else 0, k))
    return tuple(cases)


def cosine_rows(n, p, rng, spread=1.0):
    """[n][p + 1]: a gain column (not read: NaN) and the cosines of p ascending angles inside (0, pi)."""
    w = np.sort(rng.uniform(0.02, np.pi - 0.02, size=(n, p)), axis=1)
    even = np.pi * (np.arange(p) + 1.0) / (p + 1)
    w = spread * w + (1.0 - spread) * even[None, :]
    return np.concatenate([np.full((n, 1), np.nan), np.cos(w)], axis=1)


@functools.lru_cache(maxsize=None)
def dist_inputs(case):
    """(rows_a [na][p + 1], rows_b [nb][p + 1], idx_a [n], idx_b [n]): more rows than pairs on side a, fewer on side b, the
    indices with repeats; rows of b are rows of a moved a little, so that t is a distortion and not a coin toss."""
    rng = np.random.RandomState(3000 + case.seed)
    na, nb = case.pairs + 3, max(1, case.pairs - 2)
    rows_a = cosine_rows(na, case.p, rng)
    rows_b = cosine_rows(nb, case.p, rng, spread=0.5)
    idx_a = rng.randint(0, na, size=case.pairs).astype(np.int64)
    idx_b = rng.randint(0, nb, size=case.pairs).astype(np.int64)
    return lc._frozen(rows_a, rows_b, idx_a, idx_b)


@functools.lru_cache(maxsize=None)
def dist_reference(case):
    """(out [n][2], b1 [n], b2 [n]): the reference's sums and the bound between it and the device (order_bounds)."""
    rows_a, rows_b, idx_a, idx_b = dist_inputs(case)
    out = cref.distortion(rows_a, rows_b, case.k_bins, idx_a, idx_b)
    t = cref.log_ratio(rows_a[idx_a, 1:], rows_b[idx_b, 1:], case.k_bins)
    b1, b2 = cref.order_bounds(t)
    return lc._frozen(out, b1, b2)


def run_distortion(rt, rows_a, rows_b, k_bins, idx_a=None, idx_b=None, pad=0):
    """wh_lsf_distortion -> {out [n][2], guards, rc}; the output has a guard pair in front and behind."""
    from world import _hip
    from world.lsf import bin_table

    a_d, b_d = lc._wide_in(rt, rows_a, pad), lc._wide_in(rt, rows_b, pad)
    p = int(a_d.shape[1]) - 1
    torch = rt.torch
    ia = None if idx_a is None else torch.from_numpy(np.array(idx_a, dtype=np.int64)).to(rt.device)
    ib = None if idx_b is None else torch.from_numpy(np.array(idx_b, dtype=np.int64)).to(rt.device)
    n = len(rows_a) if idx_a is None and idx_b is None else len(idx_a if idx_a is not None else idx_b)
    wide = torch.full((n + 2, 2), float("nan"), dtype=torch.float64, device=rt.device)
    wide[0] = wide[-1] = -7.0
    rc = rt.lib.wh_lsf_distortion(rt.ctx, rt.stream(), rt.ptr(a_d), int(a_d.shape[0]), _hip.ld(a_d), rt.ptr(b_d),
                                  int(b_d.shape[0]), _hip.ld(b_d), p, rt.ptr(ia), rt.ptr(ib), n,
                                  _hip.f64p(bin_table(k_bins)), k_bins, rt.ptr(wide[1:]))
    host = wide.cpu().numpy()
    return {"out": host[1:-1].copy(), "guards": bool(np.all(host[0] == -7.0) and np.all(host[-1] == -7.0)), "rc": rc}


def compare_distortion(got, want, b1, b2):
    """[] when the two sums are within the bounds (a NaN where the reference has one) and the guards are intact; the worst
    error / bound ratio is returned beside it."""
    bad, worst = [], 0.0
    if got["rc"] != 0:
        bad.append("rc %d" % got["rc"])
    for col, b in ((0, b1), (1, b2)):
        g, w = got["out"][:, col], want[:, col]
        nan = np.isnan(w)
        if not np.array_equal(np.isnan(g), nan):
            bad.append("column %d: NaN in other pairs than the reference's" % col)
            continue
        with np.errstate(all="ignore"):
            err = np.abs(g[~nan] - w[~nan])
        over = err > b[~nan]
        if over.any():
            bad.append("column %d: %d pairs over the bound, worst %.3g x" % (col, int(over.sum()), float(np.max(err / b[~nan]))))
        if err.size and np.all(b[~nan] > 0):
            worst = max(worst, float(np.max(err / b[~nan])))
    if not got["guards"]:
        bad.append("a guard pair was written")
    return bad, worst
