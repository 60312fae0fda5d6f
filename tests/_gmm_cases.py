"""Shapes, data, raw C-ABI runners and the list of runs shared by tests/test_hip_gmm.py and tests/_gmm_bounds_script.py.

Every run is a function of the runtime that returns {name: host array}; the GPU test compares them with the reference
(tests/_gmm_reference.py), the bounds script runs the same list under the bounds build and reports a digest of each
result, which the test compares with the shipped library's."""
import collections
import functools
import hashlib

import numpy as np

import _gmm_reference as ref

ROW_TILE, SPLIT_ROWS = 128, 4096  # world.gmm.ROW_TILE / SPLIT_ROWS (tests/test_gmm_host.py holds them to the kernel source)

# (n_rows, d, M): a star around the centre plus twenty seeded random triples
CENTRE = (129, 39, 5)
N_ROWS = (1, 15, 16, 17, ROW_TILE - 1, ROW_TILE, ROW_TILE + 1, SPLIT_ROWS - 1, SPLIT_ROWS, SPLIT_ROWS + 1, 2 * SPLIT_ROWS + 3)
DS = (1, 3, 4, 5, 15, 16, 17, 39, 78, 156, 160)
MS = (1, 2, 5, 64)
REAL_SHAPES = ((129, 39, 5), (300, 156, 3), (40, 160, 64))


@functools.lru_cache(maxsize=None)
def exact_shapes():
    out = [CENTRE]
    out += [(n, CENTRE[1], CENTRE[2]) for n in N_ROWS if n != CENTRE[0]]
    out += [(CENTRE[0], d, CENTRE[2]) for d in DS if d != CENTRE[1]]
    out += [(CENTRE[0], CENTRE[1], m) for m in MS if m != CENTRE[2]]
    rng = np.random.RandomState(20)
    out += [(int(rng.choice(N_ROWS)), int(rng.choice(DS)), int(rng.choice(MS))) for _ in range(20)]
    return tuple(out)


# ---- raw calls: tensors in, row strides taken from the tensors -----------------------------------------------------------
def raw_estep(rt, x, mu, whiten, logc, ll=None, gamma=None, rowll=None, best=None, n=None):
    from world import _hip
    m, d = int(mu.shape[0]), int(mu.shape[1])
    n = int(x.shape[0]) if n is None else n
    _hip.check(rt.lib.wh_gmm_estep(rt.ctx, rt.stream(), rt.ptr(x), n, _hip.ld(x), d, m, rt.ptr(mu), rt.ptr(whiten), rt.ptr(logc),
                                   rt.ptr(ll), _hip.ld(ll) if ll is not None else m, rt.ptr(gamma),
                                   _hip.ld(gamma) if gamma is not None else m, rt.ptr(rowll), rt.ptr(best)))


def raw_stats(rt, x, gamma, mu, s0, s1, s2, n=None):
    from world import _hip
    m, d = int(mu.shape[0]), int(mu.shape[1])
    n = int(x.shape[0]) if n is None else n
    _hip.check(rt.lib.wh_gmm_stats(rt.ctx, rt.stream(), rt.ptr(x), n, _hip.ld(x), d, m, rt.ptr(gamma), _hip.ld(gamma), rt.ptr(mu),
                                   rt.ptr(s0), rt.ptr(s1), rt.ptr(s2)))


def raw_convert(rt, x, mu_x, a, mu_y, out, best=None, g=None, n=None):
    from world import _hip
    m, dx, dy = int(a.shape[0]), int(a.shape[1]), int(a.shape[2])
    n = int(x.shape[0]) if n is None else n
    _hip.check(rt.lib.wh_gmm_convert(rt.ctx, rt.stream(), rt.ptr(x), n, _hip.ld(x), dx, dy, m, rt.ptr(mu_x), rt.ptr(a), rt.ptr(mu_y),
                                     rt.ptr(best), rt.ptr(g), _hip.ld(g) if g is not None else m, rt.ptr(out), _hip.ld(out)))


def estep_all(rt, x, mu, whiten, logc):
    """{'ll', 'gamma', 'rowll', 'best'} of host arrays, through contiguous device tensors."""
    import torch
    n, m = len(x), len(mu)
    ll, gamma, rowll = rt.empty((n, m)), rt.empty((n, m)), rt.empty((n,))
    best = rt.empty((n,), torch.int32)
    raw_estep(rt, rt.to_device(x), rt.to_device(mu), rt.to_device(whiten), rt.to_device(logc), ll, gamma, rowll, best)
    return {"ll": ll.cpu().numpy(), "gamma": gamma.cpu().numpy(), "rowll": rowll.cpu().numpy(), "best": best.cpu().numpy()}


def stats_all(rt, x, gamma, mu):
    m, d = mu.shape
    s0, s1, s2 = rt.empty((m,)), rt.empty((m, d)), rt.empty((m, d, d))
    raw_stats(rt, rt.to_device(x), rt.to_device(gamma), rt.to_device(mu), s0, s1, s2)
    return {"s0": s0.cpu().numpy(), "s1": s1.cpu().numpy(), "s2": s2.cpu().numpy()}


def convert_all(rt, x, mu_x, a, mu_y, best=None, g=None):
    out = rt.empty((len(x), a.shape[2]))
    raw_convert(rt, rt.to_device(x), rt.to_device(mu_x), rt.to_device(a), rt.to_device(mu_y), out,
                None if best is None else rt.to_device(best, np.int32), None if g is None else rt.to_device(g))
    return {"out": out.cpu().numpy()}


# ---- exact cases: integers in [-8, 8], every partial sum exact in FP64 in any order ----------------------------------------
def _ints(rng, shape):
    return rng.randint(-8, 9, size=shape).astype(np.float64)


@functools.lru_cache(maxsize=None)
def exact_data(shape):
    """Inputs and the integer results of the three kernels for (n, d, M).  The products run through float64 BLAS: every
    value and partial sum is an integer below 2^53, so any order gives the exact integers (asserted)."""
    n, d, m = shape
    rng = np.random.RandomState((n * 31 + d * 7919 + m * 104729) % (2 ** 31))
    x, mu = _ints(rng, (n, d)), _ints(rng, (m, d))
    whiten = np.triu(_ints(rng, (m, d, d)))
    gamma = rng.randint(0, 2, size=(n, m)).astype(np.float64)
    dx = max(1, d // 2)
    dy = max(1, d - dx)
    a, mu_y = _ints(rng, (m, dx, dy)), _ints(rng, (m, dy))
    best = rng.randint(0, m, size=n).astype(np.int32)
    q = np.stack([np.sum(((x - mu[k]) @ whiten[k]) ** 2, axis=1) for k in range(m)], axis=1)
    ll = 0.0 - 0.5 * q
    e = [x - mu[k] for k in range(m)]
    s0 = np.sum(gamma, axis=0)
    s1 = np.stack([gamma[:, k] @ e[k] for k in range(m)])
    s2 = np.stack([(e[k] * gamma[:, k:k + 1]).T @ e[k] for k in range(m)])
    v = np.stack([mu_y[k] + (x[:, :dx] - mu[k, :dx]) @ a[k] for k in range(m)])
    out = v[best, np.arange(n)]
    for arr in (q, s0, s1, s2, out):
        assert np.all(arr == np.rint(arr)) and np.max(np.abs(arr), initial=0.0) < 2.0 ** 52
        arr.astype(np.int64)
    res = {"x": x, "mu": mu, "whiten": whiten, "gamma": gamma, "dx": dx, "a": a, "mu_y": mu_y, "best": best,
           "ll": ll, "first_best": np.argmax(ll, axis=1).astype(np.int32), "s0": s0, "s1": s1, "s2": s2, "out": out}
    for arr in res.values():
        if isinstance(arr, np.ndarray):
            arr.setflags(write=False)
    return res


def run_exact(rt, shape):
    dat = exact_data(shape)
    n, d, m = shape
    dx = dat["dx"]
    got = {}
    e = estep_all(rt, dat["x"], dat["mu"], dat["whiten"], np.zeros(m))
    got["ll"], got["first_best"] = e["ll"], e["best"]
    got.update(stats_all(rt, dat["x"], dat["gamma"], dat["mu"]))
    got.update(convert_all(rt, dat["x"][:, :dx], np.ascontiguousarray(dat["mu"][:, :dx]), dat["a"], dat["mu_y"], best=dat["best"]))
    return got


EXACT_KEYS = ("ll", "first_best", "s0", "s1", "s2", "out")


def same_bits(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()


# ---- real data ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def real_data(shape):
    """A random mixture with covariance condition numbers up to 1e6, rows drawn from it, the tables world.gmm makes of
    it, a Dirichlet gamma, a random best."""
    from world import gmm

    n, d, m = shape
    rng = np.random.RandomState(1000 + n + d + m)
    w, mu, cov = ref.random_mixture(m, d, rng, 1e6, spread=0.5)
    x, _ = ref.sample(w, mu, cov, n, rng)
    dx = (d + 1) // 2
    t = gmm.JointGMM(w, mu, cov, dx).host_tables()
    res = {"x": x, "mu": mu, "whiten": t["whiten"], "logc": t["logc"], "dx": dx, "a": t["a"], "mu_x": t["mu_x"],
           "mu_y": t["mu_y"], "gamma": rng.dirichlet(np.full(m, 0.3), size=n),
           "best": rng.randint(0, m, size=n).astype(np.int32)}
    for arr in res.values():
        if isinstance(arr, np.ndarray):
            arr.setflags(write=False)
    return res


def run_real(rt, shape):
    dat = real_data(shape)
    dx = dat["dx"]
    got = estep_all(rt, dat["x"], dat["mu"], dat["whiten"], dat["logc"])
    got.update(stats_all(rt, dat["x"], dat["gamma"], dat["mu"]))
    xs = np.ascontiguousarray(dat["x"][:, :dx])
    got["out_best"] = convert_all(rt, xs, dat["mu_x"], dat["a"], dat["mu_y"], best=dat["best"])["out"]
    got["out_mmse"] = convert_all(rt, xs, dat["mu_x"], dat["a"], dat["mu_y"], g=dat["gamma"])["out"]
    return got


# ---- strides: rows inside wider tensors, NaN beside them, sentinels around and between the rows of every output ----------
SENTINEL = -7.25
STRIDE_SHAPE = (131, 39, 5)


def _wide(rt, a, pad):
    wide = np.full((a.shape[0], a.shape[1] + 2 * pad), np.nan)
    wide[:, pad:pad + a.shape[1]] = a
    return rt.to_device(wide)[:, pad:pad + a.shape[1]]


def run_strided(rt, shape=STRIDE_SHAPE):
    """Every entry with ldx != d, ldg != M, ldl != M, ldo != dy.  Returns the results cut out of their buffers and, under
    'untouched', whether every cell outside them still holds the sentinel."""
    import torch
    dat = real_data(shape)
    n, d, m = shape
    dx = dat["dx"]
    dy = d - dx
    x = _wide(rt, dat["x"], 3)
    full = lambda *s: torch.full(s, SENTINEL, dtype=torch.float64, device=rt.device)  # noqa: E731
    ll_b, ga_b = full(n + 2, m + 2), full(n + 2, m + 5)
    rl_b = full(n + 2)
    be_b = torch.full((n + 2,), -7, dtype=torch.int32, device=rt.device)
    raw_estep(rt, x, rt.to_device(dat["mu"]), rt.to_device(dat["whiten"]), rt.to_device(dat["logc"]), ll_b[1:n + 1, 1:m + 1],
              ga_b[1:n + 1, 2:m + 2], rl_b[1:n + 1], be_b[1:n + 1])
    s0_b, s1_b, s2_b = full(m + 2), full(m * d + 2), full(m * d * d + 2)
    raw_stats(rt, x, _wide(rt, dat["gamma"], 2), rt.to_device(dat["mu"]), s0_b[1:m + 1], s1_b[1:m * d + 1], s2_b[1:m * d * d + 1])
    ob_b, om_b = full(n + 2, dy + 3), full(n + 2, dy + 3)
    xs = x[:, :dx]  # (the source columns of the wide rows: what lies beside them is the target's columns and NaN)
    tabs = [rt.to_device(dat[k]) for k in ("mu_x", "a", "mu_y")]
    raw_convert(rt, xs, *tabs, ob_b[1:n + 1, 1:dy + 1], best=rt.to_device(dat["best"], np.int32))
    raw_convert(rt, xs, *tabs, om_b[1:n + 1, 2:dy + 2], g=_wide(rt, dat["gamma"], 1))
    got, clean = {}, True

    def cut(name, buf, *index):
        nonlocal clean
        host = buf.cpu().numpy()
        got[name] = np.ascontiguousarray(host[index])
        rest = np.ones(host.shape, dtype=bool)
        rest[index] = False
        clean = clean and bool(np.all(host[rest] == (SENTINEL if host.dtype == np.float64 else -7)))

    rows = slice(1, n + 1)
    cut("ll", ll_b, rows, slice(1, m + 1))
    cut("gamma", ga_b, rows, slice(2, m + 2))
    cut("rowll", rl_b, rows)
    cut("best", be_b, rows)
    cut("s0", s0_b, slice(1, m + 1))
    cut("s1", s1_b, slice(1, m * d + 1))
    cut("s2", s2_b, slice(1, m * d * d + 1))
    cut("out_best", ob_b, rows, slice(1, dy + 1))
    cut("out_mmse", om_b, rows, slice(2, dy + 2))
    got["s1"], got["s2"] = got["s1"].reshape(m, d), got["s2"].reshape(m, d, d)
    got["untouched"] = np.array([clean])
    return got


# ---- the list of runs ------------------------------------------------------------------------------------------------------
Run = collections.namedtuple("Run", "name fn")


@functools.lru_cache(maxsize=None)
def all_runs():
    runs = [Run("exact n=%d d=%d M=%d #%d" % (s + (i,)), functools.partial(run_exact, shape=s)) for i, s in enumerate(exact_shapes())]
    runs += [Run("real n=%d d=%d M=%d" % s, functools.partial(run_real, shape=s)) for s in REAL_SHAPES]
    runs.append(Run("strided n=%d d=%d M=%d" % STRIDE_SHAPE, run_strided))
    return tuple(runs)


def digest(got):
    h = hashlib.blake2b(digest_size=16)
    for k in sorted(got):
        a = np.ascontiguousarray(got[k])
        h.update(k.encode())
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()
