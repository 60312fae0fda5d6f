"""Inputs, runner and comparison shared by tests/test_hip_mlpg.py and tests/_mlpg_bounds_script.py: seeded tracks, means
and variances, the reference result of every utterance (tests/_mlpg_reference.py, computed once per process and kept),
wh_delta_features / wh_mlpg through world.dynamics, and a bit-for-bit comparison of the features, the tracks and the
pivots."""
import collections
import functools

import numpy as np

import _mlpg_reference as ref

# windows by half-width: the static one first, then up to three more; the last of each list is asymmetric
WINDOWS = {
    0: ((1.0,), (0.5,), (-2.0,), (3.0,)),
    1: ref.HTS_WINDOWS + ((0.25, -1.0, 0.5),),
    2: ((0.0, 0.0, 1.0, 0.0, 0.0), (-0.2, -0.1, 0.0, 0.1, 0.2), (2.0 / 7, -1.0 / 7, -2.0 / 7, -1.0 / 7, 2.0 / 7),
        (0.1, -0.3, 0.5, 0.2, -0.4)),
}
ASYMMETRIC = ((0.0, 1.0, 0.0), (0.25, -1.0, 0.5))

Case = collections.namedtuple("Case", "name lens d half n_win per_frame seed pad max_ws windows")
Case.__new__.__defaults__ = (True, 0, 0, None, None)


def case_windows(case):
    return case.windows if case.windows is not None else WINDOWS[case.half][:case.n_win]


def edge_lengths(half):
    """1, 2, 3, 2L, 2L+1, 4L+1 (the band and the window against the ends), 63, 64, 65 and 300."""
    return tuple(sorted({1, 2, 3, 2 * half, 2 * half + 1, 4 * half + 1, 63, 64, 65, 300} - {0}))


@functools.lru_cache(maxsize=None)
def inputs(T, d, windows, seed, per_frame):
    """(x [T][d], mean [T][n_win d], var [T][n_win d] or [n_win d]), read-only: a random walk, its features plus noise,
    and variances log-uniform over sixteen decades.  The row of variances of the ldv = 0 form depends on (d, windows,
    seed) only, so that the utterances of a case share it."""
    rng = np.random.RandomState((seed * 7919 + T * 31 + d) % (2 ** 31))
    x = np.cumsum(rng.randn(T, d), axis=0)
    mean = ref.delta_features(x, windows) + 0.1 * rng.randn(T, len(windows) * d)
    if per_frame:
        var = 10.0 ** rng.uniform(-8, 8, size=(T, len(windows) * d))
    else:
        var = 10.0 ** np.random.RandomState(seed * 104729 + d).uniform(-8, 8, size=len(windows) * d)
    for a in (x, mean, var):
        a.setflags(write=False)
    return x, mean, var


@functools.lru_cache(maxsize=None)
def reference(T, d, windows, seed, per_frame):
    """(features of x, track, pivots) of one utterance."""
    x, mean, var = inputs(T, d, windows, seed, per_frame)
    c, piv = ref.mlpg(mean, var, windows)
    return ref.delta_features(x, windows), c, piv


@functools.lru_cache(maxsize=None)
def kernel_cases():
    cases = []
    ds = (1, 2, 39, 63, 64, 65, 130)
    n = 0
    for half in (0, 1, 2):
        for n_win in (1, 2, 3, 4):
            d = ds[n % len(ds)]
            cases.append(Case("L=%d n_win=%d d=%d %s" % (half, n_win, d, "per-frame" if n % 2 == 0 else "ldv=0"),
                              edge_lengths(half), d, half, n_win, per_frame=n % 2 == 0, seed=n))
            n += 1
    for d in ds:  # the HTS windows at every d, the variance form the other way round
        cases.append(Case("HTS d=%d %s" % (d, "ldv=0" if d % 2 else "per-frame"), edge_lengths(1), d, 1, 3,
                          per_frame=d % 2 == 0, seed=20 + d))
    cases.append(Case("asymmetric window", edge_lengths(1), 39, 1, 2, seed=40, windows=ASYMMETRIC))
    cases.append(Case("rows inside wider tensors", (1, 5, 64, 65, 130), 39, 1, 3, seed=41, pad=3))
    cases.append(Case("rows inside wider tensors L=2", (2, 4, 9, 70), 65, 2, 4, seed=42, pad=2))
    cases.append(Case("d=1, 130 utterances in shared waves", tuple(1 + (37 * u) % 90 for u in range(130)), 1, 1, 3, seed=43))
    cases.append(Case("d=1, 130 utterances, L=2 ldv=0", tuple(1 + (53 * u) % 70 for u in range(130)), 1, 2, 3,
                      per_frame=False, seed=44))
    return tuple(cases)


RAGGED = Case("ragged batch, empty utterances in the middle and at the end", (70, 1, 0, 129, 3, 0, 0, 64, 33, 0), 39, 1, 3,
              seed=50)
RAGGED_L2 = Case("ragged batch L=2", (5, 0, 200, 2, 66, 0), 65, 2, 4, seed=51)


def _wide(rt, a, pad):
    """The rows inside a wider tensor; what lies beside them must never be read."""
    if not pad:
        return rt.to_device(np.array(a))  # (a copy: the cached inputs are read-only)
    wide = np.full((a.shape[0], a.shape[1] + 2 * pad), np.nan)
    wide[:, pad:pad + a.shape[1]] = a
    return rt.to_device(wide)[:, pad:pad + a.shape[1]]


def assemble(case, only=None):
    """(frame offsets, x, mean, var) of the case's batch on the host (``only``: that utterance alone)."""
    win = case_windows(case)
    lens = case.lens if only is None else (case.lens[only],)
    parts = [inputs(T, case.d, win, case.seed, case.per_frame) for T in lens]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    width = len(win) * case.d
    x = np.concatenate([p[0] for p in parts]).reshape(-1, case.d)
    mean = np.concatenate([p[1] for p in parts]).reshape(-1, width)
    var = np.concatenate([p[2] for p in parts]).reshape(-1, width) if case.per_frame else parts[0][2]
    return off, x, mean, var


def run(rt, case, only=None):
    """wh_delta_features on the tracks and wh_mlpg on the means and variances: host arrays (features, track, pivots)."""
    from world.dynamics import DEFAULT_MAX_WORKSPACE_BYTES, delta_features_device, mlpg_device

    win = case_windows(case)
    off, x, mean, var = assemble(case, only)
    batch = rt.make_batch(np.zeros(len(off), dtype=np.int64), off)
    feat = delta_features_device(rt, batch, _wide(rt, x, case.pad), win)
    var_d = _wide(rt, var, case.pad) if case.per_frame else rt.to_device(np.array(var))
    c, piv = mlpg_device(rt, batch, _wide(rt, mean, case.pad), var_d, win,
                         max_workspace_bytes=case.max_ws or DEFAULT_MAX_WORKSPACE_BYTES, want_pivots=True)
    return feat.cpu().numpy(), c.cpu().numpy(), piv.cpu().numpy()


KEYS = ("features", "track", "pivots")


def same_bits(x, y):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return x.shape == y.shape and x.tobytes() == y.tobytes()


def split(case, got, only=None):
    """The run's three arrays cut into utterances: a list of {key: array}."""
    lens = case.lens if only is None else (case.lens[only],)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return [{k: a[off[u]:off[u + 1]] for k, a in zip(KEYS, got)} for u in range(len(lens))]


def compare(got, case, only=None):
    """[] when every utterance equals the reference bit for bit, else 'utterance u (T): key' strings."""
    win = case_windows(case)
    lens = case.lens if only is None else (case.lens[only],)
    bad = []
    for u, (T, have) in enumerate(zip(lens, split(case, got, only))):
        want = dict(zip(KEYS, reference(T, case.d, win, case.seed, case.per_frame)))
        for key in KEYS:
            if not same_bits(have[key], want[key]):
                bad.append("utterance %d (T=%d): %s, %d of %d differ" % (u, T, key, int(np.sum(have[key] != want[key])),
                                                                         have[key].size))
    return bad
