"""A NumPy model of the workgroup reductions of csrc/wh_reduce.h, and the inputs on which the order of a sum shows in its
bits.  Shared by tests/test_reduce_tree_model.py (no GPU: what the model and the inputs are worth) and
tests/test_hip_reduce.py (the kernels against the model).

The tree of wh::wave_sum over the 64 lanes of a wave, level by level (lane l adds the value of the lane named):
  1  quad_perm [1,0,3,2]   l ^ 1
  2  quad_perm [2,3,0,1]   l ^ 2
  3  row_half_mirror       7 - l inside its group of 8
  4  row_mirror            15 - l inside its row of 16
  5  row_bcast:15          rows 1 and 3: lane 15 of the row below; rows 0 and 2 add 0.0
  6  row_bcast:31          rows 2 and 3: lane 31; rows 0 and 1 add 0.0
and lane 63 holds the total.  The workgroup's total adds the waves' in ascending order, starting from 0.0."""
import numpy as np

LANES = np.arange(64)
SOURCES = [
    LANES ^ 1,
    LANES ^ 2,
    (LANES & ~7) | (7 - (LANES & 7)),
    (LANES & ~15) | (15 - (LANES & 15)),
    np.where((LANES >> 4) & 1, (LANES & ~15) - 1, -1),
    np.where(LANES >= 32, 31, -1),
]


def wave_total(v, flips=None):
    """Lane 63 after the six levels.  flips: per level a [64] boolean array, True where the node adds partner + own
    instead of own + partner."""
    v = np.array(v, dtype=np.float64)
    assert v.shape == (64,)
    with np.errstate(invalid="ignore", over="ignore"):
        for level, src in enumerate(SOURCES):
            other = np.where(src >= 0, v[np.maximum(src, 0)], 0.0)
            if flips is None:
                v = v + other
            else:
                v = np.where(flips[level], other + v, v + other)
    return v[63]


def block_total(v, flips=None):
    """The workgroup's total of v[NT]: the waves' totals added in ascending order from 0.0."""
    v = np.asarray(v, dtype=np.float64)
    assert v.ndim == 1 and len(v) % 64 == 0
    t = np.float64(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for w in range(len(v) // 64):
            t = t + wave_total(v[64 * w:64 * w + 64], None if flips is None else flips[w])
    return t


def left_to_right(v):
    t = np.float64(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for x in np.asarray(v, dtype=np.float64):
            t = t + x
    return t


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- inputs on which association is visible in the bits: name -> f(nt, k) -> [nt] values of the k-th summand ----------
SINGLE_LANES = (0, 1, 2, 15, 16, 31, 32, 63)


def scaled_normals(nt, k, seed=0):
    rng = np.random.RandomState(1000 * seed + 10 * k + nt)
    return rng.randn(nt) * 2.0 ** rng.randint(-60, 61, nt)


def big_cancelling(nt, k):
    """1, 1e16, -1e16 repeated, rotated over the lanes by k and scaled per summand."""
    return np.roll(np.resize([1.0, 1e16, -1e16], nt), k) * (k + 1)


def signed_zeros(nt, k):
    return np.resize([0.0, -0.0] if k % 2 == 0 else [-0.0, 0.0], nt)


def single_lane(nt, k, lane):
    """One non-zero lane per wave, a value of its own for every summand and wave."""
    v = np.zeros(nt)
    for w in range(nt // 64):
        v[64 * w + lane] = 3.0 ** k * (1.0 + w / 16.0) + 2.0 ** -30  # ([3^k, 1.44 * 3^k): no two alike)
    return v


def input_sets(nt, k_values):
    """[(name, [k_values][nt] array)]: every pattern in all summands, then a different pattern in every summand."""
    sets = [
        ("scaled normals", np.stack([scaled_normals(nt, k) for k in range(k_values)])),
        ("1, 1e16, -1e16", np.stack([big_cancelling(nt, k) for k in range(k_values)])),
        ("signed zeros", np.stack([signed_zeros(nt, k) for k in range(k_values)])),
    ]
    for lane in SINGLE_LANES:
        sets.append(("lane %d alone" % lane, np.stack([single_lane(nt, k, lane) for k in range(k_values)])))
    kinds = [lambda k: scaled_normals(nt, k, seed=1), lambda k: big_cancelling(nt, k), lambda k: single_lane(nt, k, 31),
             lambda k: signed_zeros(nt, k), lambda k: scaled_normals(nt, k, seed=2)]
    for shift in range(2):
        sets.append(("a pattern per summand, from %d" % shift,
                     np.stack([kinds[(k + shift) % len(kinds)](k) for k in range(k_values)])))
    return sets
