"""CPU: tests/_dtw_reference.py — the NumPy statement of wh_dtw's contract that the GPU tests compare with bit for bit —
against a brute-force enumeration of every monotone path, and its tie order, band and map rule on their own."""
import itertools

import numpy as np

import _dtw_reference as ref


def _all_paths(n, m):
    """Every path from (0, 0) to (n-1, m-1) by the moves (1, 1), (1, 0), (0, 1)."""
    out = []

    def walk(i, j, path):
        path = path + [(i, j)]
        if (i, j) == (n - 1, m - 1):
            out.append(path)
            return
        if i + 1 < n and j + 1 < m:
            walk(i + 1, j + 1, path)
        if i + 1 < n:
            walk(i + 1, j, path)
        if j + 1 < m:
            walk(i, j + 1, path)

    walk(0, 0, [])
    return out


def test_cost_is_the_minimum_over_every_monotone_path():
    """d = 1 and small-integer features: every local cost |a - b| and every sum is exact."""
    rng = np.random.RandomState(0)
    for n, m in itertools.product(range(1, 6), repeat=2):
        paths = _all_paths(n, m)
        for _ in range(3):
            a = rng.randint(-3, 4, size=(n, 1)).astype(np.float64)
            b = rng.randint(-3, 4, size=(m, 1)).astype(np.float64)
            r = ref.dtw(a, b)
            c = np.abs(a[:, 0][:, None] - b[:, 0][None, :])
            assert np.array_equal(ref.local_cost(a, b), c)
            sums = [sum(c[i, j] for i, j in p) for p in paths]
            assert r["cost"] == min(sums), (n, m)
            assert ref.well_formed(r["path_a"], r["path_b"], n, m)
            assert max(n, m) <= r["length"] <= n + m - 1
            assert sum(c[i, j] for i, j in zip(r["path_a"], r["path_b"])) == r["cost"]
            assert r["acc"][-1, -1] == r["cost"] and r["mean"] == r["cost"] / r["length"]
            # D of every cell is the best cost of a path that ends there
            for i, j in itertools.product(range(n), range(m)):
                best = min(sum(c[p, q] for p, q in path) for path in _all_paths(i + 1, j + 1))
                assert r["acc"][i, j] == best


def test_ties_go_to_the_diagonal_then_to_the_source_step():
    """All-equal features: every D is 0 and every comparison ties.  Walking back from the end the strict < keeps the
    diagonal until row 0 or column 0 is reached, where the only predecessor that exists is taken."""
    for n, m in itertools.product((1, 2, 3, 5, 8), repeat=2):
        r = ref.dtw(np.ones((n, 2)), np.ones((m, 2)))
        i, j, back = n - 1, m - 1, []
        while True:
            back.append((i, j))
            if i == 0 and j == 0:
                break
            i, j = (i - 1, j - 1) if i and j else ((i - 1, j) if i else (i, j - 1))
        assert list(zip(r["path_a"], r["path_b"])) == back[::-1], (n, m)
        assert np.all(r["acc"] == 0) and r["length"] == max(n, m)
    # a three-way tie: c = [[1, 0], [0, 1]] gives D(0,0) = D(1,0) = D(0,1) = 1, and (1,1) takes the diagonal
    r = ref.dtw(np.array([[0.0], [1.0]]), np.array([[1.0], [0.0]]))
    assert list(zip(r["path_a"], r["path_b"])) == [(0, 0), (1, 1)] and r["cost"] == 2.0
    # a tie between the two edge moves alone goes to the source step (i-1, j): D(1,0) = D(0,1) = 1 < D(0,0) = 3
    everywhere = [[True, True], [True, True]]
    _, B = ref.accumulate([[3.0, -2.0], [-2.0, 0.0]], everywhere)
    assert B[1][1] == 1
    _, B = ref.accumulate([[3.0, -1.0], [-2.0, 0.0]], everywhere)  # D(1,0) = 1 < D(0,1) = 2: the target step (i, j-1)
    assert B[1][1] == 2


def test_band_leaves_no_cell_unreachable_and_holds_the_path():
    rng = np.random.RandomState(1)
    for n, m in itertools.product(range(1, 14), repeat=2):
        a = rng.randint(-3, 4, size=(n, 1)).astype(np.float64)
        b = rng.randint(-3, 4, size=(m, 1)).astype(np.float64)
        for radius in (1, 2, 3):
            band = ref.in_band(n, m, radius)
            assert band[0, 0] and band[-1, -1]
            r = ref.dtw(a, b, radius)
            assert np.array_equal(np.isfinite(r["acc"]), band), (n, m, radius)
            assert np.all(band[r["path_a"], r["path_b"]])
            assert ref.well_formed(r["path_a"], r["path_b"], n, m)
    assert np.all(ref.in_band(7, 4, None))
    # a band that holds everything changes nothing
    a, b = rng.randn(9, 3), rng.randn(6, 3)
    full, wide = ref.dtw(a, b), ref.dtw(a, b, 8)
    assert np.array_equal(full["acc"], wide["acc"]) and np.array_equal(full["path_a"], wide["path_a"])


def test_map_rule_on_a_hand_written_path():
    pa = np.array([0, 1, 2, 2, 2, 3, 4, 5])
    pb = np.array([0, 0, 0, 1, 2, 3, 3, 3])
    a2b, b2a = ref.maps(pa, pb, 6, 4)
    assert a2b.tolist() == [0, 0, 1, 3, 3, 3]  # row 2 pairs with columns 0..2: (0 + 2) // 2
    assert b2a.tolist() == [1, 2, 2, 4]        # column 0 pairs with rows 0..2, column 3 with rows 3..5
    # an even run takes the lower middle
    a2b, b2a = ref.maps(np.array([0, 0, 1]), np.array([0, 1, 2]), 2, 3)
    assert a2b.tolist() == [0, 2] and b2a.tolist() == [0, 0, 1]
