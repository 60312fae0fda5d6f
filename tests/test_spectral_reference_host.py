"""CPU: tests/_spectral_reference.py against the oracle, and its comparators against deliberate mistakes — the references the
GPU tests of the rank selection and the spectral helpers rest on must be right, and must be able to say no, before a
kernel is judged by them."""
import numpy as np
import pytest

import _spectral_reference as S
from oracle import common as OC

PAIRS = ((16000, 512), (22050, 1024), (48000, 2048))


def _benign(n, seed, rows=4):
    return np.random.RandomState(seed).uniform(0.5, 1.5, (rows, n // 2 + 1))


@pytest.mark.parametrize("fs,n", PAIRS)
def test_windowed_sum_identity_is_the_oracles_cumsum_smoothing(fs, n):
    p = _benign(n, n)
    for half in (150.0 / 3, 333.3 / 3, 47.0 / 2, 800.0 / 4):
        oracle = OC.cumsum_band_mean(OC.mirror_half(p), fs, n, np.full(len(p), 2 * half))
        consts = S.band_constants(n, fs, half)
        for row in range(len(p)):
            ref = S.band_reference(S.mirrored(p[row], n, fs), n, consts)
            assert np.max(np.abs(oracle[row] - ref)) <= 1e-12 * np.max(np.abs(ref)), (half, row)


@pytest.mark.parametrize("fs,n", PAIRS)
def test_replica_reference_is_the_oracles(fs, n):
    p = _benign(n, n + 1)
    df = fs / n
    for f0 in (47.0, 71.0, 150.0, 333.3, 800.0, 10 * df):
        for reach in (f0 + df, 1.2 * f0):
            oracle = OC.low_band_replica(OC.mirror_half(p), fs, n, np.full(len(p), f0), np.full(len(p), reach))[:, :n // 2 + 1]
            for row in range(len(p)):
                for cap in (n, n // 2 + 1):
                    ref, touched, bound = S.replica_reference(p[row], n, fs, f0, reach, cap)
                    assert touched.any() and not touched[int(f0 / df) + 1:].any()
                    assert np.max(np.abs(ref - oracle[row])) <= 1e-12 * np.max(np.abs(ref)), (f0, reach, row)
                    assert S.replica_failures(ref.astype(np.float64), p[row], ref, touched, bound) == []


def test_band_constants_at_dyadic_spacings_are_exact():
    for fs, n in ((8000, 512), (16000, 1024), (16000, 2048), (48000, 4096), (96000, 8192)):
        df = fs / n
        for j in (1, 2, 3, 4, 7, 8, 41, 64, n // 2 + 3, n // 2 + 4):
            b_lo, b_hi, f_lo, f_hi = S.band_constants(n, fs, j * df / 2)
            assert f_lo == f_hi == (0.0 if j % 2 else 0.5) and b_hi - b_lo == j, (fs, n, j)
    assert S.band_constants(512, 8000, 0.0)[1] == S.band_constants(512, 8000, 0.0)[0]  # the smallest window: no whole bin


def test_integer_smoothing_reference_is_the_identity():
    fs, n = 16000, 1024
    p = np.random.RandomState(3).randint(0, 1000, n // 2 + 1)
    for j in (1, 2, 5, n // 2 + 3):
        half = j * (fs / n) / 2
        ints = S.band_integer_reference(p, n, fs, half)
        ref = S.band_reference(S.mirrored(p.astype(np.float64), n, fs), n, S.band_constants(n, fs, half))
        assert np.array_equal(ints, ref), j


# ---- the comparators say no ---------------------------------------------------------------------------------------------
def _selection_of(row, drop, off_by=0, swap=False):
    """What a selection would return that leaves out the `drop + off_by` largest (swap: the member just BELOW the threshold
    instead of the one just above it)."""
    s = np.sort(row)
    keep = list(s[:len(s) - drop - off_by])
    if swap:
        keep[-1] = s[len(s) - drop]
    return [float(np.sum(np.array(keep, dtype=np.longdouble))), float(np.sum(s.astype(np.longdouble)))]


@pytest.mark.parametrize("exact", [True, False])
def test_selection_comparator_rejects_a_wrong_member_and_one_drop_too_many(exact):
    rng = np.random.RandomState(11)
    k, drop = 1025, 22
    if exact:
        rows = (2.0 ** 20 + rng.permutation(k)).reshape(1, k)  # one exponent bin, no ties
    else:
        rows = (rng.chisquare(2, k) / (1.0 + np.arange(k)) ** 2).reshape(1, k)  # speech-like: the large bins share octaves
        top = np.sort(rows[0])[-drop - 2:]
        assert np.floor(np.log2(top[1])) == np.floor(np.log2(top[2])) and top[1] != top[2]  # a tie-free threshold bin
    m = k - drop
    assert S.selection_failures([_selection_of(rows[0], drop)], rows, m, exact) == []
    wrong = S.selection_failures([_selection_of(rows[0], drop, swap=True)], rows, m, exact)
    assert [w[:2] for w in wrong] == [(0, "small")]
    more = S.selection_failures([_selection_of(rows[0], drop, off_by=1)], rows, m, exact)
    assert [w[:2] for w in more] == [(0, "small")]
    assert S.selection_failures([[float("nan"), 0.0]], rows, m, exact) != []


def test_selection_reference_counts_ties_once():
    row = np.array([3.0] * 7 + [1.0, 2.0])
    assert S.select_reference(row, 5, integer=True) == (1 + 2 + 3 * 3, 24)
    assert S.selection_failures([[12.0, 24.0]], row.reshape(1, -1), 5, True) == []
    assert S.selection_failures([[15.0, 24.0]], row.reshape(1, -1), 5, True) != []  # a tie dropped one time too few
    assert S.selection_failures([[9.0, 24.0]], row.reshape(1, -1), 5, True) != []   # ... and one too many


def test_smoothing_comparator_rejects_an_edge_off_by_one_and_swapped_fractions():
    fs, n, kr = 22050, 1024, 5
    p = _benign(n, 5, rows=1)[0]
    v = S.mirrored(p, n, fs)
    consts = S.band_constants(n, fs, 150.0 / 3)
    b_lo, b_hi, f_lo, f_hi = consts
    assert abs(f_lo - f_hi) > 0.05
    ref = S.band_reference(v, n, consts)
    bound, _ = S.band_bound(v, n, consts, kr)
    assert S.band_failures(ref, ref, bound) == []
    assert S.band_failures(ref + 0.5 * bound, ref, bound) == []
    assert len(S.band_failures(ref + 1.5 * bound, ref, bound)) == n // 2 + 1
    assert len(S.band_failures(S.band_reference(v, n, (b_lo, b_hi + 1, f_lo, f_hi)), ref, bound)) == n // 2 + 1
    assert len(S.band_failures(S.band_reference(v, n, (b_lo, b_hi, f_hi, f_lo)), ref, bound)) == n // 2 + 1
    nan = ref.copy()
    nan[7] = np.nan
    assert S.band_failures(nan, ref, bound) == [7]


def test_smoothing_bound_follows_what_a_run_has_touched():
    fs, n, kr = 16000, 1024, 5
    consts = S.band_constants(n, fs, 40.0 / 3)
    p = np.ones(n // 2 + 1)
    p[203] = 1e12
    v = S.mirrored(p, n, fs)
    bound, big = S.band_bound(v, n, consts, kr)
    start, length = S.run_touched(n, consts, kr)
    for k in range(195, 215):
        touched = {(int(start[k]) + i) % n for i in range(int(length[k]))}
        assert (big[k] > 1e11) == (203 in touched), k
    # the run [200, 205) has met the peak by its last bin and carries it from there on; its neighbours never read bin 203
    assert big[204] > 1e11 > big[205] and big[199] < 1e11


def test_growing_one_element_is_the_reference_of_the_grown_spectrum():
    fs, n = 22050, 1024
    p = _benign(n, 13, rows=1)[0]
    ks = np.arange(n // 2 + 1)
    for half in (40.0 / 3, 150.0 / 3, 800.0 / 2):  # W = 1, 4 and 37
        consts = S.band_constants(n, fs, half)
        v = S.mirrored(p, n, fs)
        base = S.band_reference(v, n, consts)
        for j in (0, 5, 300, 512, 1019):
            grown = v.copy()
            grown[j] = 1e12 * fs / n
            ref = S.band_reference(grown, n, consts)
            got = S.band_add_peak(base.astype(S.LD), ks, n, consts, j, S.LD(grown[j]) - S.LD(v[j]))
            changed = np.nonzero(ref != base)[0]
            assert j not in (5, 300) or len(changed) >= 1  # (the others sit at the edges of the half: few bins or none reach them)
            assert np.max(np.abs(got - ref.astype(S.LD)) / np.abs(ref)) < 2.0 ** -51, (half, j)
            assert np.array_equal(got[ref == base].astype(np.float64), base[ref == base])


def test_replica_comparator_rejects_less_or_equal_at_a_bin_on_f0():
    fs, n = 16000, 1024
    p = _benign(n, 9, rows=1)[0]
    f0 = 12 * fs / n  # bin 12 lies ON f0: it is not below it
    for cap in (n, n // 2 + 1):
        ref, touched, bound = S.replica_reference(p, n, fs, f0, f0 + fs / n, cap)
        assert touched[:12].all() and not touched[12:].any()
        wrong, _, _ = S.replica_reference(p, n, fs, f0, f0 + fs / n, cap, less=np.less_equal)
        assert S.replica_failures(ref.astype(np.float64), p, ref, touched, bound) == []
        assert S.replica_failures(wrong.astype(np.float64), p, ref, touched, bound) == [12]
    # below one bin spacing there are fewer than two nodes: nothing is touched
    ref, touched, bound = S.replica_reference(p, n, fs, 0.4 * fs / n, 0.9 * fs / n, n)
    assert not touched.any() and np.array_equal(ref.astype(np.float64), p)


def test_boundaries_of_the_band_stage():
    # d4c_launch_const's expression at d4c()'s transform lengths: int(N / wlen * 8 + 0.5), wlen = 2 floor(interval N / fs) + 1
    assert [S.d4c_fft_size(fs) for fs in (8000, 16000, 22050, 32000, 48000, 96000)] == [1024, 2048, 2048, 4096, 4096, 8192]
    assert [S.d4c_boundary(fs) for fs in (8000, 16000, 22050, 32000, 48000, 96000)] == [16, 21, 29, 43, 64, 128]
