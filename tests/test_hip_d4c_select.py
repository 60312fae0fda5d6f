"""GPU: D4C's rank selection (sum_smallest, csrc/wh_d4c_select.h) on its own, through wh_d4c_select_probe, with the template
arguments of every d4c_kernel instance (n = 512 ... 8192: K = 257 ... 4097 values on 256 / 128 / 256 / 512 / 512 threads in
2 / 6 / 6 / 6 / 10 slots) and two assignments of the values to threads, against sort-and-sum (tests/_spectral_reference.py).

The selection leaves out the drop = K - m largest values by counting exponents (4 per round, per wave, merged across waves
whose maxima differ), refining the threshold bin by mantissa digits while it holds more than 32 members, and ranking what
is left with a tie rule.  Speech takes one path through that (one round, ~11 members); a selection that is wrong by one
member of the threshold bin moves a band aperiodicity by 1e-3 dB at most, which no pipeline test sees.  Here it is either
exact or wrong:

  bit for bit   integer-valued doubles below 2^39: every order of summation is exact, so s_small and s_total must BE the
                integer sums — exponents over 39 octaves (ten rounds), all values equal (every refinement level, a ranking
                of ties alone), 2^20 + a permutation (one exponent bin, refinement down to the last mantissa digit), two
                values with the threshold inside the run of equal large ones, K - 5 zeros, all zeros, the large values in
                the first / the last wave or in one thread's slots with everything else 30 octaves below;
  60 octaves    the same wave cases with the other waves 60 octaves below (2^60 (1 + j 2^-15) against 1 ... 15): such sums
                do not fit 53 bits, so s_small is exact only where nothing large is kept (drop >= the number of large values)
                and is held to the bound below otherwise — a wrong member there is off by 2^45 at least, the bound is below 2^30;
  within bound  values over 600 decades, denormals among normals, a speech-like draw: (K - 1) 2^-53 times the reference, the
                worst case of summing K non-negative terms in any order (derived in tests/_spectral_reference.py).

drop: 1, 2, 32, 33, K / 2, K - 1 and the band stage's own boundary + 1 at 8, 16, 22.05, 32, 48 and 96 kHz, one launch each
on the same uploaded rows."""
import itertools
import math

import numpy as np
import pytest

import _spectral_reference as S

pytestmark = pytest.mark.gpu

FT = S.D4C_FT  # ft_of(n), csrc/wh_d4c_types.h
SLOTS = {512: 2, 1024: 6, 2048: 6, 4096: 6, 8192: 10}
RATES = (8000, 16000, 22050, 32000, 48000, 96000)
EXACT = ("octaves", "all_equal", "permutation", "two_valued", "five_positive", "zeros", "first_wave_30", "last_wave_30",
         "one_thread")
WAVE60 = ("first_wave_60", "last_wave_60")
BOUND = ("decades", "denormals", "speech")


def drops(k):
    d = {1, 2, 32, 33, k // 2, k - 1} | {S.d4c_boundary(fs) + 1 for fs in RATES}
    return sorted(v for v in d if 1 <= v <= k - 1)


def owners(n, layout):
    """thread and slot of every bin, as d4c_select_probe_kernel assigns them (layout 0: the band stage's own)."""
    k_bins, ft, mb = n // 2 + 1, FT[n], n // 2
    thread, slot = np.full(k_bins, -1), np.full(k_bins, -1)
    if layout == 0:
        for k in range(mb // 2 + 1):
            thread[k], slot[k] = k % ft, 2 * (k // ft)
            if k != mb - k:
                thread[mb - k], slot[mb - k] = k % ft, 2 * (k // ft) + 1
    else:
        k = np.arange(k_bins)
        thread = (k_bins - 1 - k) % ft
        slot = (k - (k_bins - 1 - thread) % ft) // ft
    assert thread.min() >= 0 and slot.min() >= 0 and slot.max() <= SLOTS[n] - 1
    assert len(set(zip(thread.tolist(), slot.tolist()))) == k_bins
    return thread, slot


def _rows(n, layout, kind):
    """(rows (count, K), number of large values per row or None)"""
    k = n // 2 + 1
    rng = np.random.RandomState(n + 7 * len(kind) + ord(kind[0]))
    thread, _ = owners(n, layout)
    wave = thread // 64
    if kind == "octaves":
        return np.floor(2.0 ** rng.uniform(0.0, 39.0, (64, k))), None
    if kind == "all_equal":
        return np.full((2, k), 3.0), None
    if kind == "permutation":
        return np.stack([2.0 ** 20 + rng.permutation(k) for _ in range(4)]), None
    if kind == "two_valued":
        counts = sorted({c for d in drops(k) for c in (d + 1, d + 7) if c < k} | {2, k - 1})
        rows = np.full((len(counts), k), 3.0)
        for r, c in enumerate(counts):
            rows[r, rng.permutation(k)[:c]] = 2.0 ** 30 + 1
        return rows, None
    if kind == "five_positive":
        rows = np.zeros((4, k))
        for r in range(4):
            rows[r, rng.permutation(k)[:5]] = [1.0, 2.0, 3.0, 2.0 ** 38 - 1, 7.0]
        return rows, None
    if kind == "zeros":
        return np.zeros((2, k)), None
    if kind in ("first_wave_30", "last_wave_30", "first_wave_60", "last_wave_60"):
        w = 0 if kind.startswith("first") else int(wave.max())
        inside = np.nonzero(wave == w)[0]
        rows = rng.randint(1, 16, (4, k)).astype(np.float64)
        for r in range(4):
            j = rng.permutation(k)[:len(inside)]
            rows[r, inside] = 2.0 ** 32 + j if kind.endswith("30") else 2.0 ** 60 + j * 2.0 ** 45
        return rows, len(inside)
    if kind == "one_thread":
        owning = np.unique(thread)
        picks = [int(owning[0]), int(owning[len(owning) // 2]), int(owning[-1])]
        rows = rng.randint(1, 16, (len(picks), k)).astype(np.float64)
        for r, t in enumerate(picks):
            mine = np.nonzero(thread == t)[0]
            rows[r, mine] = 2.0 ** 32 + rng.permutation(k)[:len(mine)]
        return rows, None
    if kind == "decades":
        return 10.0 ** rng.uniform(-300.0, 300.0, (16, k)), None
    if kind == "denormals":
        rows = 10.0 ** rng.uniform(-320.0, -300.0, (16, k))  # denormal below 2.2e-308
        rows[8:] = np.where(rng.uniform(size=(8, k)) < 0.5, rows[8:], rng.uniform(0.0, 1.0, (8, k)))
        assert (rows[:8] < 2.2e-308).any() and (rows[:8] > 2.3e-308).any()
        return rows, None
    assert kind == "speech"
    return rng.chisquare(2, (16, k)) / (1.0 + np.arange(k)) ** 2, None  # powers under a 1/f^2 envelope


_cache = {}


def _case(n, layout, kind):
    """rows, their device copy and the sorted rows' running sums, shared by every drop (and by both layouts where the rows do
    not depend on the assignment)."""
    key = (n, kind, layout if kind in WAVE60 + ("first_wave_30", "last_wave_30", "one_thread") else 0)
    if key not in _cache:
        rows, n_large = _rows(n, layout, kind)
        assert rows.min() >= 0.0 and np.all(np.isfinite(rows))
        srt = np.sort(rows, axis=1)
        ints = None
        if kind in EXACT:
            assert np.all(rows == np.floor(rows)) and rows.max() < 2.0 ** 39
            ints = [[0] + list(itertools.accumulate(int(v) for v in r)) for r in srt]
        _cache[key] = (rows, _to_device(rows), srt, ints, n_large)
    return _cache[key]


def _to_device(rows):
    from world import _hip

    return _hip.Runtime.get().to_device(rows.reshape(-1))


def _select(n, layout, m, rows_d, count):
    from world import _hip

    rt = _hip.Runtime.get()
    out = rt.empty((count * 2,))
    out.fill_(float("nan"))
    _hip.check(rt.lib.wh_d4c_select_probe(rt.ctx, rt.stream(), n, layout, m, rt.ptr(rows_d), rt.ptr(out), count))
    return out.cpu().numpy().reshape(count, 2)


CASES = [(n, layout) for n in sorted(FT) for layout in (0, 1)]


@pytest.mark.parametrize("kind", EXACT)
@pytest.mark.parametrize("n,layout", CASES)
def test_integer_sums_bit_for_bit(n, layout, kind):
    k = n // 2 + 1
    rows, rows_d, _, ints, _ = _case(n, layout, kind)
    bad = []
    for drop in drops(k):
        got = _select(n, layout, k - drop, rows_d, len(rows))
        for r in range(len(rows)):
            want = (float(ints[r][k - drop]), float(ints[r][k]))
            if tuple(got[r]) != want:
                bad.append((drop, r, tuple(got[r]), want))
    assert not bad, "%d wrong (drop, row, got, want): %r" % (len(bad), bad[:6])


@pytest.mark.parametrize("kind", WAVE60)
@pytest.mark.parametrize("n,layout", CASES)
def test_waves_sixty_octaves_apart(n, layout, kind):
    k = n // 2 + 1
    rows, rows_d, srt, _, n_large = _case(n, layout, kind)
    assert 1 <= n_large < k
    bad = []
    for drop in drops(k):
        got = _select(n, layout, k - drop, rows_d, len(rows))
        for r in range(len(rows)):
            small, total = math.fsum(srt[r, :k - drop]), math.fsum(srt[r])
            if drop >= n_large:  # only the small integers are kept: their sum is exact in any order
                ok = got[r, 0] == small and small == float(sum(int(v) for v in srt[r, :k - drop]))
            else:
                ok = abs(S.LD(got[r, 0]) - S.LD(small)) <= S.LD(S.select_bound(k, small))
            ok = ok and abs(S.LD(got[r, 1]) - S.LD(total)) <= S.LD(S.select_bound(k, total))
            if not ok:
                bad.append((drop, r, tuple(got[r]), (small, total)))
    assert not bad, "%d wrong (drop, row, got, want): %r" % (len(bad), bad[:6])


@pytest.mark.parametrize("kind", BOUND)
@pytest.mark.parametrize("n,layout", CASES)
def test_float_sums_within_the_summation_bound(n, layout, kind):
    k = n // 2 + 1
    rows, rows_d, srt, _, _ = _case(n, layout, kind)
    bad, worst = [], 0.0
    for drop in drops(k):
        got = _select(n, layout, k - drop, rows_d, len(rows))
        for r in range(len(rows)):
            for j, ref in enumerate((math.fsum(srt[r, :k - drop]), math.fsum(srt[r]))):
                err, bound = abs(S.LD(got[r, j]) - S.LD(ref)), S.LD(S.select_bound(k, ref))
                worst = max(worst, float(err / bound)) if bound > 0 else worst
                if not (math.isfinite(got[r, j]) and err <= bound):
                    bad.append((drop, r, j, float(got[r, j]), ref))
    print("n %d layout %d %-9s worst error / bound %.3e" % (n, layout, kind, worst))
    assert not bad, "%d beyond (K - 1) 2^-53 (drop, row, which, got, want): %r" % (len(bad), bad[:6])


def test_the_comparator_and_the_probe_agree_on_a_plain_case():
    """S.selection_failures, the comparator the host test exercises, on the probe's output."""
    n, k = 2048, 1025
    rows, rows_d, _, _, _ = _case(n, 0, "permutation")
    assert S.selection_failures(_select(n, 0, k - 22, rows_d, len(rows)), rows, k - 22, True) == []
    rows, rows_d, _, _, _ = _case(n, 0, "speech")
    assert S.selection_failures(_select(n, 1, k - 22, rows_d, len(rows)), rows, k - 22, False) == []


def test_bad_arguments_are_refused():
    from world import _hip

    rt = _hip.Runtime.get()
    buf, res = rt.zeros((4097,)), rt.zeros((2,))
    p, o, st, probe = rt.ptr(buf), rt.ptr(res), rt.stream(), rt.lib.wh_d4c_select_probe
    assert probe(rt.ctx, st, 512, 0, 200, p, o, 1) == 0
    assert probe(None, st, 512, 0, 200, p, o, 1) != 0
    assert probe(rt.ctx, st, 512, 0, 200, None, o, 1) != 0
    assert probe(rt.ctx, st, 512, 0, 200, p, None, 1) != 0
    assert probe(rt.ctx, st, 768, 0, 200, p, o, 1) != 0     # not a transform length of D4C
    assert probe(rt.ctx, st, 512, 2, 200, p, o, 1) != 0     # no such layout
    assert probe(rt.ctx, st, 512, 0, 0, p, o, 1) != 0       # m = 0: nothing kept
    assert probe(rt.ctx, st, 512, 0, 257, p, o, 1) != 0     # m = K: nothing left out
    assert probe(rt.ctx, st, 512, 0, 200, p, o, -1) != 0
    assert probe(rt.ctx, st, 512, 0, 200, p, o, 0) == 0
