"""CPU: tests/_psola_reference.py, the NumPy statement of wh_psola's contract, checked on its own — against the same
contract as scalar loops on tiny inputs, against nine mutants that must each be told apart on the case list of
tests/_psola_cases.py, and by its properties: identity (the target equal to the analysis track returns the recording),
the bound of the normalised output, the capacities on random and illegal tracks, and the pitch of a pulse train.

All nine are told apart by the outputs.  A mark depends on a score's last bits only at a near tie, so the pairwise sum
shows on the one case built for it ("near ties": candidates whose scores are equal in real arithmetic and differ by the
rounding of their sums); the fused sum also shows in y, whose accumulation is part of the contract.  Both sum mutants are
checked on the bits of a case's scores as well."""
import numpy as np
import pytest

import _psola_cases as pc
import _psola_reference as pref
import _wsola_reference as wref

P = pref.Params
TINY = tuple(
    pc.Case("tiny %d" % i, params, utts, 900 + i) for i, (params, utts) in enumerate((
        (P(4, 10, 5, 2, 1, 1), (("tone", 120, 1.25, ("runs", ((0, 9, 20, 31), 4)), ("runs", ((0, 7, 25), 4)), ("ratio", None)),
                                ("noise", 60, 0.5, ("runs", ((0, 9), 3)), ("const", 12), ("wild", None)))),
        (P(1, 3, 2, 2, 1, 0), (("noise", 40, 2.0, ("runs", ((0, 5, 8), 6)), ("runs", ((0, 4, 9), 6)), ("ratio", None)),
                               ("periodic", 50, 50, ("const", 10), ("const", 8), ("down", None)))),
        (P(16, 7, 3, 4, 6, 1), (("nan", 70, 70, ("hostile", None), ("hostile", None), ("far", None)),
                                ("inf", 45, 1.25, ("const", 12), ("const", 4), ("ratio", None)),
                                ("noise", 0, 9, ("const", 0), ("const", 0), ("wild", None)),
                                ("noise", 1, 0, ("const", 5), ("const", 5), ("ratio", None)))),
        (P(3, 4, 0, 2, 1, 1), (("periodic", 64, 2.0, ("const", 0), ("const", 0), ("ratio", None)),
                               ("silence", 30, 30, ("const", 6), ("const", 5), ("ratio", None)))),
    )))


def _run(case, u, mutant=None):
    inp = pc.inputs(case)
    return pref.psola(inp["x"][u], inp["n_out"][u], inp["per_a"][u], inp["per_s"][u], inp["src"][u], case.params, mutant)


def _same(a, b):
    return all((pc.same_bits(a[k], b[k]) if k == "y" else a[k].tobytes() == b[k].tobytes()) for k in pc.FIELDS)


def test_vector_form_equals_the_scalar_loops():
    for case in TINY:
        inp = pc.inputs(case)
        for u in range(len(case.utts)):
            want = pref.psola_scalar(inp["x"][u], inp["n_out"][u], inp["per_a"][u], inp["per_s"][u], inp["src"][u], case.params)
            got = _run(case, u)
            for k in pc.FIELDS:
                assert got[k].dtype == want[k].dtype and len(got[k]) == len(want[k]), (case.name, u, k)
            assert _same(got, want), (case.name, u)


# the cases of the list on which each mutant is looked for, the cheapest first
WHERE = {
    "fused_sum": ("P=65 tol=15",), "pairwise_sum": ("near ties: the order of the sums decides",),
    "ties_lowest_index": ("periodic integers: exact ties",), "no_terminal_mark": ("P=65 tol=15",),
    "running_pointer": ("src decreasing",), "hanning_window": ("P=65 tol=15",), "step_from_q": ("norm 0", "mixed periods"),
    "clipped_read": ("P=65 tol=15", "src out of range"), "flip_dropped": ("stretch 0.5 and 2",),
}


def test_every_mutant_is_told_apart_on_the_case_list():
    by_name = {c.name: c for c in pc.all_cases()}
    assert set(pref.MUTANTS) == set(WHERE)
    for mutant, names in WHERE.items():
        differs = any(not _same(_run(by_name[name], u, mutant), pc.reference(by_name[name])[u])
                      for name in names for u in range(len(by_name[name].utts)))
        assert differs, mutant
    want = pc.reference(by_name["near ties: the order of the sums decides"])[0]["marks"]
    got = _run(by_name["near ties: the order of the sums decides"], 0, "pairwise_sum")["marks"]
    assert want[1] != got[1] and want[1] >= 64 and got[1] >= 64  # (mark 1 itself moves, among the candidates d >= 0)
    # the order of the sums again, by the scores of the first mark of a case: template and region as stage A stages them
    case = by_name["P=255"]
    x, period, tol = pc.inputs(case)["x"][0], 255, min(case.params.tol, 255 // 4)
    t, region = wref.read(x, -(period // 2), period), wref.read(x, period - tol - period // 2, period + 2 * tol)
    want = wref.scores(t, region, tol)
    for mutant in ("pairwise_sum", "fused_sum"):
        got = wref.scores(t, region, tol, mutant)
        assert np.allclose(got, want, rtol=1e-12, atol=1e-14) and got.tobytes() != want.tobytes(), mutant


def _identity_input(kind, n, grid, seed):
    rng = np.random.RandomState(seed)
    x = pc.wc.signal(kind, n, rng)
    per = pc.period_track(("runs", ((0, 57, 64, 71, 80, 80), 12)), n // grid + 1, rng)
    return x, per, np.arange(n // grid + 1, dtype=np.int64) * grid


def test_identity_returns_the_recording():
    """per_s == per_a, src[k] = k G, n_out == n: sel == arange, s == a, and y == x up to the rounding of a two-term sample.
    The bound: a half window is five rounded operations (the divide, u u, 3 - 2 u — whose result lies in [1, 3], so its
    half ulp is 2 eps —, the product and the difference from 1) and the derivative of the cubic is at most 1.5, so each of
    the two weights is within 1.5 eps / 2 + eps / 2 + 2 eps + eps / 2 + eps / 2 = 4.25 eps of its exact value and their sum
    within 8.5 eps of 1 (eps = 2^-53); the two products and their sum add 2 eps, the sum of the weights and the divide by
    max(W, 1) one eps each: |y - x| <= 12.5 eps max|x|, asserted as 16 eps max|x|."""
    p = P(16, 80, 50, 2, 1, 1)
    for kind, n, seed in (("tone", 6000, 1), ("noise", 3000, 2)):
        x, per, src = _identity_input(kind, n, p.grid, seed)
        r = pref.psola(x, n, per, per, src, p)
        assert np.array_equal(r["sel"], np.arange(len(r["marks"]))) and np.array_equal(r["smarks"], r["marks"]) and not np.any(r["flip"])
        worst = float(np.max(np.abs(r["y"] - x)))
        print("psola reference, identity on %s: %d marks, worst |y - x| = %.3g at max|x| = %.3g" % (kind, len(r["marks"]), worst, np.max(np.abs(x))))
        assert worst <= 16 * 2.0 ** -53 * np.max(np.abs(x)), kind


def test_normalised_output_is_bounded_by_the_input():
    """With norm, y[t] = sum w v / max(sum w, 1) is a convex combination scaled down: |y| <= max|x| up to rounding.  For n
    grains on a sample the recursive sum of the n rounded products is within n eps of its exact value relative to
    sum w |v| <= W max|x|, the sum of the weights within (n - 1) eps of W, the divide adds one: |y| <= max|x| (1 + (2 n + 4) eps)
    with room for the second-order terms — a few ulp where two grains overlap; n is counted per utterance."""
    eps = 2.0 ** -53
    for case in pc.all_cases():
        if not case.params.norm or any(u[0] in ("nan", "inf") for u in case.utts):
            continue
        for u, r in enumerate(pc.reference(case)):
            x, n_out = pc.inputs(case)["x"][u], pc.inputs(case)["n_out"][u]
            cover = np.zeros(n_out + 1, dtype=np.int64)
            for j in range(len(r["smarks"])):
                left, right = pref.widths(r["marks"], r["periods"], int(r["sel"][j]), case.params.hop)
                lo, hi = max(0, int(r["smarks"][j]) - left + 1), min(n_out, int(r["smarks"][j]) + right)
                if hi > lo:
                    cover[lo] += 1
                    cover[hi] -= 1
            n = int(np.max(np.cumsum(cover), initial=0))
            peak = float(np.max(np.abs(x))) if len(x) else 0.0
            assert np.all(np.abs(r["y"]) <= peak * (1 + (2 * n + 4) * eps)), (case.name, u, n)


def test_capacities_hold_on_random_and_illegal_tracks():
    rng = np.random.RandomState(5)
    for trial in range(60):
        p = P(int(rng.choice([1, 3, 16, 50])), int(rng.choice([1, 4, 30])), int(rng.choice([0, 1, 6, 40])), int(rng.choice([2, 3, 9, 30])),
              int(rng.choice([1, 2, 25])), int(trial % 2))
        n, n_out = int(rng.randint(0, 400)), int(rng.randint(0, 400))
        x = rng.randn(n)
        kind = ("hostile", None) if trial % 3 else ("runs", ((0, 2, 3, 9, 30, 64), 3))
        per_a, per_s = pc.period_track(kind, n // p.grid + 1, rng), pc.period_track(kind, n_out // p.grid + 1, rng)
        src = pc.source_track(("far" if trial % 4 == 0 else "wild", None), n_out // p.grid + 1, n, n_out, p.grid, rng)
        r = pref.psola(x, n_out, per_a, per_s, src, p)
        assert len(r["marks"]) <= pref.mark_capacity(n, p) and len(r["smarks"]) <= pref.smark_capacity(n_out, p), (trial, p)
        assert np.all(np.diff(r["marks"]) >= pref.min_step(p)) and np.all(np.diff(r["smarks"]) >= min(p.hop, p.smin))
        assert (len(r["marks"]) == 0) == (n == 0) and (n == 0 or (r["marks"][-1] >= n and np.all(r["marks"][:-1] < n)))
        assert np.all((r["periods"] == 0) | ((r["periods"] >= p.pmin) & (r["periods"] <= pref.PMAX)))
        if len(r["sel"]):
            assert r["sel"].min() >= 0 and r["sel"].max() < len(r["marks"]) and r["smarks"][-1] >= n_out


def test_a_pulse_train_takes_the_target_period():
    n, p = 128 * 40, P(16, 80, 20, 2, 1, 1)
    x = np.zeros(n)
    x[::128] = 1.0
    k = n // p.grid + 1
    r = pref.psola(x, n, np.full(k, 128, dtype=np.int32), np.full(k, 100, dtype=np.int32), np.arange(k, dtype=np.int64) * p.grid, p)
    assert np.all(np.diff(r["marks"]) == 128) and np.all(np.diff(r["smarks"]) == 100)
    y = r["y"][500:-500]
    ac = np.array([np.dot(y[:-lag], y[lag:]) for lag in range(20, 300)])
    assert 20 + int(np.argmax(ac)) == 100


def test_the_case_list_reaches_what_it_claims():
    by_name = {c.name: c for c in pc.all_cases()}
    used = set()
    for case in pc.period_cases():
        for r in pc.reference(case):
            used |= set(r["periods"].tolist())
    assert set(pc.PERIODS) <= used
    r = pc.reference(by_name["P=2048 tol=512"])[0]
    assert len(r["marks"]) >= 4 and np.any(np.abs(np.diff(r["marks"])[:-1] - 2048) > 256)  # a winner beyond the fourth thread slot
    r = pc.reference(by_name["stretch 0.5 and 2"])
    assert np.any(r[1]["flip"]) or np.any(r[2]["flip"])
    assert np.any(np.diff(r[0]["sel"]) > 1) and np.any(np.diff(r[1]["sel"]) == 0)
    assert len(set(pc.reference(by_name["constant src"])[0]["sel"].tolist())) == 1
    assert np.any(np.diff(pc.reference(by_name["src decreasing"])[0]["sel"]) < 0)
    for y in (pc.reference(by_name["digital silence"])[0]["y"],):
        assert not np.any(y)
    assert np.any(pc.reference(by_name["target 2048 against analysis 20"])[0]["y"] == 0.0)  # gaps between the grains
    r = pc.reference(by_name["pmin makes entries unvoiced"])[0]
    assert 40 in pc.inputs(by_name["pmin makes entries unvoiced"])["per_a"][0] and 40 not in r["periods"]
    assert np.all(np.diff(pc.reference(by_name["smin binds"])[0]["smarks"]) == 90)
