"""CPU: tests/_lsf_chain_reference.py, the NumPy statement of wh_lsf_repair / wh_lsf_distortion, against what it stands
for.  The repair equals world.lsf.repair_rows on CPU torch bit for bit on the whole case list (torch's clamp / maximum /
minimum are the contract's max / min).  The distortion's two sums are held to the bound its docstring derives, against
a long-double evaluation of the same double rows: the line spectral frequencies of every frame of the two committed
spectrogram fixtures at orders 2 / 24 / 40 / 64, each frame against the next one and against the frame half the
utterance away.  (The long double has 11 bits more: its own error is the same bound times 2^-11 and is added to it.)

Worst error / bound ratio seen (printed by every run):  s1 0.0088,  s2 0.0194 (both at p = 2; 0.0029 / 0.0051 at p = 24,
0.0028 / 0.0039 at p = 40, 0.0024 / 0.0038 at p = 64) — the bound adds up K worst cases of 4 p + 9 roundings each where
the roundings are of either sign and largely cancel, inside a product and again in the sum over the bins."""
import os

import numpy as np
import pytest

import _lsf_chain_cases as cc
import _lsf_chain_reference as cref
import _lsf_reference as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("golden_syn16k", "golden_syn48k")
ORDERS = (2, 24, 40, 64)


def fixture_cosines(name, p):
    """The cosines [F][p] of the reference's line spectral frequencies of a fixture's frames (flagged frames left out)."""
    spec = np.ascontiguousarray(np.load(os.path.join(GOLDEN, name + ".npz"))["ct_spectrogram"].T)
    a, _, _, bad = ref.levinson(ref.autocorr(spec, p), p)
    x, level = ref.lsf_from_lpc(a)
    return x[~bad & (level > 0)], spec.shape[1]


def test_repair_is_repair_rows_on_cpu_torch():
    import torch
    from world import lsf

    cases = cc.repair_cases() + tuple(cc.all_kinds_case(p) for p in cc.ORDERS)
    kinds_seen = set()
    for case in cases:
        w, kinds = cc.repair_rows_of(case)
        kinds_seen.update(kinds)
        want, changed = cc.repair_reference(case)
        got = lsf.repair_rows(torch, torch.from_numpy(np.array(w)), case.gap).numpy()
        assert cc.lc.same_bits(got, want), case.name
        assert np.array_equal(changed, np.sum(got.view(np.int64) != w.view(np.int64), axis=1)), case.name
        assert cc.lc.same_bits(want, ref.repair(w, case.gap)), case.name  # and the statement in tests/_lsf_reference.py
        assert case.gap < np.pi / (case.p + 2)
    assert kinds_seen == set(cc.ROW_KINDS)
    # a NaN spreads: forward from where it is, and back from the last angle once it got there
    case = cc.all_kinds_case(24)
    w, kinds = cc.repair_rows_of(case)
    out, changed = cc.repair_reference(case)
    for r, kind in enumerate(kinds):
        assert np.isnan(out[r]).all() == kind.startswith("nan"), kind
        if kind == "valid":
            assert changed[r] == 0 and out[r].tobytes() == w[r].tobytes()


@pytest.mark.parametrize("p", ORDERS)
def test_distortion_sums_against_long_double(p):
    worst = [0.0, 0.0]
    for name in FIXTURES:
        x, k_bins = fixture_cosines(name, p)
        assert len(x) > 20
        for shift in (1, len(x) // 2):
            xa, xb = x, np.roll(x, shift, axis=0)
            rows_a = np.concatenate([np.zeros((len(x), 1)), xa], axis=1)
            rows_b = np.concatenate([np.zeros((len(x), 1)), xb], axis=1)
            got = cref.distortion(rows_a, rows_b, k_bins)
            t = cref.log_ratio(xa, xb, k_bins, cref.LD)
            s1, s2 = np.sum(t, axis=1), np.sum(t * t, axis=1)
            b1, b2 = cref.sum_bounds(t, p)
            scale = 1.0 + 2.0 ** -11
            e1 = np.abs(got[:, 0].astype(cref.LD) - s1).astype(np.float64)
            e2 = np.abs(got[:, 1].astype(cref.LD) - s2).astype(np.float64)
            assert np.all(np.isfinite(got)) and np.all(e1 <= b1 * scale) and np.all(e2 <= b2 * scale), (name, shift)
            worst = [max(worst[0], float(np.max(e1 / b1))), max(worst[1], float(np.max(e2 / b2)))]
            # mutants on side a only: u and v swapped; the factor 0.25 left out
            for mutant in ("swapped", "no_quarter"):
                bad = cref.distortion(rows_a, rows_b, k_bins, mutant=mutant)
                m1 = np.abs(bad[:, 0].astype(cref.LD) - s1).astype(np.float64)
                m2 = np.abs(bad[:, 1].astype(cref.LD) - s2).astype(np.float64)
                assert np.all(m1 > 1e6 * b1) and np.all(m2 > 1e6 * b2), (name, shift, mutant)
    print("p = %d: worst error / bound  s1 %.4f  s2 %.4f" % (p, worst[0], worst[1]))


def test_identical_rows_and_bad_indices():
    x, k_bins = fixture_cosines(FIXTURES[0], 24)
    rows = np.concatenate([np.full((len(x), 1), np.nan), x], axis=1)[:16]
    out = cref.distortion(rows, rows, k_bins)
    assert np.all(out == 0.0)
    idx_a = np.array([0, 5, 16, -1, 3], dtype=np.int64)
    out = cref.distortion(rows, rows[::-1], k_bins, idx_a, np.array([0, 5, 1, 1, 16], dtype=np.int64))
    assert np.isfinite(out[:2]).all() and np.isnan(out[2:]).all()
    # the order bound is not looser than the truth bound's share that it covers, and is zero where t is
    t = cref.log_ratio(rows[:4, 1:], rows[:4, 1:], k_bins)
    assert np.all(np.array(cref.order_bounds(t)) == 0.0)
