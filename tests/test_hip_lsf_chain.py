"""GPU: wh_lsf_repair and wh_lsf_distortion (csrc/wh_lsf_chain.hip) through the C ABI and through world.lsf, against
tests/_lsf_chain_reference.py: the repair bit for bit — there is no tolerance on it —, the distortion's two sums within
the bound between two evaluations that share the quotient's bits and differ in the logarithm's last place and the order
of the sums (order_bounds in the reference's docstring).

Worst error / bound ratio of the distortion seen on an MI355X over the case list: 0.011 (printed by every run,
test_distortion_matches_the_reference)."""
import ctypes

import numpy as np
import pytest

import _lsf_cases as lc
import _lsf_chain_cases as cc
import _lsf_chain_reference as cref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    from world import _hip
    return _hip.Runtime.get()


# ---- repair ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cc.repair_cases(), ids=lambda c: c.name)
def test_repair_matches_the_reference_bit_for_bit(rt, case):
    w, _ = cc.repair_rows_of(case)
    want, changed = cc.repair_reference(case)
    gap, hi = cref.gap_hi(case.gap)
    for in_place in (False, True):
        got = cc.run_repair(rt, w, gap, hi, case.pad, in_place)
        assert cc.compare_repair(got, want, changed) == [], in_place
    assert cc.compare_repair(cc.run_repair(rt, w, gap, hi, case.pad, False, want_changed=False), want, changed) == []
    assert cc.compare_repair(cc.run_repair(rt, w, gap, hi, 0, True), want, changed) == []  # rows of exactly p columns
    assert rt.take_flags() == [0] * 16


@pytest.mark.parametrize("p", cc.ORDERS)
def test_every_kind_of_row(rt, p):
    case = cc.all_kinds_case(p)
    w, kinds = cc.repair_rows_of(case)
    want, changed = cc.repair_reference(case)
    gap, hi = cref.gap_hi(case.gap)
    got = cc.run_repair(rt, w, gap, hi, case.pad, True)
    assert cc.compare_repair(got, want, changed) == []
    out = got["out"]
    for r, kind in enumerate(kinds):
        if kind == "valid":  # unchanged bits
            assert got["changed"][r] == 0 and out[r].tobytes() == w[r].tobytes()
        elif kind.startswith("nan"):  # the NaN spreads as torch's does: the reference is torch's (the host test), and the
            # frame stays a NaN frame while its neighbours are whole
            assert np.isnan(out[r]).any()
        else:
            # (w[i] <= fl(w[i+1] - gap): the gap holds up to that one rounding, 2^-53 pi against gap >= 4.5e-3)
            assert np.all(np.diff(out[r]) >= gap * (1 - 1e-12)) and out[r][0] >= gap * (1 - 1e-12) and out[r][-1] <= hi, kind
        if not kind.startswith("nan"):
            assert np.all(np.isfinite(out[r])), kind
    # a frame's result depends on nothing but its own row: each frame alone
    for r in (0, 6, 7, 8, 9, 16):
        alone = cc.run_repair(rt, w[r:r + 1], gap, hi)
        assert lc.same_bits(alone["out"][0], out[r]) and alone["changed"][0] == got["changed"][r], kinds[r]


def test_repair_device_and_ilsf_give_the_torch_path_s_bits(rt):
    """world.lsf.repair_device against repair_rows on the device (the parent's path), in place and out of place on a
    column slice, and ilsf_device(min_gap > 0) against the envelope of repair_rows' result."""
    from world import lsf

    torch = rt.torch
    for p in (2, 24, 64):
        case = cc.RepairCase("chain", p, 129, 0.3 / (p + 2), 0, 40 + p)
        w, kinds = cc.repair_rows_of(case)
        rows = np.concatenate([np.linspace(-3.0, 2.0, len(w))[:, None], w], axis=1)
        rows_d = rt.to_device(rows)
        want = lsf.repair_rows(torch, rows_d[:, 1:], case.gap)
        got, changed = lsf.repair_device(rt, rows_d[:, 1:], case.gap, want_changed=True)
        assert lc.same_bits(got.cpu().numpy(), want.cpu().numpy())
        assert lc.same_bits(got.cpu().numpy(), cc.repair_reference(case)[0])
        assert np.array_equal(changed.cpu().numpy(), cc.repair_reference(case)[1])
        assert lc.same_bits(rows_d.cpu().numpy(), rows)  # out of place: the rows are as they were
        env = lsf.ilsf_device(rt, rows_d, 256, min_gap=case.gap)
        ex = torch.cat([torch.exp(rows_d[:, :1]), torch.cos(want)], dim=1)
        assert lc.same_bits(env.cpu().numpy(), lsf.envelope_device(rt, ex, 129).cpu().numpy())
        assert lc.same_bits(lsf.ilsf_device(rt, rows_d, 256).cpu().numpy(),
                            lsf.envelope_device(rt, torch.cat([torch.exp(rows_d[:, :1]), torch.cos(rows_d[:, 1:])], dim=1),
                                                129).cpu().numpy())
        again = rows_d.clone()
        lsf.repair_device(rt, again[:, 1:], case.gap, out=again[:, 1:])
        assert lc.same_bits(again[:, 1:].cpu().numpy(), want.cpu().numpy()) and lc.same_bits(again[:, 0].cpu().numpy(), rows[:, 0])
    assert tuple(lsf.repair_device(rt, rt.zeros((0, 24)), 0.01).shape) == (0, 24)
    for bad in (0.0, -0.1, np.pi / 26, float("nan")):
        with pytest.raises(ValueError):
            lsf.repair_device(rt, rt.zeros((4, 24)), bad)


# ---- distortion --------------------------------------------------------------------------------------------------------
def test_distortion_matches_the_reference(rt):
    worst = 0.0
    for case in cc.dist_cases():
        rows_a, rows_b, idx_a, idx_b = cc.dist_inputs(case)
        want, b1, b2 = cc.dist_reference(case)
        got = cc.run_distortion(rt, rows_a, rows_b, case.k_bins, idx_a, idx_b, case.pad)
        bad, ratio = cc.compare_distortion(got, want, b1, b2)
        assert bad == [], case.name
        worst = max(worst, ratio)
        again = cc.run_distortion(rt, rows_a, rows_b, case.k_bins, idx_a, idx_b, case.pad)
        assert got["out"].tobytes() == again["out"].tobytes(), case.name  # the same bits on a second run
    print("distortion: worst error / bound over %d cases: %.3f" % (len(cc.dist_cases()), worst))
    assert rt.take_flags() == [0] * 16


@pytest.mark.parametrize("p,k_bins", [(2, 129), (24, 513), (40, 1025), (64, 2049)])
def test_identical_rows_indices_and_independence(rt, p, k_bins):
    rng = np.random.RandomState(p)
    rows = cc.cosine_rows(9, p, rng)
    other = cc.cosine_rows(9, p, rng, spread=0.5)
    same = cc.run_distortion(rt, rows, rows, k_bins)
    assert same["rc"] == 0 and same["guards"] and np.all(same["out"] == 0.0) and not np.signbit(same["out"]).any()
    plain = cc.run_distortion(rt, rows, other, k_bins)["out"]
    # NULL indices and gathered indices with repeats: the same bits for the same pair of rows
    idx_a = np.array([3, 3, 0, 8, 5, 3, 1], dtype=np.int64)
    idx_b = np.array([3, 3, 0, 8, 5, 2, 1], dtype=np.int64)
    got = cc.run_distortion(rt, rows, other, k_bins, idx_a, idx_b)["out"]
    for n, (i, j) in enumerate(zip(idx_a, idx_b)):
        if i == j:
            assert got[n].tobytes() == plain[i].tobytes()
    assert got[0].tobytes() == got[1].tobytes() and got[5].tobytes() != got[0].tobytes()
    only_a = cc.run_distortion(rt, rows, other[:7], k_bins, idx_a, None)["out"]  # (pair n: rows[idx_a[n]] against other[n])
    assert only_a[4].tobytes() != plain[4].tobytes() and only_a[6].tobytes() != plain[6].tobytes()
    want = cref.distortion(rows, other[:7], k_bins, idx_a, None)
    t = cref.log_ratio(rows[idx_a, 1:], other[:7, 1:], k_bins)
    assert cc.compare_distortion({"out": only_a, "guards": True, "rc": 0}, want, *cref.order_bounds(t))[0] == []
    # a pair alone and inside a larger call
    for n in (0, 4, 8):
        alone = cc.run_distortion(rt, rows[n:n + 1], other[n:n + 1], k_bins)["out"]
        assert alone[0].tobytes() == plain[n].tobytes()


def test_bad_pairs_stay_inside_themselves(rt):
    from world.lsf import bin_table

    p, k_bins = 24, 513
    rng = np.random.RandomState(5)
    rows, other = cc.cosine_rows(12, p, rng), cc.cosine_rows(12, p, rng, spread=0.5)
    clean = cc.run_distortion(rt, rows, other, k_bins)["out"]
    idx_a = np.arange(12, dtype=np.int64)
    idx_b = np.arange(12, dtype=np.int64)
    idx_a[3], idx_b[7], idx_a[11] = 12, -1, 1 << 40
    got = cc.run_distortion(rt, rows, other, k_bins, idx_a, idx_b)
    assert got["rc"] == 0 and got["guards"]
    for n in range(12):
        if n in (3, 7, 11):
            assert np.isnan(got["out"][n]).all()
        else:
            assert got["out"][n].tobytes() == clean[n].tobytes()
    dirty = np.array(rows)
    dirty[2, 5] = np.nan  # a NaN root
    dirty[6, 9] = np.inf  # an infinite one: A2 = inf, and 0 * inf at the bin c = -1 where 2 (1 + c) = 0
    dirty[9, 5] = bin_table(k_bins)[100]  # a root exactly on a bin's cosine: P's factor, u = 0 there
    dirty[9, 6] = bin_table(k_bins)[100]  # and Q's: A2 = 0 at that bin, t = -inf
    got = cc.run_distortion(rt, dirty, other, k_bins)["out"]
    want = cref.distortion(dirty, other, k_bins)
    assert np.isnan(got[2]).all() and lc.same_bits(got[[2, 6, 9]], want[[2, 6, 9]])
    assert np.isnan(got[6]).all()
    assert got[9][0] == -np.inf and got[9][1] == np.inf
    for n in range(12):
        if n not in (2, 6, 9):
            assert got[n].tobytes() == clean[n].tobytes(), n
    assert rt.take_flags() == [0] * 16


def test_arguments_the_library_refuses(rt):
    from world.lsf import bin_table

    dp = ctypes.POINTER(ctypes.c_double)
    w, out = rt.zeros((4, 30)), rt.zeros((4, 30))

    def repair(n=4, ldw=30, p=24, gap=0.01, hi=3.0, ldo=30, src=w, dst=out):
        return rt.lib.wh_lsf_repair(rt.ctx, rt.stream(), rt.ptr(src), n, ldw, p, gap, hi, rt.ptr(dst), ldo, None)

    assert repair() == 0 and repair(n=0, src=None, dst=None) == 0
    for kw in (dict(p=1), dict(p=65), dict(n=-1), dict(ldw=23), dict(ldo=23), dict(gap=0.0), dict(gap=-1.0),
               dict(gap=float("nan")), dict(hi=0.001), dict(hi=float("nan")), dict(src=None), dict(dst=None)):
        assert repair(**kw) != 0, kw
    assert rt.lib.wh_lsf_repair(None, None, None, 0, 24, 24, 0.01, 3.0, None, 24, None) != 0
    bins = bin_table(513)
    res = rt.zeros((4, 2))

    def dist(na=4, lda=30, nb=4, ldb=30, p=24, n=4, k=513, a=w, b=out, o=res, tab=bins):
        return rt.lib.wh_lsf_distortion(rt.ctx, rt.stream(), rt.ptr(a), na, lda, rt.ptr(b), nb, ldb, p, None, None, n,
                                        None if tab is None else tab.ctypes.data_as(dp), k, rt.ptr(o))

    assert dist() == 0 and dist(n=0, o=None) == 0
    for kw in (dict(p=0), dict(p=25), dict(p=66), dict(na=-1), dict(nb=-1), dict(n=-1), dict(lda=24), dict(ldb=24),
               dict(k=1), dict(k=16386), dict(tab=None), dict(a=None), dict(b=None), dict(o=None)):
        assert dist(**kw) != 0, kw
    assert rt.lib.wh_lsf_distortion(None, None, None, 0, 25, None, 0, 25, 24, None, None, 0, None, 513, None) != 0
    rt.torch.cuda.synchronize()
    assert rt.take_flags() == [0] * 16


# ---- world.lsf: dB -----------------------------------------------------------------------------------------------------
def test_distortion_device_in_db(rt):
    """distortion_device on rows [log E, w ..] against the long-double definition on the two envelopes, both formulas,
    with and without indices; equal angles give c |g|; World.lsf_distortion is the same through NumPy."""
    from world import lsf
    from world.main import World

    p, fft_size, k = 24, 1024, 513
    rng = np.random.RandomState(11)
    w_a = np.sort(rng.uniform(0.05, np.pi - 0.05, size=(40, p)), axis=1)
    w_b = 0.6 * w_a + 0.4 * np.sort(rng.uniform(0.05, np.pi - 0.05, size=(40, p)), axis=1)
    rows_a = np.concatenate([rng.uniform(-8, 2, size=(40, 1)), w_a], axis=1)
    rows_b = np.concatenate([rng.uniform(-8, 2, size=(40, 1)), w_b], axis=1)
    a_d, b_d = rt.to_device(rows_a), rt.to_device(rows_b)
    # the device's own cosines (torch.cos on the device is not NumPy's to the last place): the truth is taken on them
    xa, xb = rt.torch.cos(a_d[:, 1:]).cpu().numpy(), rt.torch.cos(b_d[:, 1:]).cpu().numpy()
    t = cref.log_ratio(xa, xb, k, cref.LD)
    b1, b2 = cref.sum_bounds(t, p)
    s1, s2 = np.sum(t, axis=1), np.sum(t * t, axis=1)
    g = rows_a[:, 0] - rows_b[:, 0]
    for gain in (True, False):
        d = t - np.mean(t, axis=1, keepdims=True) if not gain else g[:, None].astype(cref.LD) - t
        want = cref.LD(cref.LSD_SCALE) * np.sqrt(np.mean(d * d, axis=1))
        tol = cref.db_bound(g, s1.astype(np.float64), s2.astype(np.float64), b1, b2, k, gain)
        got = lsf.distortion_device(rt, a_d, b_d, fft_size, gain=gain).cpu().numpy()
        assert np.all(np.abs(got - want.astype(np.float64)) <= tol), gain
        idx = rt.torch.arange(39, -1, -1, device=rt.device)
        rev = lsf.distortion_device(rt, a_d, b_d, fft_size, idx_a=idx, idx_b=idx, gain=gain).cpu().numpy()
        assert rev[::-1].tobytes() == got.tobytes()
        host = World().lsf_distortion(rows_a, rows_b, fft_size, gain=gain)
        assert host.tobytes() == got.tobytes()
    same = rt.to_device(np.concatenate([rows_b[:, :1], w_a], axis=1))
    got = lsf.distortion_device(rt, a_d, same, fft_size).cpu().numpy()
    assert np.array_equal(got, cref.LSD_SCALE * np.abs(g))
    assert np.all(lsf.distortion_device(rt, a_d, same, fft_size, gain=False).cpu().numpy() == 0.0)
    out_of_range = rt.torch.tensor([0, 40, -1], device=rt.device)
    got = lsf.distortion_device(rt, a_d, b_d, fft_size, idx_a=out_of_range, idx_b=rt.torch.tensor([0, 1, 2], device=rt.device))
    assert np.isfinite(got[0].item()) and np.isnan(got[1].item()) and np.isnan(got[2].item())
    assert rt.take_flags() == [0] * 16
