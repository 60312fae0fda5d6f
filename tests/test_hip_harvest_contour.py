"""GPU: Harvest's pruning and contour stages on crafted candidate maps, through wh_harvest_contour_probe
(csrc/wh_hv_probe.hip): hv_prune_kernel of wh_hv_refine.hip and the seven kernels of wh_hv_contour.hip, launched by the
launchers wh_harvest calls, stage by stage against tests/_harvest_contour_reference.py and against the unmodified
reference's recorded results (tests/golden/golden_harvest_contour.npz).  The maps are tests/_harvest_contour_cases.py's;
tests/test_harvest_contour_reference_host.py shows on the CPU which branch each of them takes.

Every case runs in both modes (0: the reference's keep masks go in; 1: the probe runs the pruning itself) and in both
list forms (dense: all 105 rows of every frame listed, zeros included; compact: only the non-zero rows, in row order).

Comparison rules.  Keep masks, base, s1 - s4, vuv, the section table (first, last, extended first, extended last, kept)
and the values picked onto the frame grid are compared BIT FOR BIT: these stages select and copy, the units are built
without contraction, and the host test holds the margins of the two decisions that depend on a summation order.  The
smoothed row is the one place with arithmetic in another order (a 300-sample hold instead of the whole padded contour):
its tolerance is HC.SMOOTH_BOUND = 16 x 8.0e-12 Hz (the float64 rounding noise of SmoothF0 itself, measured on the CPU
against np.longdouble over every case: 7.96e-12 Hz) + 4.32e-18 x 800 Hz (the hold's truncation) = 1.3e-10 Hz."""
import ctypes

import numpy as np
import pytest

import _harvest_contour_cases as HC
import _harvest_contour_reference as HR
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

MODES = (0, 1)
FORMS = ("dense", "compact")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


_refs = {}


def ref_of(name):
    """(case, the restatement's Result): computed once, shared by every test"""
    if name not in _refs:
        c = HC.get(name)
        _refs[name] = (c, HR.run(c.cands, c.scores))
    return _refs[name]


@pytest.fixture(scope="module")
def recorded():
    import os

    return dict(np.load(os.path.join(GOLDEN, "golden_harvest_contour.npz")))


def grid_5ms(n):
    return np.arange((n - 1) // 5 + 1) * 0.005


class Utt:
    """one utterance of a probe call: the map in one list form, the masks that go in (mode 0), the output times"""

    def __init__(self, cands, scores, form, alive, tp=None):
        self.n = cands.shape[1]
        self.f0, self.sc, self.lst, self.pos = HC.pack(cands, scores, form)
        self.masks = HC.masks(alive, self.pos)
        self.tp = grid_5ms(self.n) if tp is None else np.asarray(tp, dtype=np.float64)


_utts = {}


def utt_of(name, form, tp=None):
    c, r = ref_of(name)
    if tp is not None:
        return Utt(c.cands, c.scores, form, r.pruned_c != 0, tp)
    if (name, form) not in _utts:
        _utts[name, form] = Utt(c.cands, c.scores, form, r.pruned_c != 0)
    return _utts[name, form]


def probe(mode, utts):
    """-> per utterance dict(keep [n][4] uint32, rows [6][n], f0, vuv, sections [(st, ed, r0, r1, kept)])"""
    from world import _hip

    rt = _hip.Runtime.get()
    nf1 = np.array([u.n for u in utts], dtype=np.int64)
    f1_off = np.concatenate([[0], np.cumsum(nf1)])
    f_off = np.concatenate([[0], np.cumsum([len(u.tp) for u in utts])]).astype(np.int64)
    slot0 = np.concatenate([[0], np.cumsum([len(u.f0) for u in utts])])
    pool_f0 = np.concatenate([u.f0 for u in utts] + [np.zeros(1)])  # (one spare slot: an empty pool still has an address)
    pool_sc = np.concatenate([u.sc for u in utts] + [np.zeros(1)])
    lst = np.concatenate([u.lst + (int(slot0[i]) << 8) for i, u in enumerate(utts)]).astype(np.int64)
    keep_in = np.concatenate([u.masks for u in utts]) if mode == 0 else np.zeros((int(f1_off[-1]), 4), dtype=np.uint32)
    tp_d = rt.to_device(np.concatenate([u.tp for u in utts]))
    f0_d, sc_d = rt.to_device(pool_f0), rt.to_device(pool_sc)
    keep_d = rt.to_device(keep_in.view(np.int32), dtype=np.int32)
    f0_out, vuv_out = rt.empty((int(f_off[-1]),)), rt.empty((int(f_off[-1]),))
    rows = rt.zeros((6 * int(f1_off[-1]),))
    sec_cap = int(nf1.max()) // 2 + 8
    nsec = np.zeros(len(utts), dtype=np.int32)
    secs = np.zeros((len(utts), sec_cap, 5), dtype=np.int32)
    _hip.check(rt.lib.wh_harvest_contour_probe(
        rt.ctx, rt.stream(), mode, len(utts), nf1.ctypes.data_as(ctypes.c_void_p), f_off.ctypes.data_as(ctypes.c_void_p),
        rt.ptr(tp_d), rt.ptr(f0_d), rt.ptr(sc_d), len(pool_f0), lst.ctypes.data_as(ctypes.c_void_p), rt.ptr(keep_d),
        rt.ptr(f0_out), rt.ptr(vuv_out), rt.ptr(rows), nsec.ctypes.data_as(ctypes.c_void_p),
        secs.ctypes.data_as(ctypes.c_void_p), sec_cap))
    keep = keep_d.cpu().numpy().view(np.uint32)
    rows, f0_out, vuv_out = rows.cpu().numpy(), f0_out.cpu().numpy(), vuv_out.cpu().numpy()
    out = []
    for i, u in enumerate(utts):
        a, b = int(f1_off[i]), int(f1_off[i + 1])
        out.append(dict(keep=keep[a:b], rows=rows[6 * a : 6 * b].reshape(6, u.n), f0=f0_out[f_off[i] : f_off[i + 1]],
                        vuv=vuv_out[f_off[i] : f_off[i + 1]], sections=[tuple(int(v) for v in s) for s in secs[i, : nsec[i]]]))
    return out


def no_flags():
    from world import _hip

    assert _hip.Runtime.get().take_flags() == [0] * 16


def check_against_reference(got, u, r, what):
    """one utterance's probe output against the restatement's Result"""
    assert np.array_equal(HC.unmask(got["keep"], u.pos), r.pruned_c != 0), what + ": keep masks"
    assert np.array_equal(got["keep"], u.masks), what + ": keep mask words (bits beyond the list are clear)"
    for k, stage in enumerate(("base", "s1", "s2", "s3", "s4")):
        assert np.array_equal(_bits(got["rows"][k]), _bits(getattr(r, stage))), "%s: %s" % (what, stage)
    assert got["sections"] == [tuple(int(v) for v in s) for s in r.sections], what + ": sections"
    assert np.array_equal(got["rows"][5] == 0, r.s4 == 0)
    err = float(np.max(np.abs(got["rows"][5] - r.smoothed)))
    assert err <= HC.SMOOTH_BOUND, "%s: smoothed row off by %.3e Hz" % (what, err)
    idx = HR.pick_index(u.tp, u.n)
    assert np.array_equal(_bits(got["f0"]), _bits(got["rows"][5][idx])), what + ": f0 on the frame grid"
    assert np.array_equal(got["vuv"], (r.s4[idx] != 0).astype(np.float64)), what + ": vuv on the frame grid"
    return err


@pytest.mark.parametrize("name", HC.names())
def test_stages_against_the_reference(recorded, name):
    c, r = ref_of(name)
    worst = 0.0
    for form in FORMS:
        u = utt_of(name, form)
        for mode in MODES:
            got = probe(mode, [u])[0]
            worst = max(worst, check_against_reference(got, u, r, "%s mode %d %s" % (name, mode, form)))
            if name in HC.TIED and not bool(recorded[name + ".binding"]):
                continue
            # the unmodified reference's own results
            assert np.array_equal(_bits(got["rows"][4]), _bits(recorded[name + ".contour"]))
            assert np.array_equal(got["rows"][4] != 0, np.unpackbits(recorded[name + ".vuv_bits"])[: u.n] != 0)
            assert np.max(np.abs(got["rows"][5] - recorded[name + ".smoothed"])) <= HC.SMOOTH_BOUND
    print(name, "smoothed row: largest difference %.3e Hz (bound %.3e)" % (worst, HC.SMOOTH_BOUND))
    no_flags()


def test_both_list_forms_give_the_same_bits():
    """wh_hv_contour.hip's contract: only the order of a frame's candidates matters and an absent candidate is a zero"""
    for name in ("wide_lists", "pick_ties", "densest_sections_overlapping", "merge_partial_first_wins"):
        for mode in MODES:
            d, c = (probe(mode, [utt_of(name, form)])[0] for form in FORMS)
            assert np.array_equal(_bits(d["rows"]), _bits(c["rows"])) and d["sections"] == c["sections"], (name, mode)
            assert np.array_equal(_bits(d["f0"]), _bits(c["f0"])) and np.array_equal(d["vuv"], c["vuv"])
    no_flags()


def test_densest_layout_loses_no_section():
    """7-frame runs one frame apart over 1203 frames: 149 sections, each with a 209-frame window in the channel area; a
    section dropped where the area is carved (hc_sections_kernel's break) would be missing here"""
    c, r = ref_of("densest_sections")
    got = probe(1, [utt_of("densest_sections", "compact")])[0]
    assert len(got["sections"]) == len(r.sections) == 149
    assert all(s[4] == 1 for s in got["sections"])
    no_flags()


def test_one_frame_is_unvoiced():
    """a contour of one frame, which the reference cannot process (it indexes frame 1): all unvoiced, finite, no flags"""
    cands = np.zeros((HC.ROWS, 1))
    cands[7, 0] = 400.0
    scores = np.where(cands != 0, 5.0, 0.0)
    for form in FORMS:
        for mode in MODES:
            got = probe(mode, [Utt(cands, scores, form, cands != 0, tp=[0.0, 0.005])])[0]
            assert np.all(np.isfinite(got["rows"])) and not got["rows"][1:].any() and got["sections"] == []
            assert not got["f0"].any() and not got["vuv"].any()
    no_flags()


def test_two_frames_are_unvoiced():
    c, r = ref_of("shape_2")
    assert not r.vuv.any()
    got = probe(1, [utt_of("shape_2", "dense")])[0]
    assert np.all(np.isfinite(got["rows"])) and not got["rows"][1:].any() and not got["f0"].any() and not got["vuv"].any()
    no_flags()


BATCH = ("shape_17", "wide_lists", "shape_3", "densest_sections_overlapping", "pick_ties", "shape_256", "none_kept",
         "extension_to_the_clamps", "shape_2", "merge_partial_first_wins", "seams_a", "shape_255", "gaps_8_9_1",
         "touches_ends", "shape_257", "extension_stops")


def test_ragged_batch_equals_the_single_utterances():
    """16 of the cases in one call, in mixed order: every utterance bit for bit what it gives alone (f1_off, the
    per-utterance slices of the workspace, the grids sized by the longest)"""
    for mode in MODES:
        for form in FORMS:
            utts = [utt_of(name, form) for name in BATCH]
            together = probe(mode, utts)
            for name, u, got in zip(BATCH, utts, together):
                alone = probe(mode, [u])[0]
                what = "%s mode %d %s" % (name, mode, form)
                assert np.array_equal(got["keep"], alone["keep"]), what
                assert np.array_equal(_bits(got["rows"]), _bits(alone["rows"])), what
                assert got["sections"] == alone["sections"], what
                assert np.array_equal(_bits(got["f0"]), _bits(alone["f0"])) and np.array_equal(got["vuv"], alone["vuv"]), what
                check_against_reference(got, u, ref_of(name)[1], what)
    no_flags()


@pytest.mark.parametrize("name", ["seams_b", "shape_17", "three_misses_then_a_hit"])
def test_frame_grids(name):
    """5 ms and 2 ms grids, times off the 1 ms grid (halves round up) and times past the end (clamped to the last frame)"""
    c, r = ref_of(name)
    n = c.cands.shape[1]
    rng = np.random.RandomState(n)
    grids = {"5 ms": grid_5ms(n), "2 ms": np.arange((n - 1) // 2 + 1) * 0.002,
             "off grid": np.sort(rng.uniform(0, (n - 1) / 1000.0, 97)),
             "halves and the end": np.array([0.0, 0.0004999, 0.0005, 0.0015, 0.0025, (n - 1.5) / 1000, (n - 1) / 1000,
                                             n / 1000, (n + 50.0) / 1000, 10.0])}
    for label, tp in grids.items():
        u = utt_of(name, "compact", tp)
        got = probe(1, [u])[0]
        idx = HR.pick_index(tp, n)
        assert idx.min() >= 0 and idx.max() <= n - 1
        check_against_reference(got, u, r, name + " " + label)
        assert np.max(np.abs(got["f0"] - r.smoothed[idx])) <= HC.SMOOTH_BOUND
    assert HR.pick_index([10.0], n)[0] == n - 1
    no_flags()


def smooth_probe(rows):
    """mode 2: the smoothing and the pick alone on step-4 rows -> per row (smoothed, f0 at 5 ms, vuv at 5 ms)"""
    from world import _hip

    rt = _hip.Runtime.get()
    nf1 = np.array([len(r) for r in rows], dtype=np.int64)
    f1_off = np.concatenate([[0], np.cumsum(nf1)])
    tps = [grid_5ms(len(r)) for r in rows]
    f_off = np.concatenate([[0], np.cumsum([len(t) for t in tps])]).astype(np.int64)
    six = np.full(6 * int(f1_off[-1]), np.nan)  # (only row 4 is read; NaN elsewhere would show in the outputs)
    for i, r in enumerate(rows):
        six[6 * int(f1_off[i]) + 4 * len(r) : 6 * int(f1_off[i]) + 5 * len(r)] = r
    six_d, tp_d = rt.to_device(six), rt.to_device(np.concatenate(tps))
    f0_out, vuv_out = rt.empty((int(f_off[-1]),)), rt.empty((int(f_off[-1]),))
    nsec = np.full(len(rows), -1, dtype=np.int32)
    secs = np.zeros((len(rows), 1, 5), dtype=np.int32)
    vp = ctypes.c_void_p
    _hip.check(rt.lib.wh_harvest_contour_probe(
        rt.ctx, rt.stream(), 2, len(rows), nf1.ctypes.data_as(vp), f_off.ctypes.data_as(vp), rt.ptr(tp_d), None, None, 0,
        None, None, rt.ptr(f0_out), rt.ptr(vuv_out), rt.ptr(six_d), nsec.ctypes.data_as(vp), secs.ctypes.data_as(vp), 1))
    assert not nsec.any()
    six, f0_out, vuv_out = six_d.cpu().numpy(), f0_out.cpu().numpy(), vuv_out.cpu().numpy()
    return [(six[6 * int(f1_off[i]) + 5 * len(r) : 6 * int(f1_off[i]) + 6 * len(r)], f0_out[f_off[i] : f_off[i + 1]],
             vuv_out[f_off[i] : f_off[i + 1]]) for i, r in enumerate(rows)]


def test_smoothing_alone_at_the_densest_layouts(recorded):
    """Step-4 contours FixF0Contour cannot leave, handed to hc_smooth_kernel directly (mode 2): single frames nine frames
    apart — the densest layout its scratch slices (run + 300 doubles each, 256 runs at a time, in 32 nf1 + 1024) allow —,
    more than 256 runs (the second tile of the run loop), one run over everything.  A run left unsmoothed would show in
    the two-frame runs, whose values the filter moves by tens of Hz."""
    rows = HC.smooth_rows()
    want = {name: HR.smooth(row) for name, row in rows.items()}
    pair = rows["singles_and_pairs_9_apart"]
    assert np.max(np.abs(want["singles_and_pairs_9_apart"] - pair)) > 10.0
    for names in [[n] for n in rows] + [list(rows)[::-1]]:
        for name, (sm, f0, vuv) in zip(names, smooth_probe([rows[n] for n in names])):
            err = float(np.max(np.abs(sm - want[name])))
            print(name, "alone" if len(names) == 1 else "batched", "largest difference %.3e Hz" % err)
            assert err <= HC.SMOOTH_BOUND and np.array_equal(sm == 0, rows[name] == 0), name
            assert np.max(np.abs(sm - recorded["smooth." + name])) <= HC.SMOOTH_BOUND, name
            idx = HR.pick_index(grid_5ms(len(sm)), len(sm))
            assert np.array_equal(_bits(f0), _bits(sm[idx])) and np.array_equal(vuv, (rows[name][idx] != 0) * 1.0), name
    no_flags()


def test_arguments_the_probe_refuses():
    from world import _hip

    rt = _hip.Runtime.get()
    u = utt_of("shape_3", "compact")
    vp = ctypes.c_void_p
    nf1 = np.array([3], dtype=np.int64)
    f_off = np.array([0, 1], dtype=np.int64)
    lst = u.lst.copy()
    pool = rt.to_device(np.concatenate([u.f0, np.zeros(200)]))
    keep = rt.to_device(u.masks.view(np.int32), dtype=np.int32)
    buf = rt.zeros((64,))
    nsec, secs = np.zeros(1, dtype=np.int32), np.zeros((1, 16, 5), dtype=np.int32)

    def call(mode=1, n_utt=1, nf1=nf1, f_off=f_off, tp=buf, f0=pool, sc=pool, pool_n=len(u.f0), lst=lst, keep=keep, out=buf):
        return rt.lib.wh_harvest_contour_probe(
            rt.ctx, rt.stream(), mode, n_utt, nf1.ctypes.data_as(vp), f_off.ctypes.data_as(vp), rt.ptr(tp), rt.ptr(f0),
            rt.ptr(sc), pool_n, None if lst is None else lst.ctypes.data_as(vp), rt.ptr(keep), rt.ptr(out), rt.ptr(buf),
            rt.ptr(buf), nsec.ctypes.data_as(vp), secs.ctypes.data_as(vp), 16)

    assert call() == 0
    too_many = lst.copy()
    too_many[1] = (0 << 8) | 106
    assert call(lst=too_many, pool_n=len(u.f0) + 200) != 0 and b"wh_harvest_contour_probe" in rt.lib.wh_last_error()
    leaves = lst.copy()
    leaves[2] = (len(u.f0) << 8) | 1
    assert call(lst=leaves) != 0
    assert call(lst=-lst - 1) != 0
    assert call(nf1=np.array([0], dtype=np.int64)) != 0
    assert call(f_off=np.array([0, 0], dtype=np.int64)) != 0
    assert call(tp=None) != 0 and call(f0=None) != 0 and call(sc=None) != 0 and call(lst=None) != 0
    assert call(keep=None) != 0 and call(out=None) != 0
    assert call(mode=3) != 0 and call(n_utt=0) != 0 and call(pool_n=-1) != 0
    assert call() == 0
    no_flags()
