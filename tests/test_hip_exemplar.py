"""wh_knn and wh_frame_select (csrc/wh_exemplar.hip) against tests/_exemplar_reference.py, bit for bit: idx, dist, sel,
slot, total and the accumulated costs.  The cases, the runners and the references: tests/_exemplar_cases.py."""
import numpy as np
import pytest

import _exemplar_cases as xc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    from world import _hip
    return _hip.Runtime.get()


def _case(cases, name):
    return next(c for c in cases if c.name == name)


# ---- wh_knn -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", xc.knn_cases(), ids=lambda c: c.name)
def test_knn_equals_the_reference(rt, case):
    assert xc.knn_compare(case, xc.knn_run(rt, case)) == []
    assert rt.take_flags() == [0] * 16


@pytest.mark.parametrize("name", xc.SPLIT_CASES)
def test_knn_every_cut_of_the_database_gives_the_same_bytes(rt, name):
    case = _case(xc.knn_cases(), name)
    for splits in xc.knn_splits(case):
        assert xc.knn_compare(case, xc.knn_run(rt, case, splits=splits)) == [], splits


def test_knn_empty_slots_are_minus_one_and_inf(rt):
    case = _case(xc.knn_cases(), "exclusions")
    got = xc.knn_run(rt, case)
    assert np.all(got["idx"][7] == -1) and np.all(np.isposinf(got["dist"][7]))           # no candidate left
    assert np.all(got["idx"][6][4:] == -1) and np.all(np.isposinf(got["dist"][6][4:]))                  # four are left
    assert set(got["idx"][6][:4].tolist()) == {0, 1, case.n_db - 2, case.n_db - 1}
    case = _case(xc.knn_cases(), "K=8 > n_db=3")
    got = xc.knn_run(rt, case)
    assert np.all(got["idx"][:, 3:] == -1) and np.all(np.isposinf(got["dist"][:, 3:])) and np.all(got["idx"][:, :3] >= 0)


def test_knn_non_finite_database_rows_come_last_by_index(rt):
    case = _case(xc.knn_cases(), "NaN and Inf rows in the database, all listed")
    got = xc.knn_run(rt, case)
    assert xc.knn_compare(case, got) == []
    assert np.all(got["idx"][:, 27:30] == [5, 15, 29]) and np.all(np.isposinf(got["dist"][:, 27:30]))
    assert np.all(got["idx"][:, 30:] == -1)


def test_knn_a_query_does_not_depend_on_the_others(rt):
    case = _case(xc.knn_cases(), "NaN and Inf rows in the queries")
    whole = xc.knn_run(rt, case)
    assert xc.knn_compare(case, whole) == []
    clean = np.array(xc.knn_inputs(case)["q"])
    clean[3, 1], clean[xc.TILE_Q, 0] = 0.5, -0.5
    other = xc.knn_run(rt, case, q=clean)
    keep = np.ones(case.n_q, dtype=bool)
    keep[[3, xc.TILE_Q]] = False
    assert whole["idx"][keep].tobytes() == other["idx"][keep].tobytes()
    assert whole["dist"][keep].tobytes() == other["dist"][keep].tobytes()
    assert whole["idx"][xc.TILE_Q].tolist() == list(range(case.k))  # every key +inf: by index
    for case in (case, _case(xc.knn_cases(), "exclusions with ties")):
        whole = xc.knn_run(rt, case)
        for n in (0, 3, 7, 8, xc.TILE_Q - 1, xc.TILE_Q, case.n_q - 1):
            alone = xc.knn_run(rt, case, only=n)
            assert alone["rc"] == 0 and alone["guards"]
            assert alone["idx"].tobytes() == whole["idx"][n:n + 1].tobytes()
            assert xc.same_bits(alone["dist"], whole["dist"][n:n + 1])


def test_knn_repeats(rt):
    case = _case(xc.knn_cases(), "integer ties")
    a, b = xc.knn_run(rt, case, splits=7), xc.knn_run(rt, case, splits=7)
    assert a["idx"].tobytes() == b["idx"].tobytes() and a["dist"].tobytes() == b["dist"].tobytes()


def test_knn_empty_calls(rt):
    torch = rt.torch
    z = torch.zeros((4, 3), dtype=torch.float64, device=rt.device)
    idx = torch.full((4, 2), 5, dtype=torch.int32, device=rt.device)
    dist = torch.zeros((4, 2), dtype=torch.float64, device=rt.device)
    assert xc.knn_call(rt, z, 0, 3, z, 4, 3, 3, 2, None, None, 0, idx, dist) == 0  # no queries: nothing is written
    assert bool((idx == 5).all())
    assert xc.knn_call(rt, z, 4, 3, None, 0, 3, 3, 2, None, None, 0, idx, dist) == 0  # no rows: every slot is empty
    assert bool((idx == -1).all()) and bool(torch.isposinf(dist).all())
    assert rt.take_flags() == [0] * 16


def test_knn_argument_errors(rt):
    from world import _hip
    torch = rt.torch
    z = torch.zeros((4, 170), dtype=torch.float64, device=rt.device)
    i32 = torch.zeros((4,), dtype=torch.int32, device=rt.device)
    idx = torch.zeros((4, 40), dtype=torch.int32, device=rt.device)
    dist = torch.zeros((4, 40), dtype=torch.float64, device=rt.device)
    ok = dict(q=z, n_q=4, ldq=170, db=z, n_db=4, lddb=170, d=3, k=2, lo=None, hi=None, splits=0, idx=idx, dist=dist)
    order = ("q", "n_q", "ldq", "db", "n_db", "lddb", "d", "k", "lo", "hi", "splits", "idx", "dist")
    assert xc.knn_call(rt, *(ok[n] for n in order)) == 0
    for change in (dict(d=0), dict(d=161), dict(k=0), dict(k=33), dict(n_db=2 ** 31), dict(n_q=-1), dict(n_db=-1), dict(ldq=2),
                   dict(lddb=2), dict(q=None), dict(db=None), dict(idx=None), dict(dist=None), dict(lo=i32), dict(hi=i32),
                   dict(splits=-1)):
        args = dict(ok, **change)
        assert xc.knn_call(rt, *(args[n] for n in order)) != 0, change
        assert b"wh_knn" in _hip.load_library().wh_last_error(), change
    assert rt.take_flags() == [0] * 16


# ---- wh_frame_select ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", xc.sel_cases(), ids=lambda c: c.name)
def test_select_equals_the_reference(rt, case):
    assert xc.sel_compare(case, xc.sel_run(rt, case)) == []
    assert rt.take_flags() == [0] * 16


def test_select_an_utterance_does_not_depend_on_its_batch(rt):
    for name in ("ragged, empty first, last and in the middle", "integer ties", "invalid slots"):
        case = _case(xc.sel_cases(), name)
        for u in range(len(case.frames)):
            assert xc.sel_compare(case, xc.sel_run(rt, case, only=u)) == [], (name, u)


def test_select_non_finite_rows_stay_in_their_utterance(rt):
    case = _case(xc.sel_cases(), "NaN and Inf rows of y in utterance 1")
    got, clean = xc.sel_run(rt, case), xc.sel_run(rt, case, clean=True)
    assert xc.sel_compare(case, clean, clean=True) == []
    fo = xc.sel_inputs(case)["frame_off"]
    for u in (0, 2):
        s = slice(int(fo[u]), int(fo[u + 1]))
        for key in ("sel", "slot", "acc"):
            assert got[key][s].tobytes() == clean[key][s].tobytes(), (u, key)
        assert got["total"][u].tobytes() == clean["total"][u].tobytes()
    s = slice(int(fo[1]), int(fo[2]))  # the utterance that is hit: a well-formed selection
    idx = xc.sel_inputs(case)["idx"]
    assert np.all((got["slot"][s] >= 0) & (got["slot"][s] < case.k))
    assert np.array_equal(got["sel"][s], idx[s][np.arange(s.stop - s.start), got["slot"][s]])


def test_select_repeats_and_optional_outputs(rt):
    case = _case(xc.sel_cases(), "integer ties K=32")
    a, b = xc.sel_run(rt, case), xc.sel_run(rt, case)
    for key in ("sel", "slot", "total", "acc"):
        assert a[key].tobytes() == b[key].tobytes(), key
    c = xc.sel_run(rt, case, want_slot=False, want_acc=False)
    assert xc.sel_compare(case, c) == [] and c["sel"].tobytes() == a["sel"].tobytes()


def test_select_weight_zero_takes_the_nearest(rt):
    case = _case(xc.sel_cases(), "weight=0")
    got = xc.sel_run(rt, case)
    inp = xc.sel_inputs(case)
    first = np.argmin(inp["tc"], axis=1)  # (noise: no ties)
    assert np.array_equal(got["slot"], first) and np.array_equal(got["sel"], inp["idx"][np.arange(len(first)), first])


def test_select_argument_errors(rt):
    from world import _hip
    torch = rt.torch
    batch = rt.make_batch(np.zeros(2, dtype=np.int64), np.array([0, 4], dtype=np.int64))
    idx = torch.zeros((4, 40), dtype=torch.int32, device=rt.device)
    f64 = torch.zeros((4, 70), dtype=torch.float64, device=rt.device)
    ok = dict(b=batch.handle, idx=idx, tc=f64, k=2, y=f64, n_db=4, ldy=70, dy=3, succ=idx, weight=1.0, sel=idx, slot=None,
              total=f64, acc=None)
    order = ("b", "idx", "tc", "k", "y", "n_db", "ldy", "dy", "succ", "weight", "sel", "slot", "total", "acc")

    def call(a):
        return rt.lib.wh_frame_select(rt.ctx, rt.stream(), *(a[n] if n in ("b", "k", "n_db", "ldy", "dy", "weight") else rt.ptr(a[n]) for n in order))

    assert call(ok) == 0
    for change in (dict(b=None), dict(k=0), dict(k=33), dict(dy=0), dict(dy=65), dict(ldy=2), dict(n_db=-1), dict(n_db=2 ** 31),
                   dict(weight=-1.0), dict(weight=float("inf")), dict(weight=float("nan")), dict(idx=None), dict(tc=None),
                   dict(y=None), dict(succ=None), dict(sel=None), dict(total=None)):
        assert call(dict(ok, **change)) != 0, change
        assert b"wh_frame_select" in _hip.load_library().wh_last_error(), change
    assert rt.take_flags() == [0] * 16
