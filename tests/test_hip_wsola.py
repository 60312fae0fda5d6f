"""GPU: wh_wsola (csrc/wh_wsola.hip) through the C ABI, bit for bit against tests/_wsola_reference.py — the shifts and
y — at the smallest shapes that reach every edge (tests/_wsola_cases.py): hops 1, 2, 80, 176 and 1024; tolerances 0, 1 and
on both sides of every multiple of the workgroup's 256 threads that 2 D + 1 candidates cross, up to 512; the ratios 1, 4/5,
5/4, 3/2 and 1/2; position lists that are not monotone or leave the utterance by anything up to the ends of the int64
range; utterances that are empty, one sample long and shorter than a hop; ragged batches; digital silence; an
integer-valued periodic signal whose scores tie exactly; silence next to signal; a NaN and an Inf that stay inside their
utterance; repeated runs; an utterance alone against itself in its batch; delta == NULL."""
import numpy as np
import pytest

import _wsola_cases as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    from world import _hip
    return _hip.Runtime.get()


@pytest.mark.parametrize("case", wc.all_cases(), ids=lambda c: c.name)
def test_cases_match_the_reference_bit_for_bit(rt, case):
    got = wc.run(rt, case)
    assert wc.compare_case(case, got) == []
    assert rt.take_flags() == [0] * 16


def test_the_case_list_reaches_what_it_claims():
    """Host arithmetic on the references: the shifts use the whole tolerance and every thread slot, ties occur, silence rests."""
    by_name = {c.name: c for c in wc.all_cases()}
    assert {c.hop for c in wc.hop_cases()} == {1, 2, 80, 176, 1024} and {c.tol for c in wc.tol_cases()} == set(wc.TOLS)
    for case in wc.tol_cases():
        d = wc.reference(case)[0][1]
        assert np.all(np.abs(d) <= case.tol)
        # the first and the last candidate win somewhere, and a candidate of every thread slot (k = d + D, slot k // 256)
        assert d[3] == -case.tol and d[5] == case.tol, case.name
        assert set(((d[1:] + case.tol) // 256).tolist()) == set(range((2 * case.tol) // 256 + 1)), case.name
    for y, d in wc.reference(by_name["digital silence"])[:1]:
        assert not np.any(d) and not np.any(y)
    d = wc.reference(by_name["periodic integers: ties on two waves"])[0][1]
    inner = d[13:]  # (behind the first D = 200 samples, where the zeros in front of the utterance break the period)
    assert np.all(np.abs(inner) <= 2) and np.any(inner != 0)  # of the shifts 5 apart that tie, the smallest
    d = wc.reference(by_name["positions out of range"])[0][1]
    assert np.any(d != 0)


def test_bitwise_repeatable_alone_equals_in_batch_and_delta_may_be_null(rt):
    by_name = {c.name: c for c in wc.all_cases()}
    for name in ("H=80 D=50 ratios", "H=16 D=256", "ragged eight", "empty, one sample, shorter than H", "positions out of range",
                 "periodic integers: exact ties"):
        case = by_name[name]
        first, again, quiet = wc.run(rt, case), wc.run(rt, case), wc.run(rt, case, want_delta=False)
        assert first["rc"] == 0 and again["rc"] == 0 and quiet["rc"] == 0 and quiet["guards"] and quiet["delta"] is None
        for u in range(len(case.utts)):
            assert first["y"][u].tobytes() == again["y"][u].tobytes() == quiet["y"][u].tobytes(), (name, u)
            assert first["delta"][u].tobytes() == again["delta"][u].tobytes(), (name, u)
            alone = wc.run(rt, case, only=u)
            assert alone["rc"] == 0 and alone["guards"]
            assert alone["y"][0].tobytes() == first["y"][u].tobytes() and alone["delta"][0].tobytes() == first["delta"][u].tobytes(), (name, u)
    assert rt.take_flags() == [0] * 16


@pytest.mark.parametrize("what", ["nan", "inf"])
def test_a_nan_or_inf_stays_inside_its_utterance(rt, what):
    case = wc.Case(what, 80, 50, (("tone", 900, "ratio", 1.25), (what, 700, "ratio", 0.8), ("noise", 500, "ratio", 1.5)), 300)
    clean = wc.Case("clean", 80, 50, (("tone", 900, "ratio", 1.25), ("noise", 700, "ratio", 0.8), ("noise", 500, "ratio", 1.5)), 300)
    got, ref = wc.run(rt, case), wc.run(rt, clean)
    assert wc.compare_case(case, got) == [] and ref["rc"] == 0
    # (a frame may step round the one sample — every candidate that holds it scores -inf —, so y itself may stay finite)
    assert not np.all(np.isfinite(wc.inputs(case)["x"][1]))
    for u in (0, 2):  # the neighbours' bits are those of the batch without the NaN
        assert np.array_equal(wc.inputs(case)["x"][u], wc.inputs(clean)["x"][u])
        assert got["y"][u].tobytes() == ref["y"][u].tobytes() and got["delta"][u].tobytes() == ref["delta"][u].tobytes()
    # an utterance of nothing but NaN: every shift is 0
    x = [wc.inputs(case)["x"][0], np.full(700, np.nan), wc.inputs(case)["x"][2]]
    got = wc.run(rt, case, xs=x)
    assert got["rc"] == 0 and not np.any(got["delta"][1]) and np.all(np.isnan(got["y"][1][100:400]))
    assert got["y"][0].tobytes() == ref["y"][0].tobytes() and got["y"][2].tobytes() == ref["y"][2].tobytes()
    assert rt.take_flags() == [0] * 16


def test_argument_errors(rt):
    x = rt.to_device(np.ones(200))
    y = rt.empty((250,))
    d = rt.torch.zeros((5,), dtype=rt.torch.int32, device=rt.device)
    pos = [0, 60, 120, 180, 240]  # ceil(250 / 80) + 1 = 5 frames

    def rc(n_utt=1, x_off=(0, 200), y_off=(0, 250), pos_off=(0, 5), h_pos=pos, hop=80, tol=50, x_d=x, y_d=y, d_d=d, win=True):
        r = wc.call(rt, n_utt, x_off, y_off, pos_off, h_pos, hop, tol, rt.ptr(x_d), rt.ptr(y_d), rt.ptr(d_d), win)
        return r, rt.lib.wh_last_error().decode()

    assert rc()[0] == 0 and rc(d_d=None)[0] == 0 and rc(n_utt=0)[0] == 0
    assert rc(hop=1024, tol=512, y_off=(0, 250), pos_off=(0, 2), h_pos=[0, 0])[0] == 0
    bad = {
        "hop 0": dict(hop=0), "hop too large": dict(hop=1025, pos_off=(0, 2), h_pos=[0, 0]),
        "tolerance negative": dict(tol=-1), "tolerance too large": dict(tol=513),
        "x offsets decrease": dict(x_off=(200, 0)), "y offsets decrease": dict(y_off=(250, 0)),
        "position offsets decrease": dict(pos_off=(5, 0)), "negative offset": dict(x_off=(-1, 200)),
        "a list of another length": dict(pos_off=(0, 4), h_pos=pos[:4]), "a list too long": dict(pos_off=(0, 6), h_pos=pos + [0]),
        "frames for no output": dict(y_off=(0, 0)),
        "negative count": dict(n_utt=-1), "null x": dict(x_d=None), "null y": dict(y_d=None), "null window": dict(win=False),
        "null positions": dict(h_pos=None), "null offsets": dict(x_off=None),
    }
    for name, kw in bad.items():
        r, msg = rc(**kw)
        assert r != 0 and msg.startswith("wh_wsola"), (name, r, msg)
    assert rt.lib.wh_wsola(None, None, 0, None, None, None, None, 80, 50, None, None, None, None) != 0
    assert rt.take_flags() == [0] * 16
