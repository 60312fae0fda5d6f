"""GPU: wh_psola (csrc/wh_psola.hip) through the C ABI, bit for bit against tests/_psola_reference.py — y, the analysis
marks and their periods, the synthesis marks, the selection, the flips and both counts, each between guard values — at the
smallest shapes that reach every edge (tests/_psola_cases.py): the periods 2, 3, 63 .. 65, 255 .. 257 and 2048, constant
and mixed; tolerances 0, 1, 127 | 128 and 512 at P = 2048 (1025 candidates on 256 threads) and 15 | 16 | 17 at P = 65;
grids 1, 16 and 4096; unvoiced hops 1, 80 and 2048; pmin and smin free and binding; norm 0 and 1; utterances that are
empty, one sample long and shorter than a period, outputs of one sample and of none; stretches by 0.5 and 2; a source map
that is constant, decreasing, beyond both ends and at the ends of the int64 range; track entries that are negative, 1 or
above 2048; target 2048 against analysis 20 and the reverse; noise, a tone, digital silence, periodic integers whose scores
tie, silence next to signal, a NaN and an Inf that stay inside their utterance; a ragged batch of eight; repeated runs; an
utterance alone against itself in its batch; the optional outputs NULL."""
import numpy as np
import pytest

import _psola_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    from world import _hip
    return _hip.Runtime.get()


@pytest.mark.parametrize("case", pc.all_cases(), ids=lambda c: c.name)
def test_cases_match_the_reference_bit_for_bit(rt, case):
    got = pc.run(rt, case)
    assert pc.compare_case(case, got) == []
    assert rt.take_flags() == [0] * 16


@pytest.mark.parametrize("case", pc.all_cases(), ids=lambda c: c.name)
def test_bitwise_repeatable_alone_equals_in_batch_and_outputs_may_be_null(rt, case):
    """Every case twice, with the optional outputs NULL, with capacity to spare, and every utterance of it again alone."""
    first, again, quiet, roomy = pc.run(rt, case), pc.run(rt, case), pc.run(rt, case, want_marks=False), pc.run(rt, case, slack=5)
    assert first["rc"] == 0 and again["rc"] == 0 and quiet["rc"] == 0 and quiet["guards"] and roomy["rc"] == 0 and roomy["guards"]
    for u in range(len(case.utts)):
        alone = pc.run(rt, case, only=u)
        assert alone["rc"] == 0 and alone["guards"]
        assert first["y"][u].tobytes() == quiet["y"][u].tobytes(), u
        for k in pc.FIELDS:
            assert first[k][u].tobytes() == again[k][u].tobytes() == roomy[k][u].tobytes() == alone[k][0].tobytes(), (u, k)
    assert rt.take_flags() == [0] * 16


@pytest.mark.parametrize("what", ["nan", "inf"])
def test_a_nan_or_inf_stays_inside_its_utterance(rt, what):
    speech = ("runs", ((0, 57, 64, 71, 80), 6))
    utts = lambda kind: (("tone", 900, 1.25, speech, speech, ("ratio", None)), (kind, 700, 0.8, speech, ("const", 60), ("ratio", None)),
                         ("noise", 500, 1.5, speech, speech, ("ratio", None)))
    case, clean = pc.Case(what, pc.P(16, 80, 50, 2, 1, 1), utts(what), 300), pc.Case("clean", pc.P(16, 80, 50, 2, 1, 1), utts("noise"), 300)
    got, ref = pc.run(rt, case), pc.run(rt, clean)
    assert pc.compare_case(case, got) == [] and ref["rc"] == 0
    assert not np.all(np.isfinite(pc.inputs(case)["x"][1]))
    for u in (0, 2):  # the neighbours' bits are those of the batch without it
        assert np.array_equal(pc.inputs(case)["x"][u], pc.inputs(clean)["x"][u])
        for k in pc.FIELDS:
            assert got[k][u].tobytes() == ref[k][u].tobytes(), (u, k)
    # an utterance of nothing but NaN: every shift is 0, so the marks are the periods' own
    x = [pc.inputs(case)["x"][0], np.full(700, np.nan), pc.inputs(case)["x"][2]]
    got = pc.run(rt, case, xs=x)
    assert got["rc"] == 0 and got["guards"] and np.all(np.isnan(got["y"][1][100:400]))
    steps, per = np.diff(got["marks"][1]), got["periods"][1][:-1]
    assert np.array_equal(steps, np.where(per > 0, per, 80))
    for u in (0, 2):
        assert got["y"][u].tobytes() == ref["y"][u].tobytes()
    assert rt.take_flags() == [0] * 16


def test_argument_errors(rt):
    p = pc.P(16, 80, 50, 2, 1, 1)
    n, n_out = 200, 250
    x, y = rt.to_device(np.ones(n)), rt.empty((n_out,))
    torch = rt.torch
    pa = torch.full((n // 16 + 1,), 64, dtype=torch.int32, device=rt.device)
    ps = torch.full((n_out // 16 + 1,), 50, dtype=torch.int32, device=rt.device)
    src = torch.arange(n_out // 16 + 1, dtype=torch.int64, device=rt.device) * 12
    cap_a, cap_s = pc.pref.mark_capacity(n, p), pc.pref.smark_capacity(n_out, p)
    assert (cap_a, cap_s) == (101, 251)

    def rc(n_utt=1, x_off=(0, n), y_off=(0, n_out), pa_off=(0, n // 16 + 1), ps_off=(0, n_out // 16 + 1), mark_off=(0, cap_a),
           smark_off=(0, cap_s), params=p, x_d=x, pa_d=pa, ps_d=ps, src_d=src, y_d=y):
        r = pc.call(rt, n_utt, x_off, y_off, pa_off, ps_off, mark_off, smark_off, params, rt.ptr(x_d), rt.ptr(pa_d), rt.ptr(ps_d),
                    rt.ptr(src_d), rt.ptr(y_d))
        return r, rt.lib.wh_last_error().decode()

    assert rc()[0] == 0 and rc(n_utt=0)[0] == 0 and rc(mark_off=(0, cap_a + 3), smark_off=(3, cap_s + 9))[0] == 0
    assert rc(params=pc.P(4096, 2048, 512, 2048, 2048, 0), pa_off=(0, 1), ps_off=(0, 1))[0] == 0
    bad = {
        "grid 0": dict(params=p._replace(grid=0)), "grid too large": dict(params=p._replace(grid=4097), pa_off=(0, 1), ps_off=(0, 1)),
        "hop 0": dict(params=p._replace(hop=0)), "hop too large": dict(params=p._replace(hop=2049)),
        "tolerance negative": dict(params=p._replace(tol=-1)), "tolerance too large": dict(params=p._replace(tol=513)),
        "pmin 1": dict(params=p._replace(pmin=1)), "pmin too large": dict(params=p._replace(pmin=2049)),
        "smin 0": dict(params=p._replace(smin=0)), "smin too large": dict(params=p._replace(smin=2049)),
        "norm 2": dict(params=p._replace(norm=2)), "norm negative": dict(params=p._replace(norm=-1)),
        "x offsets decrease": dict(x_off=(n, 0)), "y offsets decrease": dict(y_off=(n_out, 0)), "negative offset": dict(x_off=(-1, n - 1)),
        "analysis track too short": dict(pa_off=(0, n // 16)), "analysis track too long": dict(pa_off=(0, n // 16 + 2)),
        "target tracks too short": dict(ps_off=(0, n_out // 16)), "mark capacity too small": dict(mark_off=(0, cap_a - 1)),
        "synthesis capacity too small": dict(smark_off=(0, cap_s - 1)), "mark offsets decrease": dict(mark_off=(cap_a, 0)),
        "negative count": dict(n_utt=-1), "null x": dict(x_d=None), "null y": dict(y_d=None), "null per_a": dict(pa_d=None),
        "null per_s": dict(ps_d=None), "null src": dict(src_d=None), "null offsets": dict(x_off=None), "null capacities": dict(smark_off=None),
    }
    for name, kw in bad.items():
        r, msg = rc(**kw)
        assert r != 0 and msg.startswith("wh_psola"), (name, r, msg)
    assert rt.lib.wh_psola(None, None, 0, None, None, None, None, None, None, 16, 80, 50, 2, 1, 1, *([None] * 12)) != 0
    assert rt.take_flags() == [0] * 16
