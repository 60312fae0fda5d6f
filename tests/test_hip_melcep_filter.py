"""GPU: wh_melcep_filter (csrc/wh_specfilter.hip, kind 2) through the C ABI and through world.melcep, against
tests/_melcep_reference.py at the smallest shapes that reach every edge (tests/_melcep_cases.py): every transform length
(the run form and the one-row form), hops 1, 80 and N / 2, window counts around the run length at the shortest and the
longest utterance that has them, every order and alpha with and without a denominator, ragged batches with a one-frame and
an empty utterance, row maps that are not monotone, hops on both sides of the run form in one call.

Bounds: relative RMS 1e-9 (tests/_specfilter_reference.RMS_BOUND, the suite's bound for this chain) and per sample 8 x
the worst value measured on an MI355X over the case list, relative to max|y| (tests/_melcep_reference.SAMPLE_BOUND).
Every run prints the worst figures it saw."""
import numpy as np
import pytest

import _melcep_cases as mc
import _melcep_reference as mref
import _specfilter_reference as sref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    from world import _hip
    return _hip.Runtime.get()


@pytest.mark.parametrize("case", mc.all_cases(), ids=lambda c: c.name)
def test_cases_match_the_reference(rt, case):
    got = mc.run(rt, case)
    bad, rms, worst = mc.compare_case(case, got)
    print("melcep filter %-40s relative RMS %.3g  worst sample / max|y| %.3g" % (case.name, rms, worst))
    assert bad == []
    assert rt.take_flags() == [0] * 16


def test_bitwise_repeatable_and_alone_equals_in_batch(rt):
    astride = tuple(c for c in mc.kind_cases() if c.name.startswith("hops astride"))  # run form and one-row form in one call
    assert len(astride) == 2
    for case in (mc.geometry_cases()[1], mc.geometry_cases()[5], mc.geometry_cases()[7], mc.kind_cases()[0], mc.kind_cases()[1]) + astride:
        first = mc.run(rt, case)
        again = mc.run(rt, case)
        assert first["rc"] == 0 and again["rc"] == 0
        for a, b in zip(first["y"], again["y"]):
            assert a.tobytes() == b.tobytes(), case.name
        for u in range(len(case.nys)):
            alone = mc.run(rt, case, only=u)
            assert alone["rc"] == 0 and alone["guards"]
            assert alone["y"][0].tobytes() == first["y"][u].tobytes(), (case.name, u)


def test_zero_rows_return_the_recording(rt):
    """d = 0: num == den, and rows of zeros without den."""
    from world import melcep

    worst = 0.0
    rng = np.random.RandomState(5)
    for n, hop, ny, m in ((512, 1, 40, 1), (512, 256, 1500, 24), (1024, 80, 1234, 39), (1024, 110, 2000, 64), (2048, 240, 3000, 59),
                          (4096, 480, 2500, 24)):
        x = rng.randn(ny)
        f = sref.n_windows(ny, hop)
        rows = mref.random_rows(rng, f, m)
        x_d = rt.to_device(x)
        wmap = [np.arange(f).astype(np.int32)]
        for num, den in ((rows, rows), (np.zeros_like(rows), None)):
            y = melcep.filter_device(rt, x_d, [0, ny], 16000, 5, n, rt.to_device(num), None if den is None else rt.to_device(den),
                                     hop=hop, window_map=wmap).cpu().numpy()
            worst = max(worst, float(np.max(np.abs(y - x)) / np.max(np.abs(x))))
    print("melcep filter zero rows: worst |y - x| / max|x| %.3g" % worst)
    assert worst <= sref.UNIT_BOUND
    assert rt.take_flags() == [0] * 16


def test_nan_stays_inside_its_windows(rt):
    """A NaN in row r reaches the samples [s_w, s_w + N) of the windows with map[w] == r, bit for bit nothing else, and no
    other utterance: the run form, then the one-row form with the NaN in c[0]."""
    for case, row, col, hop, n in ((mc.Case("nan", 1024, 24, 0.42, True, (80, 80), (2000, 600), (26, 9), "identity", 1, 200), 10, 17, 80, 1024),
                                   (mc.Case("nan one-row", 2048, 59, 0.554, False, (240, 240), (3000, 500), (14, 4), "identity", 0, 201),
                                    3, 0, 240, 2048)):
        clean = mc.run(rt, case)
        num = np.array(mc.inputs(case)["num"])
        num[row, col] = np.nan  # a row of utterance 0: window `row` alone uses it
        got = mc.run(rt, case, num=num)
        assert clean["rc"] == 0 and got["rc"] == 0 and got["guards"]
        s = row * hop - hop
        mask = np.zeros(case.nys[0], dtype=bool)
        mask[s:s + n] = True
        assert np.array_equal(np.isnan(got["y"][0]), mask)
        assert got["y"][0][~mask].tobytes() == clean["y"][0][~mask].tobytes()
        assert got["y"][1].tobytes() == clean["y"][1].tobytes()
    rt.take_flags()


def test_argument_errors(rt):
    n, m = 1024, 24
    num = rt.to_device(np.zeros((4, m + 1)))
    x = rt.to_device(np.ones(200))
    y = rt.empty((200,))
    wmap = [0, 1, 2, 3]  # ceil(200 / 80) + 1 = 4 windows

    def rc(n_utt=1, x_off=(0, 200), frame_off=(0, 4), map_off=(0, 4), h_map=wmap, hops=(80,), num_d=num, ldn=m + 1, den_d=None, ldd=0,
           order=m, fft_size=n, x_d=x, y_d=y, tables=(True, True)):
        r = mc.call(rt, n_utt, x_off, frame_off, map_off, h_map, hops, rt.ptr(num_d), ldn, rt.ptr(den_d), ldd, order, 0.42, fft_size,
                    rt.ptr(x_d), rt.ptr(y_d), tables)
        return r, rt.lib.wh_last_error().decode()

    assert rc()[0] == 0
    assert rc(den_d=num, ldd=m + 1)[0] == 0
    assert rc(order=1)[0] == 0
    bad = {
        "order 0": dict(order=0),
        "order 65": dict(order=65),
        "negative order": dict(order=-1),
        "null cosine table": dict(tables=(False, True)),
        "null sine table": dict(tables=(True, False)),
        "ld below a row": dict(ldn=m),
        "ldd below a row": dict(den_d=num, ldd=m),
        "2H - 1 > N": dict(hops=(513,), map_off=(0, 2), h_map=[0, 0]),
        "hop 0": dict(hops=(0,)),
        "map entry too large": dict(h_map=[0, 1, 2, 4]),
        "map entry negative": dict(h_map=[0, -1, 2, 3]),
        "map of another length": dict(map_off=(0, 3), h_map=[0, 1, 2]),
        "fft_size not a power of two": dict(fft_size=1000),
        "fft_size too small": dict(fft_size=256),
        "fft_size too large": dict(fft_size=8192),
        "null num": dict(num_d=None),
        "null x": dict(x_d=None),
        "null y": dict(y_d=None),
        "negative count": dict(n_utt=-1),
        "offsets decrease": dict(x_off=(200, 0)),
    }
    before = y.clone()
    for name, kw in bad.items():
        r, msg = rc(**kw)
        assert r != 0 and msg.startswith("wh_melcep_filter"), (name, r, msg)
    assert rt.torch.equal(before, y)  # refused before any launch
    assert rt.lib.wh_melcep_filter(None, None, 0, None, None, None, None, None, None, 0, None, 0, m, None, None, n, None, None) != 0
    # wh_spectral_filter keeps refusing kind 2
    import _specfilter_cases as sc
    assert sc.call(rt, 1, (0, 200), (0, 4), (0, 4), wmap, (80,), 2, rt.ptr(num), m + 1, None, 0, m, n, rt.ptr(x), rt.ptr(y)) != 0
    assert rt.lib.wh_last_error().decode().startswith("wh_spectral_filter")
    assert rt.take_flags() == [0] * 16


@pytest.mark.parametrize("case", (mc.geometry_cases()[4], mc.geometry_cases()[7], mc.kind_cases()[2], mc.kind_cases()[7]), ids=lambda c: c.name)
def test_agrees_with_kind_0_on_the_decoded_envelopes(rt, case):
    """wh_melcep_filter against wh_spectral_filter kind 0 fed the envelopes that spectrum_device decodes from the same
    rows: relative RMS within 2e-9 (either filter's bound against its own reference) plus the gap between the two
    references that the CPU measured (tests/_melcep_reference.FOLD_GAP_BOUND)."""
    from world import melcep, specfilter

    inp = mc.inputs(case)
    num, den = rt.to_device(inp["num"]), None if inp["den"] is None else rt.to_device(inp["den"])
    x_d = rt.to_device(np.concatenate(inp["x"]))
    kw = dict(frame_off=inp["frame_off"], hop=list(case.hops), window_map=list(inp["maps"]))
    closed = melcep.filter_device(rt, x_d, inp["x_off"], 16000, 5, case.n, num, den, case.alpha, **kw).cpu().numpy()
    sp_num = melcep.spectrum_device(rt, num, case.n, case.alpha)
    sp_den = None if den is None else melcep.spectrum_device(rt, den, case.n, case.alpha)
    folded = specfilter.filter_device(rt, x_d, inp["x_off"], 16000, 5, case.n, sp_num, sp_den, **kw).cpu().numpy()
    worst = 0.0
    for u in range(len(case.nys)):
        a, b = inp["x_off"][u], inp["x_off"][u + 1]
        worst = max(worst, sref.errors(closed[a:b], folded[a:b])[0])
    print("melcep filter against kind 0 %-32s relative RMS %.3g" % (case.name, worst))
    assert worst <= 2 * sref.RMS_BOUND + mref.FOLD_GAP_BOUND
    assert rt.take_flags() == [0] * 16


def test_the_facade_filters_like_the_reference(rt):
    """World.filter_waveform_melcep at 22.05 kHz (the period is 110.25 samples: the default map leaves the identity) against
    the reference with the reference's own map."""
    from world.main import World

    fs, n, ny, m = 22050, 1024, 9000, 24
    rng = np.random.RandomState(9)
    f = 82
    x = rng.randn(ny)
    num, den = mref.random_rows(rng, f, m), mref.random_rows(rng, f, m)
    wmap = sref.window_map(ny, f, 110, fs, 5)
    y = World().filter_waveform_melcep(fs, x, num, den, fft_size=n)
    assert mc.compare(y, mref.filter_melcep(x, num, den, wmap, 110, n, 0.45)) == []
