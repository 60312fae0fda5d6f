"""GPU: wh_spectral_filter (csrc/wh_specfilter.hip) through the C ABI and through world.specfilter, against
tests/_specfilter_reference.py at the smallest shapes that reach every edge (tests/_specfilter_cases.py): every transform
length (the run form and the one-row form), hops 1, 80 and N / 2, window counts around the run length at the shortest and
the longest utterance that has them, ragged batches with a one-frame and an empty utterance, both kinds with and without
a denominator, every order, row maps that are not monotone.

Bounds (tests/_specfilter_reference.py): relative RMS 1e-9, the bound tests/test_hip_requiem.py holds this chain to, and
per sample 8 x the worst value measured on an MI355X over the case list, relative to max|y|.  Every run prints the worst
figures it saw (test_cases_match_the_reference, test_unit_gain_returns_the_recording)."""
import numpy as np
import pytest

import _specfilter_cases as sc
import _specfilter_reference as sref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    from world import _hip
    return _hip.Runtime.get()


@pytest.mark.parametrize("case", sc.all_cases(), ids=lambda c: c.name)
def test_cases_match_the_reference(rt, case):
    got = sc.run(rt, case)
    bad, rms, worst = sc.compare_case(case, got)
    print("specfilter %-40s relative RMS %.3g  worst sample / max|y| %.3g" % (case.name, rms, worst))
    assert bad == []
    assert rt.take_flags() == [0] * 16


def test_bitwise_repeatable_and_alone_equals_in_batch(rt):
    astride = tuple(c for c in sc.kind_cases() if c.name.startswith("hops astride"))  # run form and one-row form in one call
    assert len(astride) == 2
    for case in (sc.geometry_cases()[1], sc.geometry_cases()[5], sc.kind_cases()[0], sc.kind_cases()[1], sc.kind_cases()[-2]) + astride:
        first = sc.run(rt, case)
        again = sc.run(rt, case)
        assert first["rc"] == 0 and again["rc"] == 0
        for a, b in zip(first["y"], again["y"]):
            assert a.tobytes() == b.tobytes(), case.name
        for u in range(len(case.nys)):
            alone = sc.run(rt, case, only=u)
            assert alone["rc"] == 0 and alone["guards"]
            assert alone["y"][0].tobytes() == first["y"][u].tobytes(), (case.name, u)


def test_unit_gain_returns_the_recording(rt):
    """h = 0: num == den (spectrum), a spectrogram of ones without den, the same LSF rows on both sides."""
    from world import specfilter

    worst = 0.0
    rng = np.random.RandomState(5)
    for n, hop, ny in ((512, 1, 40), (512, 256, 1500), (1024, 80, 1234), (1024, 110, 2000), (2048, 240, 3000), (4096, 480, 2500)):
        x = rng.randn(ny)
        f = sref.n_windows(ny, hop)
        spec = np.exp(rng.randn(f, n // 2 + 1))
        rows = sc.lsf_rows(f, 40, rng)
        x_d = rt.to_device(x)
        wmap = [np.minimum(np.arange(f), f - 1).astype(np.int32)]
        for num, den, kind in ((spec, spec, "spectrum"), (np.ones_like(spec), None, "spectrum"), (rows, rows, "lsf")):
            y = specfilter.filter_device(rt, x_d, [0, ny], 16000, 5, n, rt.to_device(num), None if den is None else rt.to_device(den),
                                         kind=kind, hop=hop, window_map=wmap).cpu().numpy()
            worst = max(worst, float(np.max(np.abs(y - x)) / np.max(np.abs(x))))
    print("specfilter unit gain: worst |y - x| / max|x| %.3g" % worst)
    assert worst <= sref.UNIT_BOUND
    assert rt.take_flags() == [0] * 16


def test_nan_stays_inside_its_windows(rt):
    """A NaN in gain row r reaches the samples [s_w, s_w + N) of the windows with map[w] == r, bit for bit nothing else, and
    no other utterance."""
    case = sc.Case("nan", 1024, "spectrum", True, 0, (80, 80), (2000, 600), (26, 9), "identity", 1, 200)
    clean = sc.run(rt, case)
    num = np.array(sc.inputs(case)["num"])
    num[10, 37] = np.nan  # row 10 of utterance 0: window 10 alone uses it
    got = sc.run(rt, case, num=num)
    assert clean["rc"] == 0 and got["rc"] == 0 and got["guards"]
    s = 10 * 80 - 80
    mask = np.zeros(2000, dtype=bool)
    mask[s:s + 1024] = True
    assert np.array_equal(np.isnan(got["y"][0]), mask)
    assert got["y"][0][~mask].tobytes() == clean["y"][0][~mask].tobytes()
    assert got["y"][1].tobytes() == clean["y"][1].tobytes()
    # the one-row form, a non-positive entry and kind lsf: the same containment
    case = sc.Case("nan lsf", 2048, "lsf", True, 24, (240, 240), (3000, 500), (14, 4), "identity", 0, 201)
    clean = sc.run(rt, case)
    num = np.array(sc.inputs(case)["num"])
    num[3, 0] = np.nan  # log E of row 3
    got = sc.run(rt, case, num=num)
    mask = np.zeros(3000, dtype=bool)
    mask[3 * 240 - 240:3 * 240 - 240 + 2048] = True
    assert np.array_equal(np.isnan(got["y"][0]), mask)
    assert got["y"][0][~mask].tobytes() == clean["y"][0][~mask].tobytes()
    assert got["y"][1].tobytes() == clean["y"][1].tobytes()
    rt.take_flags()


def test_argument_errors(rt):
    from world import specfilter

    n, k = 1024, 513
    num = rt.to_device(np.ones((4, k)))
    rows = rt.to_device(sc.lsf_rows(4, 24, np.random.RandomState(1)))
    x = rt.to_device(np.ones(200))
    y = rt.empty((200,))
    wmap = [0, 1, 2, 3]  # ceil(200 / 80) + 1 = 4 windows

    def rc(n_utt=1, x_off=(0, 200), frame_off=(0, 4), map_off=(0, 4), h_map=wmap, hops=(80,), kind=0, num_d=num, ldn=k, den_d=None,
           ldd=0, width=k, fft_size=n, x_d=x, y_d=y, cos=True):
        r = sc.call(rt, n_utt, x_off, frame_off, map_off, h_map, hops, kind, rt.ptr(num_d), ldn, rt.ptr(den_d), ldd, width, fft_size,
                    rt.ptr(x_d), rt.ptr(y_d), cos)
        return r, rt.lib.wh_last_error().decode()

    assert rc()[0] == 0
    assert rc(kind=1, num_d=rows, ldn=25, width=24)[0] == 0
    bad = {
        "2H - 1 > N": dict(hops=(513,), map_off=(0, 2), h_map=[0, 0]),
        "hop 0": dict(hops=(0,)),
        "map entry too large": dict(h_map=[0, 1, 2, 4]),
        "map entry negative": dict(h_map=[0, -1, 2, 3]),
        "map of another length": dict(map_off=(0, 3), h_map=[0, 1, 2]),
        "odd p": dict(kind=1, num_d=rows, ldn=25, width=23),
        "p too large": dict(kind=1, num_d=rows, ldn=25, width=66),
        "ld below a row": dict(kind=1, num_d=rows, ldn=24, width=24),
        "ldd below a row": dict(den_d=num, ldd=k - 1),
        "bins of another transform": dict(width=257),
        "fft_size not a power of two": dict(fft_size=1000, width=501),
        "fft_size too small": dict(fft_size=256, width=129),
        "fft_size too large": dict(fft_size=8192, width=4097),
        "kind": dict(kind=2),
        "null num": dict(num_d=None),
        "null x": dict(x_d=None),
        "null y": dict(y_d=None),
        "null bin table": dict(kind=1, num_d=rows, ldn=25, width=24, cos=False),
        "negative count": dict(n_utt=-1),
        "offsets decrease": dict(x_off=(200, 0)),
    }
    for name, kw in bad.items():
        r, msg = rc(**kw)
        assert r != 0 and msg.startswith("wh_spectral_filter"), (name, r, msg)
    assert rt.lib.wh_spectral_filter(None, None, 0, None, None, None, None, None, 0, None, 0, None, 0, k, None, n, None, None) != 0
    # the Python layer: mismatched orders, a map entry out of range, a bad fft_size
    den24 = rows
    num40 = rt.to_device(sc.lsf_rows(4, 40, np.random.RandomState(2)))
    with pytest.raises(ValueError):
        specfilter.filter_device(rt, x, [0, 200], 16000, 5, n, num40, den24, kind="lsf")
    with pytest.raises(ValueError):
        specfilter.filter_device(rt, x, [0, 200], 16000, 5, n, num, window_map=[[0, 1, 2, 7]])
    with pytest.raises(ValueError):
        specfilter.filter_device(rt, x, [0, 200], 16000, 5, 1000, num)
    with pytest.raises(ValueError):
        specfilter.filter_device(rt, x, [0, 200], 16000, 5, n, num, hop=600)
    assert rt.take_flags() == [0] * 16


def test_default_map_follows_the_frame_times(rt):
    """filter_device's default hop and map at 22.05 kHz (the period is 110.25 samples) against the reference with the
    reference's own map; the map leaves the identity inside the utterance."""
    from world import specfilter

    fs, n, ny = 22050, 1024, 27000
    rng = np.random.RandomState(9)
    f = 246
    x = rng.randn(ny)
    num, den = np.exp(0.3 * rng.randn(f, 513)), np.exp(0.3 * rng.randn(f, 513))
    wmap = sref.window_map(ny, f, 110, fs, 5)
    assert specfilter.default_hop(fs, 5) == 110 and np.any(wmap != np.minimum(np.arange(len(wmap)), f - 1))
    y = specfilter.filter_device(rt, rt.to_device(x), [0, ny], fs, 5, n, rt.to_device(num), rt.to_device(den)).cpu().numpy()
    assert sref.compare(y, sref.filter_spectrum(x, num, den, wmap, 110, n)) == []
