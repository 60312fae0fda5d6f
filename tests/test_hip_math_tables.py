"""GPU: the table-driven log / exp / sincospi of the spectral kernels (csrc/wh_math.h: tlog, texp, tsincospi, through
wh_math_probe's codes 3, 4, 5) at the inputs and bounds of tests/test_hip_math.py: a few ulp over the ranges the kernels feed
them and far beyond, special values passed through, and no input that takes a table index out of range."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LOG, EXP, SINCOSPI = 3, 4, 5


def _probe(which, x):
    from world import _hip

    rt = _hip.Runtime.get()
    x_d = rt.to_device(np.ascontiguousarray(x, dtype=np.float64))
    out = rt.empty((len(x) * (2 if which == SINCOSPI else 1),))
    _hip.check(rt.lib.wh_math_probe(rt.ctx, rt.stream(), which, rt.ptr(x_d), rt.ptr(out), len(x)))
    return out.cpu().numpy()


def test_tlog():
    rng = np.random.RandomState(1)
    x = np.concatenate([10 ** rng.uniform(-300, 300, 400000), 1 + rng.uniform(-1e-3, 1e-3, 100000), rng.uniform(0.5, 2.0, 100000),
                        [1.0, 2.0, 0.5, np.e, 2.2250738585072014e-308, 5e-324, 1.7976931348623157e308, 0.7071067811865476, 1.4142135623730951]])
    got, ref = _probe(LOG, x), np.log(x)
    err = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)
    print("tlog: worst relative error %.3g" % np.max(err[ref != 0]))
    assert np.max(err[ref != 0]) < 5e-16
    assert got[x == 1.0][0] == 0.0
    sp = _probe(LOG, np.array([0.0, -1.0, np.inf, np.nan]))
    assert sp[0] == -np.inf and np.isnan(sp[1]) and sp[2] == np.inf and np.isnan(sp[3])


def test_tlog_next_to_the_nodes():
    """Both sides of every midpoint between two nodes (where the node changes and |r| is largest) and the nodes themselves,
    at every binade parity: the relative error holds where log m is small (around the exact node c = 1) too."""
    mid = (np.arange(90, 183) + 0.5) / 128
    m = np.concatenate([np.nextafter(mid, 0), mid, np.nextafter(mid, 2), np.arange(90, 183) / 128.0])
    m = m[(m > 0.70) & (m < 1.42)]
    x = np.concatenate([m, m * 2.0 ** -1022, m * 2.0 ** 1000, m * 2.0 ** -3])
    got, ref = _probe(LOG, x), np.log(x.astype(np.longdouble))
    err = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)
    print("tlog at the nodes: worst relative error %.3g" % float(np.max(err[ref != 0])))
    assert np.max(err[ref != 0]) < 5e-16


def test_texp():
    rng = np.random.RandomState(2)
    x = np.concatenate([rng.uniform(-700, 700, 400000), rng.uniform(-1, 1, 100000), rng.uniform(-1e-8, 1e-8, 1000), [0.0, 1.0, -1.0, 709.0, -745.0]])
    got, ref = _probe(EXP, x), np.exp(x)
    ok = ref > 1e-300  # (denormal results round differently; nothing in the kernels gets near)
    print("texp: worst relative error %.3g" % np.max(np.abs(got[ok] - ref[ok]) / ref[ok]))
    assert np.max(np.abs(got[ok] - ref[ok]) / ref[ok]) < 5e-16
    assert got[x == 0.0][0] == 1.0
    sp = _probe(EXP, np.array([800.0, -800.0, np.inf, -np.inf, np.nan, 1e12, -1e12]))
    assert sp[0] == np.inf and sp[1] == 0.0 and sp[2] == np.inf and sp[3] == 0.0 and np.isnan(sp[4]) and sp[5] == np.inf and sp[6] == 0.0


def test_tsincospi():
    rng = np.random.RandomState(3)
    x = np.concatenate([rng.uniform(-4, 4, 400000), rng.uniform(-1e6, 1e6, 100000), np.arange(-8, 9) * 0.25, rng.uniform(-1e-9, 1e-9, 1000)])
    got = _probe(SINCOSPI, x).reshape(-1, 2)
    # reference in extended precision on the reduced argument (np.sin(pi * x) loses the digits of large x)
    r = (x - 2 * np.round(0.5 * x)).astype(np.longdouble)
    pi_l = np.longdouble("3.14159265358979323846264338327950288")
    ref_s, ref_c = np.sin(pi_l * r), np.cos(pi_l * r)
    es, ec = np.max(np.abs(got[:, 0] - ref_s.astype(np.float64))), np.max(np.abs(got[:, 1] - ref_c.astype(np.float64)))
    print("tsincospi: worst absolute error sin %.3g cos %.3g" % (es, ec))
    assert es < 3e-16
    assert ec < 3e-16
    exact = _probe(SINCOSPI, np.array([0.0, 0.5, 1.0, 1.5, 2.0, -0.5])).reshape(-1, 2)
    assert np.max(np.abs(exact - np.array([[0, 1], [1, 0], [0, -1], [-1, 0], [0, 1], [-1, 0]]))) == 0.0
    sp = _probe(SINCOSPI, np.array([np.nan, np.inf, -np.inf])).reshape(-1, 2)
    assert np.isnan(sp).all()


def test_every_input_returns():
    """Values that take a careless table index anywhere: every call returns, finite where the function is defined."""
    x = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, 1e300, -1e300, 1.7976931348623157e308, -1.7976931348623157e308,
                  np.inf, -np.inf, np.nan, 2.0 ** 31, -2.0 ** 31, 2.0 ** 52, 2.0 ** 53, 2.0 ** 63, -2.0 ** 63, 4503599627370497.0])
    lg, ex, sc = _probe(LOG, x), _probe(EXP, x), _probe(SINCOSPI, x).reshape(-1, 2)
    assert np.isnan(lg[np.isnan(x)]).all() and np.isnan(ex[np.isnan(x)]).all() and np.isnan(sc[~np.isfinite(x)]).all()
    pos = np.isfinite(x) & (x > 0)
    assert np.isfinite(lg[pos]).all()
    assert np.array_equal(ex[np.isfinite(x) & (x > 710)], np.full(int(np.sum(np.isfinite(x) & (x > 710))), np.inf))
    assert np.array_equal(ex[x < -746], np.zeros(int(np.sum(x < -746))))
    small = np.abs(x) < 1.0
    assert np.max(np.abs(sc[small] - np.array([0.0, 1.0]))) < 1e-300
