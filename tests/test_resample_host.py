"""CPU: the host half of world.resample — the filter design (firwin, the zero pads, scipy's phase table h_trans_flip,
P, n_pre_remove) that wh_resample_poly evaluates.  Run through a NumPy restatement of upfirdn's loop (the kernel's
summation order: k ascending, taps outside the signal skipped, each product rounded on its own), it must give
scipy.signal.resample_poly bit for bit; the argument checks raise; and without a GPU the device call raises (no CPU
fallback)."""
import numpy as np
import pytest

scipy_signal = pytest.importorskip("scipy.signal")

from world import _hip  # noqa: E402
from world import resample as R  # noqa: E402

RATES = (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000)


def restated(x, up, down, window=('kaiser', 5.0)):
    """upfirdn's loop over the host design, vectorised across outputs, sequential across taps."""
    x = np.asarray(x, dtype=np.float64)
    d = R.design(up, down, len(x), window)
    P, npr, n_out, ph = d["P"], d["n_pre_remove"], d["n_out"], R.phases(d)
    j = np.arange(n_out, dtype=np.int64) + npr
    t = (j * d["down"]) % d["up"]
    xi = (j * d["down"]) // d["up"]
    acc = np.zeros(n_out)
    for m in range(P):
        k = xi - P + 1 + m
        ok = (k >= 0) & (k < len(x))
        acc = np.where(ok, acc + x[np.clip(k, 0, max(len(x) - 1, 0))] * ph[t, m], acc) if len(x) else acc
    return acc


def _signal(n, seed):
    rng = np.random.RandomState(seed)
    return rng.randn(n) * 0.3 + np.sin(np.arange(n) * 0.01)


@pytest.mark.parametrize("fs_in", RATES)
def test_design_reproduces_scipy_for_every_rate_pair(fs_in):
    for fs_out in RATES:
        if fs_out == fs_in:
            continue
        d = R.design(fs_out, fs_in, 1)
        for n in (1, 2, 37, max(1, d["P"] - 3), 4410):
            x = _signal(n, n + fs_in % 97)
            ref = scipy_signal.resample_poly(x, fs_out, fs_in)
            got = restated(x, fs_out, fs_in)
            assert got.shape == ref.shape and np.array_equal(got, ref), (fs_in, fs_out, n)


def test_design_matches_the_quoted_parameters():
    d = R.design(16000, 44100, 441000)
    assert (d["up"], d["down"], d["P"]) == (160, 441, 58)
    d = R.design(16000, 48000, 480000)
    assert (d["up"], d["down"], d["P"], d["n_pre_remove"]) == (1, 3, 64, 11)
    assert R.design(1280 * 7, 147 * 7, 10)["up"] == 1280  # reduced by the gcd


def test_non_finite_samples_follow_scipy():
    x = _signal(500, 3)
    x[[0, 17, 250, 499]] = [np.inf, np.nan, -np.inf, np.inf]
    for up, down in ((160, 441), (1, 3), (3, 1)):
        assert np.array_equal(restated(x, up, down), scipy_signal.resample_poly(x, up, down), equal_nan=True)


def test_explicit_fir_window_follows_scipy():
    x = _signal(300, 5)
    for fir in (np.hanning(31), np.array([0.25, 0.5, 0.25]), np.ones(1), scipy_signal.firwin(64, 0.3)):
        for up, down in ((2, 3), (3, 1), (1, 4)):
            ref = scipy_signal.resample_poly(x, up, down, window=fir)
            assert np.array_equal(restated(x, up, down, window=fir), ref), (len(fir), up, down)


def test_integer_input_is_float64_like_scipy():
    x = (np.arange(400) * 37 % 2001 - 1000).astype(np.int16)
    assert np.array_equal(restated(x, 2, 3), scipy_signal.resample_poly(x, 2, 3))


@pytest.mark.parametrize("bad", [
    dict(x=np.zeros(8, dtype=np.float32)),
    dict(x=np.zeros(8, dtype=np.complex128)),
    dict(padtype='mean'),
    dict(padtype='line'),
    dict(cval=1.0),
    dict(up=1.5),
    dict(up=0),
    dict(down=-2),
    dict(up=True),
    dict(up=4097, down=1),
    dict(x=np.zeros((2, 2, 2))),
])
def test_unsupported_arguments_raise(bad):
    kw = dict(x=np.zeros(8), up=2, down=3)
    kw.update(bad)
    with pytest.raises((ValueError, TypeError)):
        R.resample_poly(kw.pop("x"), kw.pop("up"), kw.pop("down"), **kw)


def test_identity_ratio_is_a_copy_like_scipy():
    x = np.arange(5, dtype=np.int16)
    y = R.resample_poly(x, 3, 3)
    assert y.dtype == np.int16 and np.array_equal(y, x) and y is not x


def test_device_call_without_gpu_has_no_cpu_fallback():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the device path is covered by tests/test_hip_resample.py")
    with pytest.raises(_hip.WorldHipError):
        R.resample_poly(np.ones(100), 160, 441)
