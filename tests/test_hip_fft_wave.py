"""GPU: the wave-local transform engine (wh::fft_lds_wave, through wh_fft_probe) against numpy.fft at the shapes the
kernels run it: 512 points on the first wave of a 128- or 256-thread group in a 256-thread workgroup, and a one-wave
workgroup; forward and inverse (unnormalised)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 512


def _probe(x, gt, snt, inverse):
    from world import _hip

    rt = _hip.Runtime.get()
    flat = np.ascontiguousarray(np.stack([x.real, x.imag], axis=-1).reshape(-1), dtype=np.float64)
    x_d = rt.to_device(flat)
    out = rt.empty((len(flat),))
    _hip.check(rt.lib.wh_fft_probe(rt.ctx, rt.stream(), N, gt, snt, inverse, rt.ptr(x_d), rt.ptr(out), x.shape[0]))
    o = out.cpu().numpy().reshape(x.shape[0], N, 2)
    return o[..., 0] + 1j * o[..., 1]


@pytest.mark.parametrize("gt,snt", [(128, 256), (256, 256), (64, 64)])
@pytest.mark.parametrize("inverse", [0, 1])
def test_complex_against_numpy(gt, snt, inverse):
    rng = np.random.RandomState(gt + snt + inverse)
    x = rng.standard_normal((37, N)) + 1j * rng.standard_normal((37, N))  # an odd count: a half-filled last workgroup
    got = _probe(x, gt, snt, inverse)
    ref = np.fft.ifft(x, axis=1) * N if inverse else np.fft.fft(x, axis=1)
    rel = np.sqrt(np.mean(np.abs(got - ref) ** 2, axis=1) / np.mean(np.abs(ref) ** 2, axis=1))
    assert np.max(rel) < 1e-15, np.max(rel)


@pytest.mark.parametrize("gt,snt", [(128, 256), (256, 256)])
def test_real_input_and_round_trip(gt, snt):
    # real data (what every WORLD transform takes in): a Hermitian spectrum, and back to the input times N
    rng = np.random.RandomState(7)
    x = rng.standard_normal((9, N)).astype(np.complex128)
    fwd = _probe(x, gt, snt, 0)
    ref = np.fft.fft(x.real, axis=1)
    assert np.sqrt(np.mean(np.abs(fwd - ref) ** 2) / np.mean(np.abs(ref) ** 2)) < 1e-15
    back = _probe(fwd, gt, snt, 1) / N
    assert np.sqrt(np.mean(np.abs(back - x) ** 2) / np.mean(np.abs(x) ** 2)) < 1e-15


def test_bad_shape_is_refused():
    from world import _hip

    rt = _hip.Runtime.get()
    buf = rt.empty((2 * N,))
    assert rt.lib.wh_fft_probe(rt.ctx, rt.stream(), N, 128, 128, 0, rt.ptr(buf), rt.ptr(buf), 1) != 0
    assert rt.lib.wh_fft_probe(rt.ctx, rt.stream(), 1024, 128, 256, 0, rt.ptr(buf), rt.ptr(buf), 1) != 0
