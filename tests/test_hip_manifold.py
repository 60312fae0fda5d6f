"""GPU: the manifold vocoder's networks on the device (wh_dense_stack, world.manifold, World.encode_vae / decode_vae,
BatchEncoding.vae / with_vae_spectrogram).  Random stacks against a NumPy FP64 forward; the reference's TIMIT networks
against tests/golden/golden_manifold.npz (the reference's encode_vae with Keras restated in float32: ours is FP64, so
the bar there is float32 rounding) and the two log-spectral distortions of the reference's own example; rows that are
independent of their batch; refusals that do not crash."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ENC = os.path.join(GOLDEN, "manifold_timit_vae_encoder.h5")
DEC = os.path.join(GOLDEN, "manifold_timit_vae_decoder.h5")
ACTS = {"linear": lambda v: v, "relu": lambda v: np.maximum(v, 0.0), "tanh": np.tanh,
        "sigmoid": lambda v: 1.0 / (1.0 + np.exp(-v))}


def forward(stack, x, window=0, seg=None, in_shift=None, out_cols=None, out_shift=None, tap=-1, tap_f32=False):
    """The FP64 NumPy forward of a stack, with get_context per segment and the shifts (main.py:360-379)."""
    x = np.asarray(x, dtype=np.float64)
    if in_shift is not None:
        x = x - in_shift
    n = x.shape[0]
    seg = [0, n] if seg is None else list(seg)
    rows = []
    for a, b in zip(seg[:-1], seg[1:]):
        idx = np.arange(a, b)
        rows += [np.concatenate([x[np.clip(i + j - window, a, b - 1)] for j in range(2 * window + 1)]) for i in idx]
    h = np.array(rows).reshape(n, -1)
    z = None
    for i, (w, bb, act) in enumerate(stack.layers()):
        h = ACTS[act](h @ w.astype(np.float64) + bb.astype(np.float64))
        if i == tap:
            if tap_f32:
                h = h.astype(np.float32).astype(np.float64)
            z = h
    if out_cols is not None:
        h = h[:, out_cols[0]:out_cols[0] + out_cols[1]]
    if out_shift is not None:
        h = h + out_shift
    return (z, h) if tap >= 0 else h


def relerr(got, ref):
    return float(np.max(np.abs(got - ref)) / max(np.max(np.abs(ref)), 1e-300))


def random_stack(rng, dims, acts):
    from world.manifold import DenseStack

    return DenseStack([(rng.randn(a, b) / np.sqrt(a), rng.randn(b) * 0.1, act)
                       for a, b, act in zip(dims[:-1], dims[1:], acts)])


@pytest.fixture(scope="module")
def rt():
    from world import _hip

    return _hip.Runtime.get()


def _run(rt, stack, x, **kw):
    from world.manifold import dense_stack_device

    r = dense_stack_device(rt, rt.to_device(np.ascontiguousarray(x)), stack, **kw)
    if isinstance(r, tuple):
        return tuple(t.cpu().numpy() for t in r)
    return r.cpu().numpy()


@pytest.mark.parametrize("acts", [("relu", "relu", "linear"), ("tanh", "sigmoid", "tanh"), ("sigmoid", "linear", "relu")])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 129])
def test_random_stacks_match_fp64_forward(rt, acts, n):
    rng = np.random.RandomState(n + 7 * len(acts[0]))
    for dims, window in (((39, 256, 12, 39), 0), ((39 * 5, 100, 256, 12), 2), ((12, 39, 17, 256), 0)):
        st = random_stack(rng, dims, acts)
        d = dims[0] // (2 * window + 1)
        x = rng.randn(n, d)
        mean = rng.randn(d)
        got = _run(rt, st, x, window=window, in_shift=mean)
        ref = forward(st, x, window=window, in_shift=mean)
        assert got.shape == ref.shape and relerr(got, ref) <= 1e-12, (dims, window, relerr(got, ref))


def test_large_batch_taps_and_windows(rt):
    rng = np.random.RandomState(5)
    st = random_stack(rng, (39 * 5, 256, 256, 12, 256, 39 * 5), ("relu", "tanh", "linear", "relu", "linear"))
    n = 100003
    x = rng.randn(n, 39)
    mean = rng.randn(39)
    seg = [0, 1, 2, 50000, 50000, 99990, n]
    z, y = _run(rt, st, x, window=2, seg_off=seg, in_shift=mean, out_cols=(78, 39), out_shift=mean, tap_layer=2)
    zr, yr = forward(st, x, window=2, seg=seg, in_shift=mean, out_cols=(78, 39), out_shift=mean, tap=2)
    assert relerr(z, zr) <= 1e-12 and relerr(y, yr) <= 1e-12


def test_a_row_is_independent_of_its_batch(rt):
    rng = np.random.RandomState(9)
    st = random_stack(rng, (39, 256, 256, 12), ("relu", "relu", "linear"))
    x = rng.randn(200, 39)
    full = _run(rt, st, x)
    for i in (0, 5, 31, 32, 33, 199):
        assert np.array_equal(_run(rt, st, x[i:i + 1]), full[i:i + 1])
        assert np.array_equal(_run(rt, st, x[i:]), full[i:])  # at every other tile position


def test_wide_input_in_chunks(rt):
    rng = np.random.RandomState(11)
    st = random_stack(rng, (2048, 64, 3), ("relu", "linear"))
    x = rng.randn(70, 2048)
    assert relerr(_run(rt, st, x), forward(st, x)) <= 1e-12


@pytest.fixture(scope="module")
def timit():
    from world.manifold import DenseStack

    return DenseStack.from_h5(ENC), DenseStack.from_h5(DEC)


def test_timit_on_the_stored_mcep(golden, timit):
    from world import main

    g = golden("manifold")
    enc, dec = timit
    mcep = g["mcep"].copy()
    xc = mcep[:, 1:40]
    zc, yc = main.World().encode_vae(xc, mcep[:, 0], ENC, DEC, window=0, n0=40, batch_size=256, mean=g["mean"])
    assert zc.dtype == np.float32 and zc.shape == g["zc"].shape
    assert yc.dtype == np.float64 and yc.shape == g["yc"].shape
    assert np.array_equal(xc, g["mcep"][:, 1:] - g["mean"])  # `Xc -= mean` on the caller's array, as the reference
    assert np.max(np.abs(zc - g["zc"])) <= 1e-4
    assert np.max(np.abs(yc - g["yc"])) <= 1e-4
    assert np.array_equal(yc[:, 0], g["mcep"][:, 0])
    zr, yr = forward(enc.then(dec), g["mcep"][:, 1:], in_shift=g["mean"], out_shift=g["mean"], tap=3, tap_f32=True)
    assert relerr(zc.astype(np.float64), zr) <= 1e-12
    assert relerr(yc[:, 1:], yr) <= 1e-12
    # the decoder alone on the returned latent gives the same bits (decode_vae: an extension)
    assert np.array_equal(main.World().decode_vae(zc, mcep[:, 0], DEC, 0, 40, g["mean"]), yc)
    # the three accepted forms of a network give the same result
    z2, y2 = main.World().encode_vae(g["mcep"][:, 1:].copy(), mcep[:, 0], enc, dec, 0, 40, 1, g["mean"])
    assert np.array_equal(z2, zc) and np.array_equal(y2, yc)


def _lsd(a, b):
    a = a / np.sqrt(np.mean(a ** 2, axis=1)).reshape(-1, 1)
    b = b / np.sqrt(np.mean(b ** 2, axis=1)).reshape(-1, 1)
    return np.mean(np.mean((20 * np.log10(a) - 20 * np.log10(b)) ** 2, axis=1) ** 0.5)


def test_end_to_end_lsd_of_the_reference_example(golden):
    from scipy.io import wavfile

    from world import main

    g = golden("manifold")
    fs, xi = wavfile.read(os.path.join(GOLDEN, "test-mwm.wav"))
    x = xi / (2 ** 15 - 1)
    W = main.World()
    data = W.encode(fs, x, f0_method="harvest")
    spec = np.asarray(data["spectrogram"]).T
    mcep = W.encode_mcep(spec, n0=40)
    assert abs(_lsd(W.decode_mcep(mcep, fft_size=1024), spec) - float(g["lsd_mcep"])) <= 2e-3
    m = np.mean(mcep[:, 1:], axis=0)
    zc, yc = W.encode_vae(mcep[:, 1:40], mcep[:, 0], ENC, DEC, window=0, n0=40, batch_size=256, mean=m)
    assert zc.shape == (len(mcep), 12)
    got = _lsd(W.decode_mcep(yc, fft_size=1024), spec)
    assert abs(got - float(g["lsd_vae"])) <= 2e-3, got


def test_ragged_batch_context_stays_inside_each_utterance(timit):
    from world._synthetic import synth_utterance
    from world.batch import WorldBatch
    from world.manifold import vae_device

    fs = 16000
    xs = [synth_utterance(300 + u, fs, 0.12 + 0.05 * (u % 7)) for u in range(31)]
    wb = WorldBatch(0)
    enc = wb.encode(xs, fs, f0_method="dio")
    rng = np.random.RandomState(4)
    e = random_stack(rng, (39 * 5, 256, 256, 12), ("relu", "relu", "linear"))
    d = random_stack(rng, (12, 256, 256, 39 * 5), ("relu", "relu", "linear"))
    mean = rng.randn(39) * 0.1
    z_d, y_d = enc.vae(e, d, mean, n0=40, window=2)
    z, y = z_d.cpu().numpy(), y_d.cpu().numpy()
    mc = enc.mcep(40)
    fo = enc.batch.frame_off
    assert y.shape == (int(fo[-1]), 39) and z.shape == (int(fo[-1]), 12)
    for u in range(len(xs)):
        a, b = int(fo[u]), int(fo[u + 1])
        zu, yu = vae_device(wb.rt, mc[a:b, 1:].contiguous(), e, d, window=2, mean=mean)
        assert np.array_equal(zu.cpu().numpy(), z[a:b]) and np.array_equal(yu.cpu().numpy(), y[a:b]), u
    # the manifold-vocoded spectrogram, synthesised without leaving the device
    enc_t, dec_t = timit
    venc = enc.with_vae_spectrogram(enc_t, dec_t, np.zeros(39), n0=40)
    assert venc.spectrogram.shape == enc.spectrogram.shape and venc.f0 is enc.f0
    yv, yoff = wb.decode_device(venc)
    y0, yoff0 = wb.decode_device(enc)
    assert np.array_equal(np.asarray(yoff), np.asarray(yoff0))
    assert np.all(np.isfinite(yv.cpu().numpy()))
    assert wb.rt.take_flags() == [0] * 16


def test_unusable_arguments_raise(rt, timit):
    from world import _hip, main
    from world.manifold import DenseStack, dense_stack_device

    x_d = rt.to_device(np.zeros((4, 3)))
    vp = ctypes.c_void_p

    def call(units, acts, w, b):
        units = np.array(units, np.int32)
        acts = np.array(acts, np.int32)
        w = np.ascontiguousarray(w, np.float64)
        b = np.ascontiguousarray(b, np.float64)
        seg = np.array([0, 4], np.int64)
        out = rt.empty((4, int(units[-1])))
        return rt.lib.wh_dense_stack(rt.ctx, rt.stream(), rt.ptr(x_d), 4, 3, 3,
                                     seg.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 1, 0, vp(None), len(units),
                                     units.ctypes.data_as(vp), acts.ctypes.data_as(vp), w.ctypes.data_as(vp),
                                     b.ctypes.data_as(vp), 0, int(units[-1]), -1, vp(None), 0, 0, vp(None),
                                     rt.ptr(out), int(units[-1]), 0)

    assert call([300, 2], [1, 0], np.zeros(3 * 300 + 300 * 2), np.zeros(302)) != 0
    assert b"256" in _hip.load_library().wh_last_error()
    assert call([4], [7], np.zeros(12), np.zeros(4)) != 0
    assert b"activation" in _hip.load_library().wh_last_error()
    w = np.zeros(12)
    w[5] = np.nan
    assert call([4], [1], w, np.zeros(4)) != 0
    assert b"non-finite" in _hip.load_library().wh_last_error()
    assert call([4], [1], np.ones(12), np.ones(4)) == 0
    rng = np.random.RandomState(0)
    with pytest.raises(ValueError, match="limit is 256"):
        dense_stack_device(rt, x_d, DenseStack([(rng.randn(3, 257), np.zeros(257), "relu"),
                                                (rng.randn(257, 2), np.zeros(2), "linear")]))
    with pytest.raises(ValueError, match="swish"):
        DenseStack([(rng.randn(3, 4), np.zeros(4), "swish")])
    with pytest.raises(ValueError, match="non-finite"):
        DenseStack([(np.full((3, 4), np.nan), np.zeros(4), "relu")])
    with pytest.raises(AssertionError):
        main.World().encode_vae(np.zeros((5, 39)), np.zeros(5), ENC, DEC, 0, 12, 256, 0.0)
    # the context is still usable afterwards
    enc, dec = timit
    z, y = main.World().encode_vae(np.zeros((3, 39)), np.zeros(3), enc, dec, 0, 40, 256, 0.0)
    assert np.all(np.isfinite(y))
