"""GPU: world.melcep.melcep_device / spectrum_device — one host table each through the product kernel (prologue log,
epilogue exp) — against the long-double product with the bound tests/_feature_reference.py derives, at every K and order
the tables are built for and at row counts around the kernel's 128-row tile; then code and decode on the committed
spectrogram fixtures, where the facade's NumPy forms must agree with the device forms bit for bit."""
import os

import numpy as np
import pytest

import _feature_reference as fref
import _melcep_reference as mref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K_BINS = (257, 513, 1025, 2049)
ORDERS = (1, 24, 59, 64)
ROWS = (1, 127, 128, 129)
ALPHAS = (0.42, 0.554, -0.3, 0.0)
# every (K, m) once, the row counts and alphas going round; the centre (513, 24) at every row count
SHAPES = tuple((k, m, ROWS[(i + j) % 4], ALPHAS[(i + 2 * j) % 4]) for i, k in enumerate(K_BINS) for j, m in enumerate(ORDERS))
SHAPES += tuple((513, 24, r, 0.42) for r in ROWS if (513, 24, r, 0.42) not in SHAPES)


@pytest.fixture(scope="module")
def rt():
    from world import _hip
    return _hip.Runtime.get()


@pytest.mark.parametrize("k_bins, order, rows, alpha", SHAPES)
def test_coding_and_decoding_are_the_long_double_products(rt, k_bins, order, rows, alpha):
    from world import melcep

    rng = np.random.RandomState(k_bins + 7 * order + rows)
    spec = np.exp(rng.uniform(-12, 3, size=(rows, k_bins)))
    got = melcep.melcep_device(rt, rt.to_device(spec), order, alpha).cpu().numpy()
    assert got.shape == (rows, order + 1)
    fref.check("melcep_device", got, spec, k_bins, k_bins, None, 1.0, melcep.encode_table(k_bins, order, alpha).w, 2, 0)
    c = mref.random_rows(rng, rows, order)
    got = melcep.spectrum_device(rt, rt.to_device(c), 2 * (k_bins - 1), alpha).cpu().numpy()
    assert got.shape == (rows, k_bins)
    fref.check("spectrum_device", got, c, order + 1, order + 1, None, 1.0, melcep.decode_table(order, alpha, k_bins).w, 0, 2)
    assert rt.take_flags() == [0] * 16


def test_rows_inside_a_wider_tensor(rt):
    """The leading dimension is the tensor's: columns 3 .. 3 + K of a wider spectrogram, columns 1 .. 26 of wider rows."""
    from world import melcep

    rng = np.random.RandomState(2)
    wide = np.exp(rng.uniform(-3, 3, size=(40, 520)))
    a = melcep.melcep_device(rt, rt.to_device(wide)[:, 3:516], 24, 0.42).cpu().numpy()
    b = melcep.melcep_device(rt, rt.to_device(np.ascontiguousarray(wide[:, 3:516])), 24, 0.42).cpu().numpy()
    assert a.tobytes() == b.tobytes()
    rows = mref.random_rows(rng, 40, 26)
    a = melcep.spectrum_device(rt, rt.to_device(rows)[:, 1:26], 1024, 0.42).cpu().numpy()
    b = melcep.spectrum_device(rt, rt.to_device(np.ascontiguousarray(rows[:, 1:26])), 1024, 0.42).cpu().numpy()
    assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name, fs, order", [("golden_syn16k", 16000, 24), ("golden_syn16k", 16000, 40), ("golden_syn48k", 48000, 59)])
def test_code_and_decode_a_cheaptrick_spectrogram(rt, name, fs, order):
    """The fixture's CheapTrick spectrogram coded at the customary alpha and order and decoded again.  The log-spectral
    distance to the input is a figure (printed; DESIGN section 23 records it), not a gate: it is the smoothing that a
    cepstrum of that order does.  The rows are the reference's, and the facade's NumPy forms are the device forms."""
    from world import melcep
    from world.main import World

    spec = np.ascontiguousarray(np.load(os.path.join(GOLDEN, name + ".npz"))["ct_spectrogram"].T)
    f, k_bins = spec.shape
    alpha = melcep.default_alpha(fs)
    mc_d = melcep.melcep_device(rt, rt.to_device(spec), order, alpha)
    back_d = melcep.spectrum_device(rt, mc_d, 2 * (k_bins - 1), alpha)
    mc, back = mc_d.cpu().numpy(), back_d.cpu().numpy()
    lsd = np.sqrt(np.mean((10 * np.log10(back / spec)) ** 2, axis=1))
    print("melcep %s order %d alpha %g: %d frames of %d bins, log-spectral distance mean %.3f dB, worst frame %.3f dB"
          % (name, order, alpha, f, k_bins, float(np.mean(lsd)), float(np.max(lsd))))
    assert np.all(np.isfinite(mc)) and np.all(back > 0)
    want = mref.sp2mc(spec, order, alpha)
    assert np.max(np.abs(mc - want)) <= 1e-9 * np.max(np.abs(want))  # (the suite's chain bound; the product itself is held above)
    w = World()
    assert w.encode_melcep(spec, order, fs=fs).tobytes() == mc.tobytes()
    assert w.decode_melcep(mc, 2 * (k_bins - 1), fs=fs).tobytes() == back.tobytes()
    shifted = mc + 0.01
    got = w.melcep_distortion(mc, shifted)
    assert got.tobytes() == melcep.mcd_db_device(mc_d, rt.to_device(shifted)).cpu().numpy().tobytes()
    assert np.allclose(got, mref.mcd_db(mc, shifted), rtol=64 * np.finfo(np.float64).eps, atol=0)
    assert rt.take_flags() == [0] * 16
