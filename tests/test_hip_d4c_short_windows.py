"""GPU: D4C's register-fed windows (csrc/wh_d4c_window.h) at every number of rows a window can span.  At 16 kHz a frame's
transform has 2048 points on 256 threads, eight rows per thread; a window of at most four rows takes the short gather
(every pitch above 62.5 Hz), a longer one the gather of all rows.  wh_d4c on batches of one to four frames at pitches on
both sides of that boundary — frames at either end of the utterance, whose sample indices are clamped, and utterances
shorter than one window — against the oracle at the tolerances of tests/test_hip_d4c.py, into buffers whose NaN guard rows
must survive."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FS = 16000


def _voiced(n, f0, seed):
    """Harmonics of f0 falling off as 1 / h^2 (nearly all energy below 4 kHz: the gate passes) over a noise floor."""
    t = np.arange(n) / FS
    rng = np.random.RandomState(seed)
    x = np.zeros(n)
    for h in range(1, int(7000 / f0) + 1):
        x += np.sin(2 * np.pi * h * f0 * t + rng.uniform(0, 2 * np.pi)) / h ** 2
    return 0.3 * x + 1e-3 * rng.randn(n)


def _d4c_guarded(x, f0, tp):
    """wh_d4c into the middle rows of NaN-filled tensors -> (aperiodicity (K, F), coarse (nap, F), guards intact)."""
    from world import _hip

    rt = _hip.Runtime.get()
    nf, nfft_spec, nap = len(tp), 1024, 1  # (16 kHz: 3 fs / 71 + 1 -> 1024 bins of output; one band of 3 kHz below fs / 2 - 3 kHz)
    k = nfft_spec // 2 + 1
    ap = rt.torch.full((nf + 2, k), float("nan"), dtype=rt.torch.float64, device=rt.device)
    coarse = rt.torch.full((nf + 2, nap), float("nan"), dtype=rt.torch.float64, device=rt.device)
    batch = rt.make_batch([0, len(x)], [0, nf])
    x_d, tp_d, f0_d, vuv_d = rt.to_device(x), rt.to_device(tp), rt.to_device(f0), rt.to_device(np.ones(nf))
    _hip.check(rt.lib.wh_d4c(rt.ctx, rt.stream(), batch.handle, rt.ptr(x_d), rt.ptr(tp_d), rt.ptr(f0_d), rt.ptr(vuv_d), float(FS),
                             0.85, nfft_spec, rt.ptr(ap[1:nf + 1]), rt.ptr(coarse[1:nf + 1])))
    ap, coarse = ap.cpu().numpy(), coarse.cpu().numpy()
    assert rt.take_flags() == [0] * 16
    guards = np.isnan(ap[[0, -1]]).all() and np.isnan(coarse[[0, -1]]).all()
    return ap[1:-1].T, coarse[1:-1].T, bool(guards)


@pytest.mark.parametrize("f0", [47.0, 62.0, 63.0, 125.0, 400.0])
def test_windows_of_every_row_count_at_the_utterance_edges(f0):
    from oracle import aperiodicity as oap

    assert int(2 ** np.ceil(np.log2(3 * FS / 71 + 1))) == 1024
    n_long = 6400
    end = (n_long - 1) / FS
    cases = [(n_long, [0.0]), (n_long, [end]), (n_long, [0.2]), (n_long, [0.0, 0.2]), (n_long, [0.0, 0.005, 0.2]),
             (n_long, [0.0, 0.01, 0.395, end]),
             (60, [0.0]), (100, [0.0, 0.005]), (320, [0.0, 0.005, 0.01, 0.015])]  # shorter than a window of 4 / f0 (and of 3 / f0)
    passed = 0
    for i, (n, tp) in enumerate(cases):
        x = _voiced(n, f0, 100 + i)
        tp = np.array(tp)
        f0s = np.full(len(tp), f0)
        want_ap, want_coarse, _ = oap.d4c_np(x, FS, f0s.copy(), np.ones(len(tp)), tp)
        ap, coarse, guards = _d4c_guarded(x, f0s, tp)
        print(f0, n, list(tp), "coarse", coarse.ravel(), "want", want_coarse.ravel(),
              "max |d ap|", np.max(np.abs(ap - want_ap)))
        assert guards, (n, list(tp))
        assert np.array_equal(coarse != 0, want_coarse != 0), (n, list(tp))  # the same frames pass the gate
        assert np.max(np.abs(coarse - want_coarse)) < 1e-6, (n, list(tp))  # dB
        assert np.max(np.abs(ap - want_ap)) < 1e-7, (n, list(tp))
        passed += int((want_coarse != 0).sum())
    assert passed > 0  # (the band stage ran, not only the gate)
