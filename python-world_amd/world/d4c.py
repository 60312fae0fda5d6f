"""D4C aperiodicity ("Love Train") — drop-in for world/d4c.py:10 of the reference, executed by the
HIP kernels behind wh_d4c (include/world_hip.h)."""
import numpy as np

from . import _hip


def d4c_device(rt, batch, x_d, tp_d, f0_d, vuv_d, fs, threshold, fft_size_for_spectrum, want_coarse=False):
    """Device-resident core: returns (aperiodicity [F][K], coarse_ap [F][nap] or None); f0_d zeroed where vuv==0."""
    nf = batch.total_frames
    interval = 2000 if fs < 16000 else 3000
    nap = int(np.floor(np.min([15000, fs / 2 - interval]) / interval))
    assert nap > 0  # world/d4c.py:35
    k = fft_size_for_spectrum // 2 + 1
    ap = rt.empty((nf, k))
    coarse = rt.empty((nf, nap)) if want_coarse else None
    _hip.check(rt.lib.wh_d4c(rt.ctx, rt.stream(), batch.handle, rt.ptr(x_d), rt.ptr(tp_d), rt.ptr(f0_d),
                             rt.ptr(vuv_d), float(fs), float(threshold), int(fft_size_for_spectrum), rt.ptr(ap),
                             rt.ptr(coarse)))
    return ap, coarse


def aperiodicity_from_bands_device(rt, coarse_d, gate_d, fs, fft_size_for_spectrum):
    """The last step of d4c() alone (world/d4c.py:45-59, wh_aperiodicity_from_bands): dense aperiodicity [F][K] from the
    band values [F][nap] as 'coarse_ap' holds them and the voicing gate [F] (0: the frame's row is 1 - 1e-12) — the rows
    d4c_device writes for the same frames, bit for bit."""
    nf, nap = (int(v) for v in coarse_d.shape)
    interval = 2000 if fs < 16000 else 3000
    want = int(np.floor(np.min([15000, fs / 2 - interval]) / interval))
    if nap != want or tuple(gate_d.shape) != (nf,):
        raise ValueError("aperiodicity_from_bands: at fs = %r d4c() has %d band(s) and one gate value per frame, got "
                         "coarse %s and gate %s" % (fs, want, tuple(coarse_d.shape), tuple(gate_d.shape)))
    k = int(fft_size_for_spectrum) // 2 + 1
    ap = rt.empty((nf, k))
    _hip.check(rt.lib.wh_aperiodicity_from_bands(rt.ctx, rt.stream(), nf, nap, k, float(fs), interval,
                                                 rt.ptr(coarse_d.contiguous()), rt.ptr(gate_d.contiguous()), rt.ptr(ap)))
    return ap


def aperiodicity_gate_device(rt, ap_d):
    """[F] float64: 0 where row f of d4c_device's aperiodicity is the constant row of a frame the voicing gate rejected
    (world/d4c.py:49-51), 1 where it came from the bands — read from bin 0 (wh_aperiodicity_gate)."""
    nf, k = (int(v) for v in ap_d.shape)
    gate = rt.empty((nf,))
    _hip.check(rt.lib.wh_aperiodicity_gate(rt.ctx, rt.stream(), nf, k, rt.ptr(ap_d), rt.ptr(gate)))
    return gate


@_hip.serialised
def aperiodicity_from_coarse(coarse_ap, ap_gate, fs, fft_size):
    """Dense 'aperiodicity' (fft_size // 2 + 1, frames) of one utterance from d4c()'s 'coarse_ap' (nap, frames) and the
    gate (frames,) — NumPy in, NumPy out, evaluated on the device like features.decode_mcep."""
    coarse_ap = np.asarray(coarse_ap, dtype=np.float64)
    ap_gate = np.asarray(ap_gate, dtype=np.float64)
    if coarse_ap.ndim != 2 or ap_gate.shape != (coarse_ap.shape[1],):
        raise ValueError("aperiodicity_from_coarse: coarse_ap must be (bands, frames) and ap_gate (frames,), got %s and %s"
                         % (coarse_ap.shape, ap_gate.shape))
    rt = _hip.Runtime.get()
    ap = aperiodicity_from_bands_device(rt, rt.to_device(coarse_ap.T), rt.to_device(ap_gate), fs, fft_size)
    return rt.to_host(ap, transpose=True)


@_hip.serialised
def d4c(x, fs, f0_object, threshold=0.85, fft_size_for_spectrum=None):
    """Same contract as the reference: zeroes f0_object['f0'] where vuv==0, adds 'aperiodicity' (K,F)
    and 'coarse_ap' (nap,F) to the SAME dict and returns it (world/d4c.py:28-32,61-64)."""
    if fft_size_for_spectrum is None:
        fft_size_for_spectrum = int(2 ** np.ceil(np.log2(3 * fs / 71 + 1)))
    rt = _hip.Runtime.get()
    x = np.asarray(x, dtype=np.float64)
    f0 = f0_object['f0']
    _hip.same_frames("d4c", temporal_positions=f0_object['temporal_positions'], f0=f0, vuv=f0_object['vuv'])
    batch = rt.make_batch([0, len(x)], [0, len(f0)])
    f0_d = rt.to_device(f0)
    ap, coarse = d4c_device(rt, batch, rt.to_device(x), rt.to_device(f0_object['temporal_positions']), f0_d,
                            rt.to_device(f0_object['vuv']), fs, threshold, int(fft_size_for_spectrum), want_coarse=True)
    f0[...] = f0_d.cpu().numpy()
    f0_object['aperiodicity'] = rt.to_host(ap, transpose=True)
    f0_object['coarse_ap'] = rt.to_host(coarse, transpose=True)
    return f0_object
