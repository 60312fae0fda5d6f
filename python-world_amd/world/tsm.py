"""Time-scale and pitch modification of recordings without analysis and synthesis: waveform-similarity overlap-add
(wh_wsola, csrc/wh_wsola.hip; the contract is in include/world_hip.h, DESIGN section 20, and in NumPy in
tests/_wsola_reference.py) and, with world.resample, Kobayashi and Toda's f0 transformation for vocoder-free conversion.

Frames of 2 H - 1 samples are copied from the recording to an integer output hop H; every frame's start may move by up to
D samples from its nominal position to where the recording continues the frame before best.  Stretching by p / q and
resampling by q / p keeps the duration and multiplies f0 — and the formants — by p / q; the differential filter
(world.specfilter, world.gmm.convert_waveform) is then trained and applied on the shifted recording and moves the envelope
to the target.

    y_d, y_off = stretch_device(rt, x_d, x_off, fs, 1.25)                  # 1.25 x as long, the same pitch
    y_d, frac = shift_pitch_device(rt, x_d, x_off, fs, ratio)              # x's layout, f0 x frac = as_fraction(ratio)
    ratio = log_f0_ratio(ce_source, ce_target)                             # the ratio of the geometric mean f0s

window, n_frames, positions, positions_from_map, default_hop_tol, as_fraction, stretched_length and check_wsola_args are
host code and need neither the library nor a GPU."""
from fractions import Fraction

import numpy as np

from . import _hip

MAX_HOP, MAX_TOL = 1024, 512
MAX_DENOMINATOR = 64


# ---- host ------------------------------------------------------------------------------------------------------------
def window(hop):
    """float64 [2 H - 1]: 0.5 - 0.5 cos(pi (j + 1) / H), the spectral filter's window; win[j] + win[j + H] = 1."""
    j = np.arange(2 * int(hop) - 1, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(np.pi * (j + 1.0) / float(hop))


def n_frames(n_out, hop):
    """ceil(n_out / H) + 1 frames cover n_out samples (frame m starts at output sample m H - H); none for an empty output."""
    return 0 if n_out <= 0 else -(-int(n_out) // int(hop)) + 1


def positions(n_out, hop, ratio):
    """int64 [n_frames]: the nominal input start of every frame for a uniform stretch by ``ratio`` (output over input
    duration): floor((m H - 1) / ratio + 0.5) - (H - 1) in float64 — the frame whose output centre is m H - 1 is taken
    around the input sample (m H - 1) / ratio.  At ratio 1 frame m starts at m H - H and the output is the input."""
    if not np.isfinite(float(ratio)) or float(ratio) <= 0:
        raise ValueError("positions: the ratio must be positive and finite, got %r" % (ratio,))
    m = np.arange(n_frames(n_out, hop), dtype=np.float64)
    return (np.floor((m * float(hop) - 1.0) / float(ratio) + 0.5) - (float(hop) - 1.0)).astype(np.int64)


def positions_from_map(n_out, hop, out_times, in_times):
    """int64 [n_frames] for a non-uniform stretch: the piecewise-linear map through the points (out_times[i], in_times[i])
    (in samples; out_times strictly ascending, at least two points; the end segments are extended beyond the ends) takes
    every frame's output centre m H - 1 to its input centre c: floor(c + 0.5) - (H - 1)."""
    to, ti = np.asarray(out_times, dtype=np.float64), np.asarray(in_times, dtype=np.float64)
    if to.ndim != 1 or to.shape != ti.shape or len(to) < 2 or not np.all(np.isfinite(to)) or not np.all(np.isfinite(ti)):
        raise ValueError("positions_from_map: two finite 1-D lists of the same length >= 2, got shapes %s and %s" % (to.shape, ti.shape))
    if np.any(np.diff(to) <= 0):
        raise ValueError("positions_from_map: out_times must ascend strictly")
    centre = np.arange(n_frames(n_out, hop), dtype=np.float64) * float(hop) - 1.0
    seg = np.clip(np.searchsorted(to, centre, side="right") - 1, 0, len(to) - 2)
    c = ti[seg] + (centre - to[seg]) * ((ti[seg + 1] - ti[seg]) / (to[seg + 1] - to[seg]))
    return (np.floor(c + 0.5) - (float(hop) - 1.0)).astype(np.int64)


def default_hop_tol(fs):
    """(H, D): 8 ms and 5 ms in whole samples — (128, 80) at 16 kHz, (176, 110) at 22.05 kHz, (384, 240) at 48 kHz."""
    hop = max(1, int(np.floor(float(fs) * 0.008 + 1e-9)))
    tol = int(np.floor(float(fs) * 0.005 + 1e-9))
    if hop > MAX_HOP or tol > MAX_TOL:
        raise ValueError("default_hop_tol: 8 ms and 5 ms at fs = %r are %d and %d samples, beyond the library's %d and %d: "
                         "pass hop and tol" % (fs, hop, tol, MAX_HOP, MAX_TOL))
    return hop, tol


def as_fraction(ratio):
    """Fraction(ratio).limit_denominator(64): the p / q that shift_pitch_device stretches and resamples by."""
    if isinstance(ratio, bool) or not isinstance(ratio, (int, float, Fraction, np.integer, np.floating)):
        raise ValueError("as_fraction: the ratio must be a number, got %r" % (ratio,))
    r = ratio if isinstance(ratio, Fraction) else Fraction(float(ratio)) if not isinstance(ratio, (int, np.integer)) else Fraction(int(ratio))
    if r <= 0:
        raise ValueError("as_fraction: the ratio must be positive, got %r" % (ratio,))
    f = r.limit_denominator(MAX_DENOMINATOR)
    if f <= 0:
        raise ValueError("as_fraction: %r is below 1 / %d" % (ratio, 2 * MAX_DENOMINATOR))
    return f


def stretched_length(n, ratio):
    """round(ratio n), halves upwards: exact for a Fraction, floor(ratio n + 0.5) in float64 otherwise."""
    if isinstance(ratio, Fraction):
        return int((2 * int(n) * ratio.numerator + ratio.denominator) // (2 * ratio.denominator))
    if not np.isfinite(float(ratio)) or float(ratio) <= 0:
        raise ValueError("stretched_length: the ratio must be positive and finite, got %r" % (ratio,))
    return int(np.floor(float(ratio) * float(n) + 0.5))


def check_wsola_args(x_off, y_lengths, positions, hop, tol, where="wsola"):
    """ValueError for what wh_wsola refuses.  ``positions``: one integer list per utterance.  Returns
    (x_off, y_off, pos_off, pos) as contiguous int64 arrays."""
    for name, v, lo, hi in (("hop", hop, 1, MAX_HOP), ("tol", tol, 0, MAX_TOL)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
            raise ValueError("%s: %s must be an integer in [%d, %d], got %r" % (where, name, lo, hi, v))
    x_off = _hip.check_sample_offsets(x_off, where)
    n = len(x_off) - 1
    if len(y_lengths) != n or len(positions) != n:
        raise ValueError("%s: %d utterances, %d output lengths and %d position lists" % (where, n, len(y_lengths), len(positions)))
    lens = _hip.check_output_lengths(y_lengths, where)
    plist = []
    for u in range(n):
        p = np.asarray(positions[u])
        if p.ndim != 1 or len(p) != n_frames(lens[u], hop):
            raise ValueError("%s: utterance %d of %d output samples at hop %d has %d frames, its position list %s entries"
                             % (where, u, lens[u], hop, n_frames(lens[u], hop), np.shape(p)))
        if len(p) and not np.issubdtype(p.dtype, np.integer):
            raise ValueError("%s: utterance %d: positions must be integers, got %s" % (where, u, p.dtype))
        plist.append(p.astype(np.int64))
    y_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    pos_off = np.concatenate([[0], np.cumsum([len(p) for p in plist])]).astype(np.int64)
    pos = np.ascontiguousarray(np.concatenate(plist) if plist else np.zeros(0), dtype=np.int64)
    return x_off, y_off, pos_off, pos


# ---- device ----------------------------------------------------------------------------------------------------------
def wsola_device(rt, x_d, x_off, y_lengths, positions, hop, tol):
    """wh_wsola on the resident recordings ``x_d`` (flat, utterance u at x_off[u]:x_off[u+1]): utterance u becomes
    y_lengths[u] samples whose frames are taken around positions[u] (n_frames(y_lengths[u], hop) nominal input starts; any
    integer is legal, the recording is 0 outside itself).  Returns (y_d, y_off, delta_d): the outputs one after the other,
    their host offsets, and the int32 shift of every frame in the order of the concatenated position lists."""
    where = "wsola_device"
    x_off, y_off, pos_off, pos = check_wsola_args(x_off, y_lengths, positions, hop, tol, where)
    _hip.check_recording(rt, x_d, x_off, where)
    n = len(x_off) - 1
    win = np.ascontiguousarray(window(hop), dtype=np.float64)
    with rt.lock, rt.on_stream():
        y_d = rt.empty((int(y_off[-1]),))
        delta_d = rt.torch.zeros((int(pos_off[-1]),), dtype=rt.torch.int32, device=rt.device)
        if n:
            _hip.check(rt.lib.wh_wsola(rt.ctx, rt.stream(), n, _hip.i64p(x_off), _hip.i64p(y_off), _hip.i64p(pos_off),
                                       _hip.i64p(pos), int(hop), int(tol), _hip.f64p(win), rt.ptr(x_d), rt.ptr(y_d),
                                       rt.ptr(delta_d)))
    return y_d, y_off, delta_d


def _per_utterance(ratio, n, where):
    r = [ratio] * n if np.ndim(ratio) == 0 or isinstance(ratio, Fraction) else list(ratio)
    if len(r) != n:
        raise ValueError("%s: %d ratios for %d utterances" % (where, len(r), n))
    return r


def _hop_tol(fs, hop, tol):
    if hop is None or tol is None:
        dh, dt = default_hop_tol(fs)
        hop, tol = dh if hop is None else hop, dt if tol is None else tol
    return hop, tol


def stretch_device(rt, x_d, x_off, fs, ratio, hop=None, tol=None):
    """The recordings time-stretched: utterance u becomes round(ratio n_u) samples, its duration x ratio, at its own pitch.
    ``ratio``: a number (or Fraction), or one per utterance.  ``hop`` / ``tol``: default_hop_tol(fs) when None.  Returns
    (y_d, y_off)."""
    where = "stretch_device"
    x_off = np.ascontiguousarray(x_off, dtype=np.int64)
    n = len(x_off) - 1
    hop, tol = _hop_tol(fs, hop, tol)
    check_wsola_args([0], [], [], hop, tol, where)  # (hop and tol, before anything is divided by the hop)
    ratios = _per_utterance(ratio, max(n, 0), where)
    lens = [stretched_length(int(x_off[u + 1] - x_off[u]), ratios[u]) for u in range(n)]
    pos = [positions(lens[u], hop, ratios[u]) for u in range(n)]
    y_d, y_off, _ = wsola_device(rt, x_d, x_off, lens, pos, hop, tol)
    return y_d, y_off


def shift_pitch_device(rt, x_d, x_off, fs, ratio, hop=None, tol=None, window=('kaiser', 5.0)):
    """The recordings with f0 x p / q at their own durations, p / q = as_fraction(ratio): stretched by p / q, resampled by
    q / p (world.resample.resample_device: scipy.signal.resample_poly(.., q, p) bit for bit), then trimmed or zero-padded to
    the input's length.  Returns (y_d in x's layout — utterance u at x_off[u]:x_off[u+1] —, the Fraction used).  The
    resampling moves the whole spectrum: the formants move by p / q with f0; the differential filter trained on the
    shifted recording moves the envelope to the target.  The alternative that leaves the formants in place — and takes a
    contour as well as a ratio — is world.psola.modify_device(.., pitch=log_f0_ratio(a, b))."""
    from .resample import resample_device

    where = "shift_pitch_device"
    x_off = _hip.check_sample_offsets(x_off, where)
    n = len(x_off) - 1
    fracs = [as_fraction(r) for r in _per_utterance(ratio, n, where)]
    with rt.lock, rt.on_stream():
        s_d, s_off = stretch_device(rt, x_d, x_off, fs, fracs if n else 1, hop, tol)
        r_d, r_off = resample_device(rt, s_d, s_off, [f.denominator for f in fracs], [f.numerator for f in fracs], window)
        y_d = rt.torch.zeros((int(x_d.shape[0]),), dtype=rt.torch.float64, device=rt.device)
        for u in range(n):
            keep = int(min(x_off[u + 1] - x_off[u], r_off[u + 1] - r_off[u]))
            if keep:
                y_d[int(x_off[u]):int(x_off[u]) + keep] = r_d[int(r_off[u]):int(r_off[u]) + keep]
    return y_d, (fracs[0] if np.ndim(ratio) == 0 or isinstance(ratio, Fraction) else fracs)


def log_f0_ratio(ce_source, ce_target):
    """exp(mean log f0 of the target's voiced frames - mean log f0 of the source's): the ratio of the two corpora's
    geometric mean f0, the ratio to hand to shift_pitch_device.  ``ce_source`` / ``ce_target``: CompactEncodings or
    BatchEncodings (device or host); a frame counts when its vuv is set and its f0 positive.  One reduction per corpus on
    the device the encoding lives on; ValueError when a corpus has no voiced frame."""
    means = []
    for name, e in (("source", ce_source), ("target", ce_target)):
        f0, vuv = getattr(e, "f0", None), getattr(e, "vuv", None)
        if f0 is None or vuv is None:
            raise ValueError("log_f0_ratio: the %s must be a CompactEncoding or a BatchEncoding, got %r" % (name, type(e).__name__))
        if isinstance(f0, np.ndarray):
            f0h, voiced = np.asarray(f0, dtype=np.float64), (np.asarray(vuv) != 0) & (np.asarray(f0) > 0)
            count, total = int(np.count_nonzero(voiced)), float(np.sum(np.log(f0h[voiced])))
        else:
            voiced = (vuv != 0) & (f0 > 0)
            count = int(voiced.sum().item())
            total = float(f0[voiced].log().sum().item()) if count else 0.0
        if count == 0:
            raise ValueError("log_f0_ratio: the %s has no voiced frame" % name)
        means.append(total / count)
    return float(np.exp(means[1] - means[0]))


# ---- NumPy forms (World.stretch_waveform / World.shift_pitch_waveform) -------------------------------------------------
def stretch_waveform_numpy(fs, x, ratio, hop=None, tol=None):
    return _hip.recording_through("stretch_waveform", x, lambda rt, x_d, x_off: stretch_device(rt, x_d, x_off, fs, ratio, hop, tol)[0])


def shift_pitch_waveform_numpy(fs, x, ratio, hop=None, tol=None):
    return _hip.recording_through("shift_pitch_waveform", x,
                                  lambda rt, x_d, x_off: shift_pitch_device(rt, x_d, x_off, fs, ratio, hop, tol)[0])
