"""Pitch contours from outside and frame-grid conversion: what the reference's World.set_pitch leaves open
(world/main.py:164-168 raises NotImplementedError: "need to resample to set values at given temporal positions (which
are presumably shared with the spectrogram)").  Both resamplings are np.interp, reproduced bit for bit by the kernels
behind wh_interp_contour and wh_regrid_rows (csrc/wh_regrid.hip).

The knot-list checks and the destination grid are host code and need neither the library nor a GPU."""
import ctypes

import numpy as np

from . import _hip, _tables


# ---- host: knot lists ----------------------------------------------------------------------------------------------
def knot_lists(times, values, n_utt, where="set_pitch_contour"):
    """Per-utterance knot lists from what a caller passes: one pair of 1-D arrays for every utterance, or a list with one
    array per utterance on each side (``values=None``: ``times`` is a list of (time, value) pairs).  Returns
    (knot_off int64 [n_utt+1], time float64, value float64) — the ragged layout wh_interp_contour takes.  Raises
    ValueError for a wrong number of lists, lengths that disagree, an empty list, and times that are not finite and
    strictly increasing; touches no device."""
    if values is None:
        pairs = list(times)
        if any(len(p) != 2 for p in pairs):
            raise ValueError("%s: without `values`, `times` must be a list of (time, value) pairs" % where)
        times, values = [p[0] for p in pairs], [p[1] for p in pairs]
    if isinstance(times, np.ndarray):
        shared = times.ndim == 1 and times.dtype != object
    else:
        shared = len(times) > 0 and np.ndim(times[0]) == 0
    if shared:  # one pair of arrays for every utterance
        times, values = [times] * n_utt, [values] * n_utt
    times, values = list(times), list(values)
    if len(times) != n_utt or len(values) != n_utt:
        raise ValueError("%s: %d time list(s) and %d value list(s) for a batch of %d utterance(s)"
                         % (where, len(times), len(values), n_utt))
    ts, vs = [], []
    for u, (t, v) in enumerate(zip(times, values)):
        t = np.asarray(t, dtype=np.float64)
        v = np.asarray(v, dtype=np.float64)
        if t.ndim != 1 or v.ndim != 1 or len(t) != len(v):
            raise ValueError("%s: utterance %d: time and value must be 1-D and of one length, got %s and %s"
                             % (where, u, t.shape, v.shape))
        if len(t) == 0:
            raise ValueError("%s: utterance %d: no knots" % (where, u))
        if not np.all(np.isfinite(t)):
            raise ValueError("%s: utterance %d: knot times must be finite" % (where, u))
        if np.any(np.diff(t) <= 0):
            raise ValueError("%s: utterance %d: knot times must be strictly increasing" % (where, u))
        ts.append(t)
        vs.append(v)
    off = np.concatenate([[0], np.cumsum([len(t) for t in ts])]).astype(np.int64)
    cat = lambda parts: np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(0), dtype=np.float64)  # noqa: E731
    return off, cat(ts), cat(vs)


def interp_contour_host(tp, time, value, voiced_rule=True):
    """The rule of wh_interp_contour for one utterance in NumPy: (f0, vuv), or np.interp alone without the rule.  A frame
    is voiced iff every knot np.interp reads for it has value > 0: both bracketing knots, or the single knot on an exact
    hit, at the last knot and outside the range."""
    tp, time, value = (np.asarray(a, dtype=np.float64) for a in (tp, time, value))
    r = np.interp(tp, time, value)
    if not voiced_rule:
        return r
    n = len(time)
    j = np.clip(np.searchsorted(time, tp, side="right") - 1, 0, n - 1)
    single = (tp < time[0]) | (j >= n - 1) | (time[j] == tp)
    pos = value > 0
    voiced = np.where(single, pos[j], pos[j] & pos[np.minimum(j + 1, n - 1)])
    return np.where(voiced, r, 0.0), voiced.astype(np.float64)


# ---- host: the destination grid ------------------------------------------------------------------------------------
def destination_times(tp_u, frame_period):
    """Frame times of one utterance on the grid of ``frame_period`` ms: the project's own expression
    _tables.frame_times(n', frame_period), shifted by the utterance's first frame time when that is not 0, with n' the
    number of grid points not beyond its last source frame time — NumPy float semantics throughout, as decode_device
    derives its geometry.  An untouched 5 ms utterance regridded to 5 ms gets its own frame times back, bit for bit."""
    tp_u = np.asarray(tp_u, dtype=np.float64)
    if len(tp_u) == 0:
        return np.zeros(0)
    if not frame_period > 0:
        raise ValueError("regrid: frame_period must be positive, got %r" % (frame_period,))
    t0, last = float(tp_u[0]), float(tp_u[-1])
    guess = int(np.floor((last - t0) / (frame_period / 1000))) + 3
    g = _tables.frame_times(max(guess, 1), frame_period)
    if t0 != 0:
        g = g + t0
    return g[:max(1, int(np.searchsorted(g, last, side="right")))]


def check_source_times(tp_h, frame_off, where="regrid"):
    """The source frame times must increase strictly inside every utterance (np.interp's precondition)."""
    for u in range(len(frame_off) - 1):
        t = tp_h[int(frame_off[u]):int(frame_off[u + 1])]
        if not np.all(np.isfinite(t)) or np.any(np.diff(t) <= 0):
            raise ValueError("%s: utterance %d: frame times must be finite and strictly increasing" % (where, u))


# ---- device --------------------------------------------------------------------------------------------------------
def interp_contour_device(rt, batch, tp_d, knot_off, time, value, voiced_rule=True):
    """wh_interp_contour on a resident batch: (f0_d, vuv_d) with the voiced rule, (values_d, None) without."""
    nf = batch.total_frames
    out = rt.empty((nf,))
    vuv = rt.empty((nf,)) if voiced_rule else None
    vp = ctypes.c_void_p
    _hip.check(rt.lib.wh_interp_contour(rt.ctx, rt.stream(), batch.handle, rt.ptr(tp_d),
                                        knot_off.ctypes.data_as(_hip._c_i64p), time.ctypes.data_as(vp),
                                        value.ctypes.data_as(vp), 1 if voiced_rule else 0, rt.ptr(out), rt.ptr(vuv)))
    return out, vuv


def regrid_rows_device(rt, src_batch, dst_batch, tp_src_d, tp_dst_d, rows_d, positive_rule=False, out=None):
    """wh_regrid_rows: a frame-major [F][K] tensor (or a per-frame [F] one) on the destination grid."""
    k = 1 if rows_d.dim() == 1 else int(rows_d.shape[1])
    if int(rows_d.shape[0]) != src_batch.total_frames or not rows_d.is_contiguous():
        raise ValueError("regrid: the tensor must be contiguous with one row per source frame (%d), got %s"
                         % (src_batch.total_frames, tuple(rows_d.shape)))
    if out is None:
        out = rt.empty((dst_batch.total_frames,) if rows_d.dim() == 1 else (dst_batch.total_frames, k))
    _hip.check(rt.lib.wh_regrid_rows(rt.ctx, rt.stream(), src_batch.handle, dst_batch.handle, rt.ptr(tp_src_d),
                                     rt.ptr(tp_dst_d), rt.ptr(rows_d), rt.ptr(out), k, 1 if positive_rule else 0))
    return out


def regrid_encoding(enc, frame_period):
    """BatchEncoding.regrid: see there."""
    from .batch import BatchEncoding

    rt = enc.rt
    fo = enc.batch.frame_off
    tp_h = enc.host_times()
    check_source_times(tp_h, fo)
    parts = [destination_times(tp_h[int(fo[u]):int(fo[u + 1])], frame_period) for u in range(enc.n_utt)]
    tp_dst_h = np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(0), dtype=np.float64)
    dst_off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    with rt.lock, rt.on_stream():
        nb = rt.make_batch(enc.batch.x_off, dst_off)
        tp_dst = rt.to_device(tp_dst_h)
        nb.tp_d, nb.tp_host, nb.frame_period = tp_dst, tp_dst_h, frame_period
        tp_src = enc.temporal_positions

        def move(t, positive=False):
            return None if t is None else regrid_rows_device(rt, enc.batch, nb, tp_src, tp_dst, t.contiguous(), positive)

        out = BatchEncoding(rt, nb, enc.fs, tp_dst.clone(), move(enc.f0, True), move(enc.vuv, True), move(enc.spectrogram),
                            move(enc.aperiodicity), enc.fft_size, enc.is_requiem, frame_period, tp_host=tp_dst_h.copy())
        out.coarse_ap, out.ap_gate = move(enc.coarse_ap), move(enc.ap_gate, True)
    return out
